"""What the top-n multiply chooses ON ITS OWN -- no form switch set -- proved from ctx.stats() the way
tests/test_multiply_threshold_gpu.py proves the forms it forces.  66 000 synthetic names vectorised by the library, f32,
identical rows not grouped (SG_COLLAPSE=0: rows are rows), the index as postings_build makes it; four products on the four
sides of the bars of csrc/sg_plan.h that a product of this size can reach on a GPU in milliseconds:

  self-join, 0.8, top 10          66 000 rows >= 65 536: the pruned kernel in the self-join form
  rows 0 .. 40 000 x index, 0.8   a matrix of its own is no self-join: the pruned kernel, one-sided
  self-join, 0.3, top 10          below 0.40: the exact kernel, in the self-join form (66 000 >= 16 384), every row
  self-join, 0.8, top 129         more than two register lists: the exact kernel, one-sided

Each result is the same product's under SG_PRUNE=0, SG_SYM=0 (the one-sided exact kernel), bit for bit.
tests/test_multiply_plan_cpu.py holds every bar of the rule at the bar and one step under it, without a GPU."""
import numpy as np
import pytest

from string_grouper_amd.synth import synth_names

pytestmark = pytest.mark.gpu

N_ROWS = 66000
N_LEFT = 40000


def test_the_form_the_library_chooses_with_no_switch_set(ctx):
    from string_grouper_amd.vectorizer import HipTfidfVectorizer
    ctx.set_option("SG_COLLAPSE", "0")
    names = synth_names(N_ROWS, seed=11)
    vec = HipTfidfVectorizer(dtype=np.float32, ctx=ctx)
    p = vec.prepare(names)
    vec.fit_prepared([p])
    dA = vec.transform_prepared(p)
    dL = ctx.csr_from_scipy(dA.to_scipy()[:N_LEFT])
    post = ctx.postings_build(dA)
    assert ctx.postings_rows(post)[:2] == (N_ROWS, N_ROWS)
    products = (("self-join 0.8 top 10", dA, 10, 0.8, lambda st: st["prune_rows"] > 0 and st["prune_symmetric"] == 1),
                ("rows 0 .. 40 000 x index 0.8 top 10", dL, 10, 0.8, lambda st: st["prune_rows"] > 0 and st["prune_symmetric"] == 0),
                ("self-join 0.3 top 10", dA, 10, 0.3,
                 lambda st: st["prune_rows"] == 0 and st["prune_symmetric"] == 1 and st["exact_rows"] == N_ROWS),
                ("self-join 0.8 top 129", dA, 129, 0.8, lambda st: st["prune_rows"] == 0 and st["prune_symmetric"] == 0))
    for what, left, top_n, thr, proof in products:
        res = ctx.spgemm_topn(left, post, top_n, thr, True)
        st = ctx.stats()
        got = res.to_scipy()
        res.free()
        keys = ("prune_rows", "prune_symmetric", "exact_rows")
        print(what, {k: st[k] for k in keys})
        assert proof(st), f"{what}: another form ran: { {k: st[k] for k in keys} }"
        ctx.set_option("SG_PRUNE", "0")
        ctx.set_option("SG_SYM", "0")
        ref = ctx.spgemm_topn(left, post, top_n, thr, True)
        st = ctx.stats()
        assert st["prune_rows"] == 0 and st["prune_symmetric"] == 0, f"{what}: the reference product is not the one-sided exact kernel's: {st}"
        want = ref.to_scipy()
        ref.free()
        ctx.set_option("SG_PRUNE", None)
        ctx.set_option("SG_SYM", None)
        assert got.shape == want.shape and got.nnz > 0, what
        assert np.array_equal(got.indptr, want.indptr), f"{what}: match counts differ"
        assert np.array_equal(got.indices, want.indices), f"{what}: match columns differ"
        assert got.data.dtype == want.data.dtype and np.array_equal(got.data, want.data), f"{what}: scores differ"
    post.free()
    dL.free()
    dA.free()
