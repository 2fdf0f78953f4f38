"""Every form of the top-n multiply (tests/_threshold_cases.py: FORMS) on matrices whose ROW NORMS ARE NOT 1
(tests/_offnorm_cases.py), compared BIT FOR BIT with the oracle's port: shape, indptr, indices, dtype and data are equal or
the test fails; no tolerance anywhere.  What is under test beside the two rules (strictly greater than the threshold; score
descending, then column ascending) is the SCALE: norm_up, the largest row norm of the right-hand matrix rounded up, which
K3 divides every quantised bound of the index by (bq, fq, b24, the 8-bit records) and K4p multiplies by (c_a, c1, C16, the
budget of the suffix, q8_scale).  Everything else the suite multiplies has norm_up = 1.000001, where the two cannot disagree.

  three_quarter  norm_up ~ 0.75, every score 9k/1024; self-product
  mixed          norms 1, 1/2 and 1/4 in one matrix, scores k/1024; self-product
  half_right     unit rows against rows of norm 1/2 (norm_up ~ 0.5, the left values unscaled); one-sided only
  half_left      rows of norm 1/2 against unit rows (the scale on the left alone); one-sided only
  band           TF-IDF rows x 1.00004: squared norms in the gate's band (1, 1.0001], norm_up > 1, inexact products,
                 thresholds from the port's own scores -- two of them above 1 -- and plain 1.0

Each form is forced with context options and must PROVE from ctx.stats() that it ran before its result counts.  Each runs
two ways -- (identical rows not grouped, the index over the library's row permutation) and (grouped, in row order); the
other two combinations are covered at norm 1 by tests/test_multiply_threshold_gpu.py and add nothing about scale -- and the
forms that can be one-sided also with a slice of the rows (1000:3000; the band 500:3500) as a left matrix of its own.

The ladder is larger than a seventh of tests/_threshold_cases.py's (12 x 150 + 4 000 = 5 812 rows) because two forms
could not be reached on that, whatever the switches (tests/_offnorm_cases.py has the counts):
  * 6 381 filler rows, 8 313 rows in all (the band: 8 400 names): the index build permutes the rows -- and writes the
    packed rows and the 8-bit records, which the scale goes into, along with the copy -- only for more than two tiles of
    them, 8 192 for the pruned kernels' index: on fewer no pruned form runs "over the row permutation";
  * 160 candidates per anchor: with 150 no row of half_right / half_left has 64 DISTINCT matches at 0.4375 (58 at most),
    so with identical rows grouped no list comes out full and full-lists-handed-on cannot prove itself.
tests/test_offnorm_cases_cpu.py counts, without a GPU, the rows that fill a list in every case, grouped or not.
tests/test_offnorm_cases_cpu.py shows without a GPU that the port's answer on these inputs is the arithmetic one and that a
broken rule changes it; tests/test_prune_model.py that the filters' formulas lose no match at these scales and that
quantising against another norm than the multiply's does."""
import numpy as np
import pytest

from tests import _offnorm_cases as F
from tests import _threshold_cases as T
from tests.test_multiply_threshold_gpu import _assemble, assert_identical

pytestmark = pytest.mark.gpu

WAYS = (("0", True), ("1", False))          # (SG_COLLAPSE, index over the row permutation)


def own_threshold(case: str, dtype) -> float:
    """the one threshold per case at which the forms about cuts beyond 64 run, and sort=False: the lowest (rows with 64
    matches and more -- tests/test_offnorm_cases_cpu.py)"""
    return min(F.thresholds(case, dtype))


def schedule(form: T.Form, case: str, dtype):
    """[(top_n, thr, sort)] of a form on a case: cuts 5 and 64 at every threshold (t and the number below t), or the form's
    own cuts (65 .. 128, 129+) at the case's lowest threshold; sort=False once."""
    own = own_threshold(case, dtype)
    if form.cuts is not None:
        return [(c, own, True) for c in form.cuts] + [(form.cuts[0], own, False)]
    return [(c, thr, True) for thr in F.thresholds(case, dtype) for c in F.CUTS_EVERYWHERE] + [(F.CUTS_EVERYWHERE[0], own, False)]


def products(ctx, form: T.Form, case: str, dtype):
    """Run the form's schedule both ways; yields (what, proof holds, stats, info, got, want) per multiply."""
    one_sided_only = case in ("half_right", "half_left")
    _, B = F.operands(case, dtype)
    sched = schedule(form, case, dtype)
    for collapse, permute in WAYS:
        ctx.reset_options()
        for k, v in {**form.build, **form.run, "SG_COLLAPSE": collapse}.items():
            ctx.set_option(k, v)
        if collapse == "1":
            ctx.set_option("SG_COLLAPSE_LEFT", "1")
        dB = ctx.csr_from_scipy(B)
        post = ctx.postings_build(dB, permute=permute)
        n_index, n_caller, _ = ctx.postings_rows(post)
        assert n_caller == B.shape[0]
        assert (n_index < n_caller) == (collapse == "1") and (n_index == n_caller) == (collapse == "0")
        assert n_index > T.TILE_ROWS and (ctx.postings_permutation(post)[0] != 0) == permute      # a tile boundary is crossed
        lefts = []
        if not one_sided_only:
            lefts.append((None, dB, B.shape[0]))
        if not form.self_join:
            L = F.operands(case, dtype, None if one_sided_only else F.left_slice(case))[0]
            lefts.append((F.left_slice(case), ctx.csr_from_scipy(L), L.shape[0]))
        for rows, dL, n_left in lefts:
            for top_n, thr, sort in sched:
                res = ctx.spgemm_topn(dL, post, top_n, thr, sort)
                st = ctx.stats()
                got = res.to_scipy()
                res.free()
                info = dict(n=n_index if rows is None else n_left, n_left=n_left, long_rows=0, top_n=top_n, thr=thr)
                what = (f"{form.name} {case} {np.dtype(dtype).name} SG_COLLAPSE={collapse} permute={permute} "
                        f"{'self-product' if rows is None else 'one-sided'} top_n={top_n} thr={thr!r} sort={sort}")
                want = F.port(case, dtype, top_n, thr, sort, 0, None if one_sided_only else rows)
                yield what, bool(form.proof(st, info)), st, info, got, want
        for rows, dL, _ in lefts:
            if rows is not None:
                dL.free()
        post.free()
        dB.free()


@pytest.mark.parametrize("dtype", F.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name,case", [(f.name, c) for f in T.FORMS for c in F.CASES if c in F.SELF_CASES or not f.self_join])
def test_form_equals_the_port_off_the_unit_norm(ctx, name, case, dtype):
    """One line of FORMS on one case: every threshold of the case with thr = t (the pairs at t are no matches) and thr =
    the number below t (they are, by one ulp) at cuts 5 and 64; the forms about cuts beyond 64 with their own cuts at the
    case's lowest threshold; sort=False once.  Two ways, the one-sided forms also with a slice of the rows as the left
    matrix; half_right / half_left are one-sided products and run the forms without self_join only."""
    form = T.form(name)
    n = 0
    for what, proved, st, info, got, want in products(ctx, form, case, dtype):
        keys = ("prune_rows", "prune_symmetric", "exact_rows", "prune_survivors", "prune_scored")
        assert proved, f"{what}: another form ran: { {k: st[k] for k in keys} } {info}"      # FIRST: which form ran
        assert_identical(got, want, what)
        n += 1
    lefts = 1 if (form.self_join or case not in F.SELF_CASES) else 2
    assert n == len(WAYS) * lefts * len(schedule(form, case, dtype))


@pytest.mark.parametrize("dtype", F.DTYPES, ids=lambda d: np.dtype(d).name)
def test_row_ranges_of_the_selfjoin_form_on_mixed_norms(ctx, dtype):
    """sg_selfjoin_range / sg_selfjoin_merge with three ranks played one after the other on `mixed` (norms 1, 1/2, 1/4):
    three contiguous ranges and three interleaved shares, top_n 10 at the number below 0.4375 (hundreds of pairs at exactly
    0.4375 are matches by one ulp, hundreds of rows are cut inside a block of equal scores), the ranks' pair lists
    concatenated in rank order and with every record in REVERSE order.  The rows put together are the port's."""
    import torch
    from string_grouper_amd import distributed as D
    from string_grouper_amd.vectorizer import HipTfidfVectorizer
    A = F.mixed(dtype)
    n = A.shape[0]
    thr, top_n = F.pred(0.4375, dtype), 10
    ops = D.HipOps(ctx, lambda: HipTfidfVectorizer(dtype=dtype, ctx=ctx))
    ctx.set_option("SG_COLLAPSE", "0")
    ctx.set_option("SG_PRUNE_MIN_THRESHOLD", "0.25")     # (the bar of the pruned kernels is a tuning: 0.45 by default)
    dA = ctx.csr_from_scipy(A)
    world = 3
    bounds = D.selfjoin_row_ranges(n, world)
    want = F.port("mixed", dtype, top_n, thr)
    for permute in (True, False):
        post = ctx.postings_build(dA, permute=permute)
        assert ctx.postings_rows(post) == (n, n, 0) and (ctx.postings_permutation(post)[0] != 0) == permute
        layouts = {"contiguous": [(int(bounds[r]), int(bounds[r + 1]), 1) for r in range(world)],
                   "interleaved": [(0, n - r, world) for r in range(world)]}
        for layout, shares in layouts.items():
            for reverse in (False, True):
                parts = [ops.selfjoin_range(dA, post, top_n, thr, *sh) for sh in shares]
                assert all(p is not None for p in parts), "the self-join form did not take the range"
                assert ctx.stats()["prune_symmetric"] == 1 and ctx.stats()["prune_rows"] > 0
                words = parts[0].words
                pairs_all = torch.cat([ops.selfjoin_pairs(p).clone() for p in parts])
                assert pairs_all.numel() > 0 and pairs_all.numel() % words == 0
                if reverse:
                    pairs_all = pairs_all.view(-1, words).flip(0).contiguous().view(-1)
                blocks = [ops.selfjoin_merge(parts[r], pairs_all, *shares[r]) for r in range(world)]
                got = _assemble(blocks, n, min(top_n, n), dtype, n)
                for b in blocks:
                    b.free()
                assert_identical(got, want, f"{layout} reverse={reverse} permute={permute}")
        post.free()
    dA.free()
