"""The second filter's early exit on the GPU (sg_spgemm_pruned.hip: q8_passes; the rest norms: sg_postings.hip, both record
writers and the in-place rewrite): the stream forms with the second filter forced on, on tests/_q8_early_cases.py's built
matrix -- ten thousand rows, more than two tiles; left rows whose candidates (by the restated first filter) have records of
1 .. 60 entries that leave at every stored boundary or at none, candidates beyond 60 entries (no copy), left rows of 65 .. 128
terms (the wide launch) and of norm 1/2 (tests/test_q8_early_exit_cpu.py checks that the matrix holds them).  Results equal the
port BIT FOR BIT with the switch SG_Q8_EARLY=0 (every rest norm written as unknown: no lane leaves early) and without it, and
prune_survivors, prune_scored and out_nnz are equal between the two.  The index is built both ways: over the library's row
permutation (gather_rows_kernel writes the records) and in row order (q8_pack_kernel does).

The two settings are compared on ONE built index: the switch holds for the multiplies that follow it, and an index built under
the other setting has its rest norms re-written in place (sg_postings_sync_q8_early) -- in both directions here, so the norms
the rewrite computes are used as well as the writers'.  Two BUILDS cannot be compared that way: the fill places a segment's
postings by atomic counters, their order moves the first filter's false alarms, and prune_survivors / prune_scored differ
between two builds under equal settings, before this change as after it (this matrix, stream-selfjoin, float32, 0.8, MI355X:
(100848, 2657) and (100839, 2660) with the library of the commit before; one built index gives the same figures every time)."""
import numpy as np
import pytest

from tests import _q8_early_cases as Q
from tests import _threshold_cases as T
from tests.test_multiply_threshold_gpu import assert_identical

pytestmark = pytest.mark.gpu

TOP_N = 10
FORMS = ["stream-selfjoin", "stream-one-sided-q8"]
KEYS = ("prune_survivors", "prune_scored", "out_nnz")
_PORT = {}


def port(dtype, thr):
    from oracle import port as P
    key = (np.dtype(dtype).name, thr)
    if key not in _PORT:
        m, _ = Q.built(dtype)
        _PORT[key] = P.sp_matmul_topn_port(m, m.T, TOP_N, thr, True, 8)
    return _PORT[key]


@pytest.mark.parametrize("dtype", T.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", FORMS)
def test_early_exit_changes_no_result_and_no_statistic(ctx, name, dtype):
    form = T.form(name)
    m, _ = Q.built(dtype)
    n_long = int((np.diff(m.indptr) > 128).sum())
    n = 0
    for permute in (True, False):
        for built_with, then in (("1", "0"), ("0", "1")):
            ctx.reset_options()
            for k, v in {**form.build, **form.run, "SG_COLLAPSE": "0", "SG_Q8_EARLY": built_with}.items():
                ctx.set_option(k, v)
            dA = ctx.csr_from_scipy(m)
            post = ctx.postings_build(dA, permute=permute)
            assert (ctx.postings_permutation(post)[0] != 0) == permute
            seen = {}
            for early in (built_with, then):
                ctx.set_option("SG_Q8_EARLY", early)
                for thr in Q.THRESHOLDS:
                    res = ctx.spgemm_topn(dA, post, TOP_N, thr, True)
                    st = ctx.stats()
                    got = res.to_scipy()
                    res.free()
                    what = f"{name} {np.dtype(dtype).name} permute={permute} built with SG_Q8_EARLY={built_with}, run with {early}, thr={thr}"
                    info = dict(n=m.shape[0], n_left=m.shape[0], long_rows=n_long, top_n=TOP_N, thr=thr)
                    assert form.proof(st, info), f"{what}: another form ran: {st}"
                    assert st["prune_scored"] < st["prune_survivors"], f"{what}: the second filter rejected nothing: {st}"
                    assert_identical(got, port(dtype, thr), what)
                    assert st["out_nnz"] == port(dtype, thr).nnz, what
                    seen[(early, thr)] = [st[k] for k in KEYS]
            for thr in Q.THRESHOLDS:
                print(name, np.dtype(dtype).name, permute, built_with, thr, seen[("1", thr)], seen[("0", thr)])
                assert seen[("1", thr)] == seen[("0", thr)], (name, permute, built_with, thr)
                n += 1
            post.free()
            dA.free()
    assert n == 4 * len(Q.THRESHOLDS)
