"""The exact multiply (K4: sg_spgemm_topn.hip, spgemm_topn_kernel) on inputs built at the edges of its loops
(tests/_exact_edge_cases.py: posting segments of 1 .. 1345 entries and of a whole tile, chunks of a left row with 0 .. 64
segments, hits at the corners of the sweep, lists carried through tile groups and passes, ties whose row order and position
order disagree, many dissimilar rows a wave), compared BIT FOR BIT with the oracle's port: shape, indptr, indices, dtype and
data are equal or the test fails; no tolerance anywhere.  tests/test_exact_edge_cases_cpu.py shows without a GPU that the
inputs reach every edge and that a kernel wrong at one of them would change the answer.

One test per (family, dtype, tile size, permutation on / off); inside it SG_TILE_GROUP = 1, 2, 0 (a launch a tile, two tiles
then one, one launch) times the family's (top_n, threshold, sort) schedule, and the whole schedule once more on the same
index at SG_TILE_GROUP=1: the second results must be the first.  Before a result counts the test proves from ctx.stats()
that the exact kernel took the product one-sided (no pruned rows, no self-join form, nobody handed over: the statistic
``exact_rows`` counts the rows the PRUNED multiply hands on, none here) and that the products made are the census's sum of list
lengths -- K3 built the lists the case was designed for --, and from the downloaded table that the index is permuted exactly
when asked, by the rule the builder restates.

The self-join launch (spgemm_topn_selfjoin_rows_kernel) has a test of its own: one cosine-like matrix on both sides under the
switches of the exact-selfjoin line of tests/_threshold_cases.py (FORMS), top_n 1, 64, 65 and 128 -- the form ends there --,
proved by prune_rows == 0, prune_symmetric == 1 and exact_rows == n; then once more with a pair list of eight chunks
(SG_SYM_PAIR_CAP), where the form is called off and the one-sided kernel must give the same bits."""
import ctypes as C

import numpy as np
import pytest

from tests import _exact_edge_cases as E
from tests.test_multiply_threshold_gpu import assert_identical

pytestmark = pytest.mark.gpu

CASES = [(f, d, t, p) for f in E.FAMILIES for d in E.DTYPES for t in E.TILES for p in (False, True)]
IDS = [f"{f}-{np.dtype(d).name}-{t}-{'permuted' if p else 'row-order'}" for f, d, t, p in CASES]
SELF_CASES = [(d, t, p) for d in E.DTYPES for t in E.SELF_TILES for p in (False, True)]
SELF_IDS = [f"selfjoin-{np.dtype(d).name}-{t}-{'permuted' if p else 'row-order'}" for d, t, p in SELF_CASES]
ONE_SIDED = {"SG_PRUNE": "0", "SG_COLLAPSE": "0", "SG_COLLAPSE_LEFT": "0", "SG_EXACT_NATIVE": "0"}


def _upload_as_stored(ctx, m):
    """ctx.csr_from_scipy without its sort of the rows: one left row is in descending column order on purpose."""
    from string_grouper_amd import _native as N
    indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(m.indices, dtype=np.int32)
    data = np.ascontiguousarray(m.data)
    out = C.c_void_p()
    N.check(N.lib().sg_csr_from_host(ctx.h, m.shape[0], m.shape[1], N._ptr(indptr), N._ptr(indices), N._ptr(data),
                                     N.np_dtype_code(data.dtype), C.byref(out)))
    return N.Csr(ctx, out)


def _device_u32(ptr, n):
    import torch
    from string_grouper_amd import distributed as D
    return torch.as_tensor(D.DeviceTensorView(ptr, n, "<u4"), device=torch.device("cuda", 0)).cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("family,dtype,tile_cols,permute", CASES, ids=IDS)
def test_exact_kernel_equals_the_port_at_the_edges_of_its_loops(ctx, family, dtype, tile_cols, permute):
    n_cu = 4
    if family == "waves":
        import torch
        n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    case = E.build(family, dtype, tile_cols, permute, n_cu)
    n_left = case.A.shape[0]
    assert family != "waves" or n_left >= 4 * n_cu
    macs = E.census(case)["macs"] if family != "waves" else int(np.diff(case.lists.ptr)[case.A.indices].sum())
    for k, v in ONE_SIDED.items():
        ctx.set_option(k, v)
    if family == "waves":
        ctx.set_option("SG_WAVES_PER_CU", "1")
    dB = ctx.csr_from_scipy(case.B)
    dA = _upload_as_stored(ctx, case.A)
    post = ctx.postings_build(dB, tile_cols, permute=permute)
    assert ctx.postings_rows(post) == (case.n, case.n, 0)
    p_orig, p_pos = ctx.postings_permutation(post)
    assert (p_orig != 0) == permute, "the index is permuted exactly when asked"
    if permute:
        assert np.array_equal(_device_u32(p_orig, case.n), case.orig_of) and np.array_equal(_device_u32(p_pos, case.n), case.pos_of)
    want = {key: E.port(case, *key) for key in case.schedule}
    first = {}
    n = 0
    for group, again in ((1, False), (2, False), (0, False), (1, True)):
        ctx.set_option("SG_TILE_GROUP", str(group))
        for key in case.schedule:
            top_n, thr, sort = key
            res = ctx.spgemm_topn(dA, post, top_n, thr, sort)
            st = ctx.stats()
            got = res.to_scipy()
            res.free()
            what = (f"{family} {np.dtype(dtype).name} tile {tile_cols} permute={permute} SG_TILE_GROUP={group} top_n={top_n} thr={thr!r} "
                    f"sort={sort}{' (second run)' if again else ''}")
            # FIRST: which kernel ran, on which lists
            assert st["prune_rows"] == 0 and st["prune_symmetric"] == 0 and st["exact_rows"] == 0, f"{what}: another form ran: {st}"
            assert st["macs"] == macs, f"{what}: {st['macs']} products, the lists designed make {macs}"
            assert_identical(got, want[key], what)
            if again:
                assert_identical(got, first[key], what + " against the first run")
            elif group == 1:
                first[key] = got
            n += 1
    assert n == 4 * len(case.schedule)
    post.free()
    dA.free()
    dB.free()


@pytest.mark.parametrize("dtype,tile_cols,permute", SELF_CASES, ids=SELF_IDS)
def test_exact_selfjoin_launch_equals_the_port(ctx, dtype, tile_cols, permute):
    from tests import _threshold_cases as T
    case = E.build("selfjoin", dtype, tile_cols, permute)
    form = T.form("exact-selfjoin")
    # SG_EXACT_NATIVE=0: the tile the case was designed for is the one that runs
    for k, v in {**form.build, **form.run, "SG_COLLAPSE": "0", "SG_EXACT_NATIVE": "0"}.items():
        ctx.set_option(k, v)
    macs = E.census(case)["macs"]
    dA = ctx.csr_from_scipy(case.B)
    post = ctx.postings_build(dA, tile_cols, permute=permute)
    assert ctx.postings_rows(post) == (case.n, case.n, 0)
    p_orig, p_pos = ctx.postings_permutation(post)
    assert (p_orig != 0) == permute, "the index is permuted exactly when asked"
    if permute:
        assert np.array_equal(_device_u32(p_orig, case.n), case.orig_of) and np.array_equal(_device_u32(p_pos, case.n), case.pos_of)
    want = {key: E.port(case, *key) for key in case.schedule}
    first = {}
    for cap, again in ((None, False), (None, True), (8 * E.PAIR_CHUNK, False)):
        ctx.set_option("SG_SYM_PAIR_CAP", None if cap is None else str(cap))
        for key in case.schedule:
            top_n, thr, sort = key
            res = ctx.spgemm_topn(dA, post, top_n, thr, sort)
            st = ctx.stats()
            got = res.to_scipy()
            res.free()
            what = (f"selfjoin {np.dtype(dtype).name} tile {tile_cols} permute={permute} top_n={top_n} thr={thr!r} sort={sort}"
                    f"{' (second run)' if again else ''}{'' if cap is None else f' SG_SYM_PAIR_CAP={cap}'}")
            if cap is None:      # FIRST: the exact kernel in the self-join form, every row through its launch
                assert form.proof(st, dict(n=case.n)), f"{what}: another form ran: {st}"
            else:                # the pair list overran: the form was called off, the one-sided exact kernel took the product
                assert st["prune_rows"] == 0 and st["prune_symmetric"] == 0, f"{what}: the form was not called off: {st}"
            assert st["macs"] == macs, f"{what}: {st['macs']} products, the lists designed make {macs}"
            assert_identical(got, want[key], what)
            if again:
                assert_identical(got, first[key], what + " against the first run")
            elif cap is None:
                first[key] = got
    post.free()
    dA.free()
