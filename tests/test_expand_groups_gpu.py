"""The expansion of grouped results on inputs built at its edges (tests/_expand_cases.py): expand_simple_kernel and
expand_merge_kernel of sg_collapse.hip -- runs of 2, 3, 63, 64, 65, 66, 128 and 200 tying groups, the cut inside a run, at its
end and before it, more queued rows than the merge kernel has workgroups, calls that queue none --, through every entry point
that ends in them, and expand_left_rows_kernel of sg_spgemm_topn.hip.  BIT FOR BIT, float32 and float64: counts, columns,
values and the result's stride are the statement's (``ref_expand``) or the port's on the ungrouped matrices, or the test
fails; no tolerance anywhere.  tests/test_expand_cases_cpu.py shows without a GPU that the inputs reach every edge and that a
kernel wrong at one of them would change an answer; a failure here names the row's kind, as that test names it.

  - sg_topn_expand_groups called directly at every stride: all rows, an ascending subset, a shuffled list, one row, a list
    whose rows queue nothing; every call twice, the result over groups unchanged afterwards;
  - sg_topn_expand_range over the permuted and the row-order index: whole, empty, one position, the shares of 2, 3 and 8 ranks;
  - sg_spgemm_topn one-sided (no row -> group table in the kernels) at top_n 1, 2, 10, 64, 65 and 128, unsorted once, the
    repeated left rows under SG_COLLAPSE_LEFT=1, and the same products with SG_COLLAPSE=0; the self-join of the layout whose
    groups score against each other, where the groups are fewer than top_n;
  - the refusals, each followed by a good call."""
import numpy as np
import pytest

from oracle import port as P
from tests import _expand_cases as X
from tests._numpy_ops import NumpyOps
from tests.test_parity_gpu import _device_u32, assert_csr_identical
from tests.test_postings_build_paths_gpu import _options

pytestmark = pytest.mark.gpu

DT = lambda d: np.dtype(d).name


class _Device:
    """the layout on the device and its three indices: over groups (permuted, in row order) and over all rows"""

    def __init__(self, ctx, dtype):
        self.L = X.layout(dtype)
        self.dA = ctx.csr_from_scipy(self.L.A)
        with _options(ctx, {"SG_COLLAPSE": "1"}):
            self.permuted = ctx.postings_build(self.dA, X.TILE, permute=True)
            self.row_order = ctx.postings_build(self.dA, X.TILE, permute=False)
        with _options(ctx, {"SG_COLLAPSE": "0"}):
            self.plain = ctx.postings_build(self.dA, X.TILE, permute=True)

    def free(self):
        for h in (self.permuted, self.row_order, self.plain, self.dA):
            h.free()


@pytest.fixture(scope="module")
def dev(_session_ctx):
    made = {}

    def get(dtype):
        key = np.dtype(dtype).type
        if key not in made:
            made[key] = _Device(_session_ctx, key)
        return made[key]

    yield get
    for d in made.values():
        d.free()
    _session_ctx.reset_options()


_WANT = {}


def _want_all(cs):
    """the statement for every row of a case: computed once, never changed"""
    key = (cs.dtype, cs.S)
    if key not in _WANT:
        _WANT[key] = X.ref_expand(cs.L, None, cs.cols, cs.vals, cs.counts, min(cs.S, cs.L.n))
        for a in _WANT[key]:
            a.setflags(write=False)
    return _WANT[key]


def _assert_rows(cs, got, want, rows, what):
    """counts, columns and the values' bits up to the counts; the message names the first row that differs and its kind"""
    assert got[0].shape == want[0].shape and got[1].dtype == want[1].dtype, f"{what}: {got[0].shape} {got[1].dtype}, want {want[0].shape}"
    mask = np.arange(want[0].shape[1])[None, :] < want[2][:, None]
    bits = f"u{want[1].itemsize}"
    differs = (got[2] != want[2]) | ((got[0] != want[0]) & mask).any(axis=1) | ((got[1].view(bits) != want[1].view(bits)) & mask).any(axis=1)
    if differs.any():
        k = int(np.flatnonzero(differs)[0])
        row = k if rows is None else int(rows[k])
        kind = cs.names[cs.kind_of_group[cs.L.gid[row]]]
        n = int(want[2][k])
        raise AssertionError(f"{what}: {int(differs.sum())} rows differ; the first is output row {k} = row {row}, kind '{kind}' "
                             f"({'queued' if cs.row_queued[row] else 'kept'}): count {int(got[2][k])} want {n}\n"
                             f"  columns {got[0][k, :n].tolist()}\n  want    {want[0][k, :n].tolist()}\n"
                             f"  values  {got[1][k, :n].tolist()}\n  want    {want[1][k, :n].tolist()}")


@pytest.mark.parametrize("S", X.STRIDES)
@pytest.mark.parametrize("dtype", X.DTYPES, ids=DT)
def test_expand_groups_called_directly(ctx, dev, dtype, S):
    from string_grouper_amd import _native as N
    cs, d = X.case(dtype, S), dev(dtype)
    L, post = cs.L, d.permuted
    n_index, n_caller, p_gid = ctx.postings_rows(post)
    assert (n_index, n_caller) == (L.n_groups, L.n) and p_gid, "the index is over groups"
    ctx.sync()
    np.testing.assert_array_equal(_device_u32(p_gid, L.n), L.gid)
    queued = X.census(cs)["queued_rows"]        # one call queues more rows than the merge kernel has workgroups, one queues none
    assert queued["none-queued"] == 0 and (S == 1 or queued["all"] > X.MERGE_BLOCKS), queued
    groups = ctx.topn_from_host(cs.cols, cs.vals, cs.counts, L.n_groups)
    want_all = _want_all(cs)
    for which, rows in cs.row_lists.items():
        d_rows = None if rows is None else (ctx.upload_ints(rows) if which == "shuffled" else ctx.upload_sorted_ints(rows))
        want = want_all if rows is None else tuple(a[rows] for a in want_all)
        for run in ("first", "second"):
            what = f"{DT(dtype)} stride {S} rows '{which}' ({queued[which]} queued), {run} run"
            out = ctx.topn_expand_groups(post, groups, d_rows.ptr if d_rows else 0, len(d_rows) if d_rows else 0)
            assert out.dims() == (len(want[2]), min(S, L.n), N.np_dtype_code(dtype), L.n), f"{what}: {out.dims()}"
            got = out.to_host()
            out.free()
            _assert_rows(cs, got, want, rows, what)
        if d_rows:
            d_rows.free()
    back = groups.to_host()
    groups.free()
    assert np.array_equal(back[0], cs.cols) and back[1].tobytes() == cs.vals.tobytes() and np.array_equal(back[2], cs.counts), \
        "the result over groups was changed"


@pytest.mark.parametrize("permute", [True, False], ids=["permuted", "row-order"])
@pytest.mark.parametrize("dtype", X.DTYPES, ids=DT)
def test_expand_range(ctx, dev, dtype, permute):
    d = dev(dtype)
    L, post = d.L, d.permuted if permute else d.row_order
    n_u = L.n_groups
    assert ctx.postings_rows(post)[:2] == (n_u, L.n)
    p_orig, p_pos = ctx.postings_permutation(post)
    assert (p_orig != 0) == (p_pos != 0) == permute, "the index is permuted exactly when asked"
    pos_of = None
    if permute:
        ctx.sync()
        pos_of = _device_u32(p_pos, n_u)
        assert np.array_equal(pos_of, NumpyOps.permutation(n_u)[1]) and not np.array_equal(pos_of, np.arange(n_u))
    hub = int(L.group_of_type[L.t["h1000"]])
    ranges = [(0, n_u, 1), (0, 0, 1), (n_u, n_u, 1), (0, 1, 1), (n_u - 1, n_u, 1)]
    ranges += [(k, k + 1, 1) for k in (int(pos_of[hub]) if permute else hub, n_u // 2)]
    ranges += [(0, n_u - r, world) for world in (2, 3, 8) for r in range(world)]
    for S in (10, 200):
        cs = X.case(dtype, S)
        groups = ctx.topn_from_host(cs.cols, cs.vals, cs.counts, n_u)
        want_all = _want_all(cs)
        shares = {}
        for lo, hi, step in ranges:
            what = f"{DT(dtype)} {'permuted' if permute else 'row order'} stride {S} range ({lo}, {hi}, {step})"
            out, d_rows = ctx.topn_expand_range(post, groups, lo, hi, step)
            rows = ctx.download_ints(d_rows).astype(np.int64)
            got = out.to_host()
            out.free()
            d_rows.free()
            assert (np.diff(rows) > 0).all(), f"{what}: the rows do not ascend"
            np.testing.assert_array_equal(rows, X.range_rows(L, pos_of, lo, hi, step), err_msg=what)
            assert (len(rows) == 0) == (lo == hi)
            _assert_rows(cs, got, tuple(a[rows] for a in want_all), rows, what)
            if step > 1:
                shares.setdefault(step, []).append(rows)
        for world, parts in shares.items():
            assert len(parts) == world and np.array_equal(np.sort(np.concatenate(parts)), np.arange(L.n)), \
                f"the shares of {world} ranks are not disjoint or do not cover every row"
        groups.free()


def _multiply(ctx, dA, post, top_n, thr, sort=True, products=None, what=""):
    res = ctx.spgemm_topn(dA, post, top_n, thr, sort)
    st = ctx.stats()
    got = res.to_scipy()
    res.free()
    assert products is None or st["macs"] == products, f"{what}: {st['macs']} products, not {products}"
    return got


@pytest.mark.parametrize("top_n", X.TOP_NS)
@pytest.mark.parametrize("dtype", X.DTYPES, ids=DT)
def test_one_sided_products_through_the_multiply(ctx, dev, dtype, top_n):
    d = dev(dtype)
    L = d.L
    assert ctx.postings_rows(d.permuted)[0] == L.n_groups and ctx.postings_rows(d.plain) == (L.n, L.n, 0)
    A, names = X.left_matrix(dtype)
    R, _ = X.repeated(A, names)
    for left, opts, how in ((A, {}, "left rows"), (R, {"SG_COLLAPSE_LEFT": "1"}, "repeated left rows, SG_COLLAPSE_LEFT=1")):
        what = f"{DT(dtype)} top_n {top_n} {how}"
        want = P.sp_matmul_topn_port(left, L.A.T, top_n, X.THRESHOLD, True, 4)      # the port on the FULL matrices
        dL = ctx.csr_from_scipy(left)
        with _options(ctx, opts):
            # FIRST what ran: every column of the index over groups lists ONE group, so the products made are the entries of
            # the left rows multiplied -- those of the 114 distinct rows when the repeated ones were grouped
            got = _multiply(ctx, dL, d.permuted, top_n, X.THRESHOLD, products=A.nnz, what=what)
            assert_csr_identical(got, want, what)
            if top_n == 10:      # unsorted: every row by ascending column
                by_column = want.copy()
                by_column.sort_indices()
                assert_csr_identical(_multiply(ctx, dL, d.permuted, top_n, X.THRESHOLD, sort=False), by_column, what + " sort=False")
        dL.free()
        dL = ctx.csr_from_scipy(left)        # (a matrix of its own: groups stay with the matrix they were made for)
        with _options(ctx, {"SG_COLLAPSE": "0"}):
            assert_csr_identical(_multiply(ctx, dL, d.plain, top_n, X.THRESHOLD), got, what + " against SG_COLLAPSE=0")
        dL.free()


@pytest.mark.parametrize("dtype", X.DTYPES, ids=DT)
def test_self_join_with_fewer_groups_than_top_n(ctx, dtype):
    """70 groups in 134 rows, every group 0.25 from every other: a run of 69 in every row, and rows of up to 128 columns from
    a result over groups that has 70."""
    V = X.variant(dtype)
    dV = ctx.csr_from_scipy(V.A)
    with _options(ctx, {"SG_COLLAPSE": "1"}):
        post = ctx.postings_build(dV)
        n_index, n_caller, p_gid = ctx.postings_rows(post)
        assert (n_index, n_caller) == (V.n_groups, V.n) and p_gid
        ctx.sync()
        np.testing.assert_array_equal(_device_u32(p_gid, V.n), V.gid)
        for top_n in X.TOP_NS:
            want = P.sp_matmul_topn_port(V.A, V.A.T, top_n, X.VARIANT_THRESHOLD, True, 4)
            assert_csr_identical(_multiply(ctx, dV, post, top_n, X.VARIANT_THRESHOLD), want, f"{DT(dtype)} top_n {top_n}")
        post.free()
    dV.free()


@pytest.mark.parametrize("dtype", X.DTYPES, ids=DT)
def test_refusals_each_followed_by_a_good_call(ctx, dev, dtype):
    d, cs = dev(dtype), X.case(dtype, 10)
    L, n_u = d.L, d.L.n_groups
    groups = ctx.topn_from_host(cs.cols, cs.vals, cs.counts, n_u)
    want_all = _want_all(cs)

    def good(after):
        out = ctx.topn_expand_groups(d.permuted, groups)
        got = out.to_host()
        out.free()
        _assert_rows(cs, got, want_all, None, f"{DT(dtype)} the call after {after}")

    def good_range(after):
        out, d_rows = ctx.topn_expand_range(d.permuted, groups, 0, n_u, 1)
        got, rows = out.to_host(), ctx.download_ints(d_rows)
        out.free()
        d_rows.free()
        assert np.array_equal(rows, np.arange(L.n))
        _assert_rows(cs, got, want_all, None, f"{DT(dtype)} the range after {after}")

    with pytest.raises(ValueError, match="not built over groups"):
        ctx.topn_expand_groups(d.plain, groups)
    good("an index without groups")
    with pytest.raises(ValueError, match="not built over groups"):
        ctx.topn_expand_range(d.plain, groups, 0, n_u, 1)
    good_range("an index without groups")
    short = ctx.topn_from_host(cs.cols[:-1], cs.vals[:-1], cs.counts[:-1], n_u)
    with pytest.raises(ValueError, match="one row per group"):
        ctx.topn_expand_groups(d.permuted, short)
    with pytest.raises(ValueError, match="one row per group"):
        ctx.topn_expand_range(d.permuted, short, 0, n_u - 1, 1)
    short.free()
    good("a result with a row too few")
    other = ctx.topn_from_host(cs.cols, cs.vals.astype(np.float64 if np.dtype(dtype) == np.float32 else np.float32), cs.counts, n_u)
    with pytest.raises(ValueError, match="value type"):
        ctx.topn_expand_groups(d.permuted, other)
    other.free()
    good("the other value type")
    too_many = ctx.upload_ints(np.zeros(L.n + 1, np.int64))       # (every number a row of the matrix: only the length is wrong)
    with pytest.raises(ValueError, match="more rows than the matrix has"):
        ctx.topn_expand_groups(d.permuted, groups, too_many.ptr, len(too_many))
    too_many.free()
    good("more rows than the matrix has")
    for lo, hi in ((0, n_u + 1), (5, 4), (-1, 3)):
        with pytest.raises(ValueError, match="outside the groups"):
            ctx.topn_expand_range(d.permuted, groups, lo, hi, 1)
        good_range(f"the range ({lo}, {hi})")
    groups.free()
