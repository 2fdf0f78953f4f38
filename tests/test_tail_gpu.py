"""The kernels that run after the multiply, each called directly through the C ABI on the constructed inputs of
tests/_tail_cases.py and compared BIT FOR BIT with the plain references there (numpy / scipy / pandas doing what the
reference project does): K5 sg_topn_zip, K6 sg_matchlist_build, K7 sg_matchlist_best_master, K8 sg_matchlist_group_reps,
K9 sg_csr_rowwise_dot, and sg_row_costs.  No tolerance anywhere: counts, columns, values, dtype and shape are equal or the
test fails.  tests/test_tail_references_cpu.py shows, without a GPU, that these inputs tell each reference from the same
reference with one thing wrong (summation order, accumulator width, tie rule, connectivity, the zip's floor, kept zeros)."""
import numpy as np
import pytest

from tests import _tail_cases as T

pytestmark = pytest.mark.gpu


def upload(ctx, t: T.TopN):
    return ctx.topn_from_host(t.cols, t.vals, t.counts, t.n_cols)


def assert_topn_equal(got, want: T.TopN):
    """got: a device result; equal shape, stride, dtype, counts, and the stored cells of every row."""
    n, stride = want.cols.shape
    assert got.dims() == (n, stride, 1 if want.vals.dtype == np.float64 else 0, want.n_cols)
    cols, vals, counts = got.to_host()
    assert cols.shape == (n, stride) and cols.dtype == np.int32 and vals.dtype == want.vals.dtype
    assert counts.dtype == np.int32 and np.array_equal(counts, want.counts)
    mask = np.arange(stride)[None, :] < want.counts[:, None]
    assert np.array_equal(cols[mask], want.cols[mask])
    assert np.array_equal(vals[mask], want.vals[mask])


def assert_list_equal(got, want: T.CsrList):
    row_ptr, cols, vals = got.to_host()
    assert got.dims() == (len(want.row_ptr) - 1, len(want.cols), 1 if want.vals.dtype == np.float64 else 0)
    assert row_ptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == want.vals.dtype
    assert np.array_equal(row_ptr, want.row_ptr)
    assert np.array_equal(cols, want.cols)
    assert np.array_equal(vals, want.vals)


# ---------------------------------------------------------------------------------------------------- K5
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", T.ZIP_CASES)
def test_zip_equals_reference_at_every_cut(ctx, name, dtype):
    """1, 2, 5 and 9 parts of unequal strides (one without entries, rows empty everywhere, rows filled beyond 64), equal
    scores across entries 63 / 64 / 65 and 127 / 128, parts that arrive unsorted, parts in descending column order; cut
    inside the first pass of 64, at its end, inside and at the end of the second, in the third, and above all strides."""
    case = T.zip_case(name, dtype)
    parts = [upload(ctx, p) for p in case.parts]
    for top_n in T.ZIP_TOP_N + (1000,):
        want = T.ref_zip(case, top_n)
        assert want.cols.shape[1] == min(top_n, sum(p.cols.shape[1] for p in case.parts))
        assert_topn_equal(ctx.topn_zip(parts, case.offsets, top_n), want)


# ---------------------------------------------------------------------------------------------------- K6
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True), (True, True)], ids=["plain", "diag", "sym", "diag+sym"])
@pytest.mark.parametrize("name", T.MATCHLIST_SQUARE)
def test_matchlist_build_square(ctx, name, flags, dtype):
    """Stored diagonals that are not 1, rows filled to the stride, empty rows, one-directional and two-sided pairs; a hub
    column listed by 20 000 rows it does not list back; n = 1; no entries at all."""
    t = T.matchlist_case(name, dtype)
    res = upload(ctx, t)
    assert_list_equal(ctx.matchlist_build(res, *flags), T.ref_matchlist(t, *flags, False))
    if flags == (False, False):
        assert_list_equal(ctx.matchlist_build(res, False, False, True), T.ref_matchlist(t, False, False, True))


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("sort_by_column", [False, True])
def test_matchlist_build_non_square(ctx, sort_by_column, dtype):
    t = T.matchlist_case("wide", dtype)
    assert_list_equal(ctx.matchlist_build(upload(ctx, t), False, False, sort_by_column), T.ref_matchlist(t, False, False, sort_by_column))


# ---------------------------------------------------------------------------------------------------- K7
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", T.BEST_MASTER_CASES)
def test_best_master(ctx, name, dtype):
    """About 5 000 x 3 000 with columns nobody names (-1), maxima shared by many rows (the lowest wins) and one unit in the
    last place above the runner-up; a maximum shared by 2 500 rows; a list without rows."""
    t = T.best_master_case(name, dtype)
    ml = ctx.matchlist_build(upload(ctx, t), False, False)
    want = T.ref_best_master(T.topn_to_list(t), t.n_cols)
    got = ml.best_master(t.n_cols)
    assert got.dtype == np.int32 and got.shape == (t.n_cols,)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------- K8
def check_group_reps(ctx, case: T.GraphCase):
    t = case.topn
    n = len(t.counts)
    src = T.topn_to_list(t)
    ml = ctx.matchlist_build(upload(ctx, t), False, False)
    assert_list_equal(ml, src)
    for centroid in (False, True):
        got = ml.group_reps(centroid)
        assert got.dtype == np.int32 and got.shape == (n,)
        want = T.ref_group_reps(src, n, centroid)
        assert np.array_equal(got, want), f"centroid={centroid}: {(got != want).sum()} of {n} representatives differ"


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("rest", T.BOUNDARY_RESTS)
def test_group_reps_row_length_sweep(ctx, rest, dtype):
    """Two-candidate components whose winner depends on the summation order (float64) or on the width of the accumulator
    (float32) at every branch of numpy's pairwise sum; exact ties (float32) go to the lower index; isolated nodes."""
    check_group_reps(ctx, T.centroid_sweep_case(rest, dtype))


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", T.GRAPH_CASES)
def test_group_reps_graphs(ctx, name, dtype):
    """One-directional edges only (weak connectivity); a path of 100 000 nodes renumbered at random and numbered along its
    length; stars whose centre has the highest index; thousands of two- and three-node components with tied centroids;
    isolated nodes."""
    check_group_reps(ctx, T.graph_case(name, dtype))


# ---------------------------------------------------------------------------------------------------- K9
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_rowwise_dot(ctx, dtype):
    """Common-column counts at every branch of the pairwise sum; no common column; empty rows; products that underflow to 0
    (dropped, they take no place in the order) and subnormal ones (kept); mixed magnitudes."""
    case = T.dot_case(dtype)
    got = ctx.rowwise_dot(ctx.csr_from_scipy(case.a), ctx.csr_from_scipy(case.b))
    want = T.ref_rowwise_dot(case.a, case.b)
    assert got.dtype == want.dtype == dtype and got.shape == want.shape
    assert np.array_equal(got, want), f"rows {np.flatnonzero(got != want)[:10]} differ"
    assert np.array_equal(np.signbit(got), np.signbit(want))


# ---------------------------------------------------------------------------------------------------- row costs
@pytest.mark.parametrize("collapse", ["0", None], ids=["SG_COLLAPSE=0", "default"])
@pytest.mark.parametrize("name", T.COST_CASES)
def test_row_costs(ctx, name, collapse):
    """(A != 0) @ df over the rows the index holds: B's rows with SG_COLLAPSE=0, one row per group of identical rows when
    the index says it grouped them -- which it does by default for 'repeats' (cosine-like, 9 000 rows >= 8 192, two thirds of
    them repeats >= 3 %: sg_collapse.hip) and for nothing else here.  The row permutation of the index changes no cost."""
    case = T.cost_case(name)
    ctx.set_option("SG_COLLAPSE", collapse)
    A, B = ctx.csr_from_scipy(case.a), ctx.csr_from_scipy(case.b)
    costs = {}
    for permute in (True, False):
        Bt = ctx.postings_build(B, permute=permute)
        n_index, n_caller, _ = ctx.postings_rows(Bt)
        assert n_caller == case.b.shape[0]
        index_rows = case.b
        assert (n_index < n_caller) == (name == "repeats" and collapse is None)
        if collapse == "0":
            assert n_index == n_caller
        elif n_index < n_caller:
            index_rows = T.distinct_rows(case.b)
            assert n_index == index_rows.shape[0]
        got = ctx.row_costs(A, Bt)
        assert got.dtype == np.int64 and got.shape == (case.a.shape[0],)
        assert np.array_equal(got, T.ref_row_costs(case.a, index_rows))
        costs[permute] = got
    assert np.array_equal(costs[True], costs[False])
