"""The refusals of the drivers behind the multiply -- K5 sg_topn_zip, K6 sg_matchlist_build, K8 sg_matchlist_group_reps, K9
sg_csr_rowwise_dot, sg_row_costs and the result operations of a resident corpus (sg_topn_concat_rows, _put_rows, _drop_columns,
_forget) and sg_selfjoin_merge -- and what the same context does right after one.  Every test (1) makes a call the host refuses by its arguments,
before anything is allocated or launched, and holds the exception's type and a word of its sentence, (2) makes a good call of
the same function on the same context, and (3) holds that call to a numpy expectation: the references of tests/_tail_cases.py
where there is one, otherwise written out here.  Results of 4 - 8 rows and stride 2 - 3, both value types; no tolerance.
The last test builds match lists of results without rows."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import _merge_cases as M
from tests import _tail_cases as T
from tests.test_selfjoin_merge_gpu import merge_and_compare
from tests.test_tail_gpu import assert_list_equal, assert_topn_equal, upload

pytestmark = pytest.mark.gpu

DTYPES = T.DTYPES


def other(dtype):
    return np.float64 if dtype == np.float32 else np.float32


def small_result(dtype, n_rows, n_cols, stride, seed) -> T.TopN:
    """Rows of 0 .. stride entries, distinct columns, scores k / 64 (exact in both value types), by score descending and
    column ascending as the multiply leaves them."""
    rng = np.random.default_rng(seed)
    cols = np.zeros((n_rows, stride), np.int32)
    vals = np.zeros((n_rows, stride), dtype)
    counts = np.zeros(n_rows, np.int32)
    for i in range(n_rows):
        k = min(int(rng.integers(0, stride + 1)), n_cols)
        c = rng.choice(n_cols, k, replace=False) if k else np.zeros(0, np.int64)
        v = (rng.integers(1, 64, k) / 64).astype(dtype)
        order = np.lexsort((c, -v))
        cols[i, :k], vals[i, :k], counts[i] = c[order], v[order], k
    t = T.TopN(cols, vals, counts, n_cols)
    T.check_preconditions(t)
    return t


def square_result(dtype) -> T.TopN:
    """4 x 4, stride 3: a pair stored from both sides (with the one score a pair has), pairs stored from one side, a stored
    diagonal that is not 1, an empty row, a full row."""
    def v(r, c):
        return (1 + 8 * min(r, c) + max(r, c)) / 64
    rows = [[(1, v(0, 1)), (2, v(0, 2))], [(0, v(0, 1)), (1, 0.75)], [], [(2, v(2, 3)), (0, v(0, 3)), (1, v(1, 3))]]
    row_ptr = np.cumsum([0] + [len(r) for r in rows])
    cols = np.array([c for r in rows for c, _ in r], np.int32)
    vals = np.array([s for r in rows for _, s in r], dtype)
    t = T.topn_from_rows(row_ptr, cols, vals, 4, stride=3)
    T.check_preconditions(t)
    return t


def small_csr(dtype, n_rows, n_cols, seed) -> sp.csr_matrix:
    """Rows of 2 .. 5 entries and an empty one, sorted, values k / 8 (every product and every sum of a row is exact in both
    value types)."""
    rng = np.random.default_rng(seed)
    ptr, cols = [0], []
    for i in range(n_rows):
        k = int(rng.integers(2, 6)) if i != 1 else 0
        cols.append(np.sort(rng.choice(n_cols, k, replace=False)))
        ptr.append(ptr[-1] + k)
    cols = np.concatenate(cols).astype(np.int32)
    m = sp.csr_matrix(((rng.integers(1, 8, len(cols)) / 8).astype(dtype), cols, np.array(ptr, np.int32)), shape=(n_rows, n_cols))
    assert m.has_canonical_format and m.dtype == dtype
    return m


# ---------------------------------------------------------------------------------------------------- K5
ZIP_REFUSALS = {
    "rows": (ValueError, "parts disagree"),
    "dtypes": (ValueError, "parts disagree"),
    "top_n=0": (ValueError, "bad argument"),
    "offset=2^31": (OverflowError, "exceeds int32"),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ZIP_REFUSALS)
def test_zip_refuses_and_then_zips(ctx, what, dtype):
    a, b = small_result(dtype, 5, 4, 2, 1), small_result(dtype, 5, 6, 3, 2)
    da, db = upload(ctx, a), upload(ctx, b)
    bad = {"rows": small_result(dtype, 6, 6, 3, 3), "dtypes": small_result(other(dtype), 5, 6, 3, 2)}.get(what)
    dbad = upload(ctx, bad) if bad is not None else db
    exc, word = ZIP_REFUSALS[what]
    with pytest.raises(exc, match=word):
        ctx.topn_zip([da, dbad], [2 ** 31 if what == "offset=2^31" else 0, 4], 0 if what == "top_n=0" else 4)
    case = T.ZipCase((a, b), np.array([0, 4], np.int64), 10)
    for top_n in (1, 4, 9):
        assert_topn_equal(ctx.topn_zip([da, db], case.offsets, top_n), T.ref_zip(case, top_n))


# ---------------------------------------------------------------------------------------------------- K6
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flags", [(True, False), (False, True)], ids=["fix_diagonal", "symmetrize"])
def test_matchlist_build_refuses_a_wide_result_and_then_builds(ctx, flags, dtype):
    wide, square = small_result(dtype, 4, 6, 3, 4), square_result(dtype)
    dwide, dsquare = upload(ctx, wide), upload(ctx, square)
    with pytest.raises(ValueError, match="square"):
        ctx.matchlist_build(dwide, *flags)
    for sort_by_column in (False, True):
        assert_list_equal(ctx.matchlist_build(dwide, False, False, sort_by_column),
                          T.ref_matchlist(wide, False, False, sort_by_column))
    assert_list_equal(ctx.matchlist_build(dsquare, *flags), T.ref_matchlist(square, *flags, False))
    assert_list_equal(ctx.matchlist_build(dsquare, True, True), T.ref_matchlist(square, True, True, False))


@pytest.mark.parametrize("dtype", DTYPES)
def test_matchlist_build_of_results_without_rows(ctx, dtype):
    """0 x 0 (square: every flag) and 0 x 5 (no flag): an empty list whose row pointer is [0]; then a list of 5 rows."""
    for n_cols, flag_sets in ((0, [(False, False, False), (True, True, False), (False, False, True)]),
                              (5, [(False, False, False), (False, False, True)])):
        empty = T.TopN(np.zeros((0, 2), np.int32), np.zeros((0, 2), dtype), np.zeros(0, np.int32), n_cols)
        dempty = upload(ctx, empty)
        assert dempty.dims() == (0, 2, 1 if dtype == np.float64 else 0, n_cols)
        for flags in flag_sets:
            ml = ctx.matchlist_build(dempty, *flags)
            assert ml.dims() == (0, 0, 1 if dtype == np.float64 else 0)
            row_ptr, cols, vals = ml.to_host()
            assert row_ptr.tolist() == [0] and len(cols) == 0 and len(vals) == 0 and vals.dtype == dtype
            assert ml.best_master(n_cols).tolist() == [-1] * n_cols
    five = small_result(dtype, 5, 5, 3, 5)
    dfive = upload(ctx, five)
    for flags in ((False, False, False), (False, False, True), (True, True, False)):
        assert_list_equal(ctx.matchlist_build(dfive, *flags), T.ref_matchlist(five, *flags))


# ---------------------------------------------------------------------------------------------------- K8
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_reps_refuses_a_wide_list_and_then_groups(ctx, dtype):
    wide, square = small_result(dtype, 4, 6, 3, 6), square_result(dtype)
    with pytest.raises(ValueError, match="square"):
        ctx.matchlist_build(upload(ctx, wide), False, False).group_reps(False)
    ml = ctx.matchlist_build(upload(ctx, square), True, True)
    want = T.ref_matchlist(square, True, True, False)
    assert_list_equal(ml, want)
    for centroid in (False, True):
        got = ml.group_reps(centroid)
        assert got.dtype == np.int32 and np.array_equal(got, T.ref_group_reps(want, 4, centroid))
    assert ml.group_reps(False).tolist() == [0, 0, 0, 0]      # rows 0, 1, 3 by their pairs, row 2 through (3, 2)


# ---------------------------------------------------------------------------------------------------- K9
DOT_REFUSALS = {"rows": "differ in shape", "columns": "differ in shape", "dtypes": "differ in value type"}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", DOT_REFUSALS)
def test_rowwise_dot_refuses_and_then_multiplies(ctx, what, dtype):
    a, b = small_csr(dtype, 5, 7, 7), small_csr(dtype, 5, 7, 8)
    bad = {"rows": small_csr(dtype, 4, 7, 9), "columns": small_csr(dtype, 5, 8, 9), "dtypes": b.astype(other(dtype))}[what]
    A, B = ctx.csr_from_scipy(a), ctx.csr_from_scipy(b)
    with pytest.raises(ValueError, match=DOT_REFUSALS[what]):
        ctx.rowwise_dot(A, ctx.csr_from_scipy(bad))
    got = ctx.rowwise_dot(A, B)
    want = T.ref_rowwise_dot(a, b)
    assert got.dtype == dtype and want.dtype == dtype and got.shape == (5,)
    assert np.array_equal(got, want) and np.any(want > 0)


# ---------------------------------------------------------------------------------------------------- row costs
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_costs_refuses_other_columns_and_then_counts(ctx, dtype):
    a, b = small_csr(dtype, 5, 8, 10), small_csr(dtype, 6, 8, 11)
    A, B = ctx.csr_from_scipy(a), ctx.csr_from_scipy(b)
    Bt = ctx.postings_build(B)
    assert ctx.postings_rows(Bt)[:2] == (6, 6)
    with pytest.raises(ValueError, match="different numbers of columns"):
        ctx.row_costs(ctx.csr_from_scipy(small_csr(dtype, 5, 7, 10)), Bt)
    got = ctx.row_costs(A, Bt)
    assert got.dtype == np.int64 and np.array_equal(got, T.ref_row_costs(a, b)) and got.sum() > 0


# ---------------------------------------------------------------------------------------------------- the corpus's result operations
def stacked(parts, stride) -> T.TopN:
    """scipy's vstack of result blocks: the parts' rows one after the other at the given stride."""
    cols = np.concatenate([np.pad(p.cols, ((0, 0), (0, stride - p.cols.shape[1]))) for p in parts])
    vals = np.concatenate([np.pad(p.vals, ((0, 0), (0, stride - p.vals.shape[1]))) for p in parts])
    return T.TopN(cols, vals, np.concatenate([p.counts for p in parts]), parts[0].n_cols)


def without_columns(t: T.TopN, rows, dead, top_n) -> T.TopN:
    """C[rows][:, keep] cut at top_n: the entries of the named rows whose column is not dead, in their order, renumbered by the
    dead columns below them."""
    stride = max(min(top_n, t.cols.shape[1]), 1)
    dead = np.asarray(dead, np.int64)
    out = T.TopN(np.zeros((len(rows), stride), np.int32), np.zeros((len(rows), stride), t.vals.dtype),
                 np.zeros(len(rows), np.int32), t.n_cols - len(dead))
    for k, r in enumerate(rows):
        c, v = t.cols[r, :t.counts[r]], t.vals[r, :t.counts[r]]
        live = ~np.isin(c, dead)
        c, v = (c[live] - np.searchsorted(dead, c[live]))[:stride], v[live][:stride]
        out.cols[k, :len(c)], out.vals[k, :len(c)], out.counts[k] = c, v, len(c)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ["columns", "dtypes"])
def test_concat_rows_refuses_and_then_stacks(ctx, what, dtype):
    a, b = small_result(dtype, 4, 6, 2, 12), small_result(dtype, 5, 6, 3, 13)
    bad = small_result(dtype, 5, 7, 3, 13) if what == "columns" else small_result(other(dtype), 5, 6, 3, 13)
    da, db = upload(ctx, a), upload(ctx, b)
    with pytest.raises(ValueError, match="parts disagree"):
        ctx.topn_concat_rows([da, upload(ctx, bad)])
    assert_topn_equal(ctx.topn_concat_rows([da, db]), stacked([a, b], 3))
    assert_topn_equal(ctx.topn_concat_rows([db, da, db]), stacked([b, a, b], 3))
    assert_topn_equal(ctx.topn_concat_rows([da]), a)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ["longer rows", "as many row numbers"])
def test_put_rows_refuses_and_then_puts(ctx, what, dtype):
    res, src = small_result(dtype, 6, 6, 2, 14), small_result(dtype, 2, 6, 2, 15)
    bad = small_result(dtype, 2, 6, 3, 15) if what == "longer rows" else src
    dres, which = upload(ctx, res), ctx.upload_ints([4, 1, 0])
    with pytest.raises(ValueError, match=what):
        ctx.topn_put_rows(dres, which.ptr, 2 if what == "longer rows" else 3, upload(ctx, bad))
    assert_topn_equal(dres, res)                              # (the refused call wrote nothing)
    ctx.topn_put_rows(dres, which.ptr, 2, upload(ctx, src))
    want = T.TopN(res.cols.copy(), res.vals.copy(), res.counts.copy(), 6)
    for k, row in enumerate((4, 1)):
        want.cols[row], want.vals[row], want.counts[row] = src.cols[k], src.vals[k], src.counts[k]
    assert_topn_equal(dres, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ["top_n", "more dead columns"])
def test_drop_columns_refuses_and_then_drops(ctx, what, dtype):
    res = small_result(dtype, 8, 5, 3, 16)
    dres = upload(ctx, res)
    all_and_one, dead = ctx.upload_sorted_ints(range(6)), ctx.upload_sorted_ints([1, 3])
    with pytest.raises(ValueError, match=what):
        ctx.topn_drop_columns(dres, dead if what == "top_n" else all_and_one, 0 if what == "top_n" else 2)
    assert np.isin(res.cols[:, 0][res.counts > 0], [1, 3]).any()       # (a best entry is dropped: the cut sees the next ones)
    for top_n in (1, 2, 3, 7):
        assert_topn_equal(ctx.topn_drop_columns(dres, dead, top_n), without_columns(res, range(8), [1, 3], top_n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_forget_refuses_a_wide_result_and_then_forgets(ctx, dtype):
    wide, square = small_result(dtype, 5, 6, 2, 17), small_result(dtype, 6, 6, 2, 18)
    dead = ctx.upload_sorted_ints([1, 4])
    with pytest.raises(ValueError, match="not square"):
        ctx.topn_forget(upload(ctx, wide), dead, 2)
    got, d_short = ctx.topn_forget(upload(ctx, square), dead, 2)
    n_short = len(d_short)
    kept = [0, 2, 3, 5]
    want = without_columns(square, kept, [1, 4], 2)
    assert_topn_equal(got, T.TopN(want.cols, want.vals, want.counts, 4))
    short = [k for k, r in enumerate(kept) if square.counts[r] >= 2 and want.counts[k] < 2]
    assert n_short == len(short) and ctx.download_ints(d_short, n_short).tolist() == short
    assert short, "no row was cut short: the case shows nothing of the list of short rows"
    d_short.free()


# ---------------------------------------------------------------------------------------------------- the self-join merge
@pytest.mark.parametrize("dtype", DTYPES)
def test_selfjoin_merge_refuses_a_stride_beyond_128_and_then_merges(ctx, dtype):
    """pairs_select_kernel holds a row in two register lists of 64: a result of 129 columns is refused on the host, whatever
    its rows hold (these hold a few entries and are named by two records each), and stays as it was; 128 columns are taken."""
    wide = small_result(dtype, 6, 300, 129, 19)
    dwide = upload(ctx, wide)
    records = M.make_records([250, 251] * 6, np.repeat(np.arange(6), 2), [0.5, 0.25] * 6, dtype)
    d_records = ctx.upload_ints(records.reshape(-1))
    with pytest.raises(ValueError, match="at most 128 columns"):
        ctx.selfjoin_merge(dwide, None, d_records.ptr, len(records), records.shape[1], 0, 6, 1)
    assert_topn_equal(dwide, wide)                            # (the refused call wrote nothing)
    back = dwide.to_host()
    assert np.array_equal(back[0], wide.cols) and back[1].tobytes() == wide.vals.tobytes()
    d_records.free()
    for name in ("boundaries-128", "batches-128"):
        merge_and_compare(ctx, M.case(name, dtype), M.want(name, dtype), None, f"{name} after the refusal")
