"""What a matrix derived from another carries over (csrc/sg_internal.h: the table at csr_inherit), seen from outside through
the binding: the norms K2 divided the rows by (``Csr.row_norms``), the words the vectoriser leaves (``Csr.vectoriser_words``),
the shape (``Csr.dims``) and the rows themselves (``Csr.to_scipy``).  One case per way of deriving a matrix -- transform, row
block, concatenation, selection, taking, reweighing -- and one for the groups of identical rows a left matrix caches, which a
row-block view must neither share nor free."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from oracle import port as P
from string_grouper_amd import _native as N
from string_grouper_amd.vectorizer import HipTfidfVectorizer, idf_from_df

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]

# a few dozen short strings: repeats (groups of identical rows), two shorter than an n-gram ("", "ab": rows without entries)
STRINGS = ["Acme Tools Ltd", "ACME TOOLS LIMITED", "acme tools ltd", "Borealis Shipping", "Borealis Shipping Co", "", "!!??",
           "Cedar & Pine Joinery", "Cedar and Pine Joinery", "Delta Freight", "Delta Freight", "Delta Freight GmbH",
           "Eastgate Bakery", "Eastgate Bakeries", "Fjord Salmon AS", "Fjord Salmon", "Gable Roofing", "Gable Roofing Inc",
           "Harbour Lights Cafe", "Harbor Lights Cafe", "Ironbridge Castings", "Iron Bridge Castings", "Juniper Press",
           "Juniper Press", "Kestrel Couriers", "Kestrel Courier Services", "Lantern Books", "Lantern Bookshop", "ab",
           "Marlow Dairy", "Marlow Dairies Ltd", "Northwind Traders", "Northwind Traders", "Oakfield Motors",
           "Oakfield Motor Company", "Pendle Ceramics", "Quarry Hill Stone", "Quarryhill Stone Ltd", "Riverside Vets",
           "Riverside Veterinary Practice"]
EMPTY_ROWS = [5, 28]
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.asarray(got.indptr, np.int64), np.asarray(want.indptr, np.int64)), f"{what}: row pointers differ"
    assert np.array_equal(got.indices, want.indices), f"{what}: columns differ"
    assert got.data.dtype == want.data.dtype and np.array_equal(_bits(got.data), _bits(want.data)), f"{what}: values differ"


def _fitted(ctx, dtype):
    vec = HipTfidfVectorizer(dtype=dtype, ctx=ctx)
    vec.fit_prepared([vec.prepare(pd.Series(STRINGS))])
    return vec


def _rows(vec, strings):
    return vec.transform_prepared(vec.prepare(pd.Series(list(strings))))


def _made(ctx, dtype):
    """(vectoriser, the transform of STRINGS on the device, the same on the host, its norms): made once a dtype, only read."""
    if dtype not in _cache:
        vec = _fitted(ctx, dtype)
        m = _rows(vec, STRINGS)
        _cache[dtype] = (vec, m, m.to_scipy(), m.row_norms())
    return _cache[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_transform_carries_norms_and_words_only_when_asked(ctx, dtype):
    vec, m, host, norms = _made(ctx, dtype)
    assert m.dims() == (len(STRINGS), host.shape[1], host.nnz, N.np_dtype_code(dtype))
    assert norms is not None and norms.dtype == np.float64 and len(norms) == len(STRINGS)
    empty = np.flatnonzero(np.diff(host.indptr) == 0)
    assert empty.tolist() == EMPTY_ROWS and (norms[empty] == 0.0).all() and (np.delete(norms, empty) > 0.0).all()
    assert m.vectoriser_words() is None
    try:
        ctx.set_option("SG_ROW_BLOCKS", "1")
        with_words = _rows(vec, STRINGS)
        words = with_words.vectoriser_words()
        assert words is not None and words[0] == 0 and words[2] == int(np.diff(host.indptr).max())
        assert np.array_equal(_bits(with_words.row_norms()), _bits(norms))
        with_words.free()
    finally:
        ctx.set_option("SG_ROW_BLOCKS", None)
    assert _rows(vec, STRINGS[:3]).vectoriser_words() is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_blocks_share_the_parents_norms_shifted(ctx, dtype):
    vec, m, host, norms = _made(ctx, dtype)
    view = m.row_block(3, 30)
    assert view.dims() == (27, host.shape[1], host[3:30].nnz, N.np_dtype_code(dtype))
    assert np.array_equal(_bits(view.row_norms()), _bits(norms[3:30]))
    _same(view.to_scipy(), host[3:30], "rows 3 .. 30")
    inner = view.row_block(2, 10)                            # a block of a block: rows 5 .. 13, rebased twice
    assert inner.dims() == (8, host.shape[1], host[5:13].nnz, N.np_dtype_code(dtype))
    assert np.array_equal(_bits(inner.row_norms()), _bits(norms[5:13]))
    _same(inner.to_scipy(), host[5:13], "rows 2 .. 10 of rows 3 .. 30")
    for k in (0, 7, len(STRINGS)):                           # no rows
        none = m.row_block(k, k)
        assert none.dims() == (0, host.shape[1], 0, N.np_dtype_code(dtype))
        assert none.row_norms() is not None and len(none.row_norms()) == 0
        assert none.to_scipy().shape == (0, host.shape[1]) and none.to_scipy().nnz == 0
        none.free()
    inner.free()
    view.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_concatenation_carries_norms_when_every_part_has_them(ctx, dtype):
    vec, m, host, norms = _made(ctx, dtype)
    other = _rows(vec, STRINGS[20:33])
    both = ctx.csr_concat([m, other])
    assert np.array_equal(_bits(both.row_norms()), _bits(np.concatenate([norms, norms[20:33]])))
    _same(both.to_scipy(), sp.vstack([host, host[20:33]], format="csr", dtype=dtype), "two vectoriser matrices")
    callers = ctx.csr_from_scipy(host[8:19])
    assert callers.row_norms() is None and callers.vectoriser_words() is None
    for what, parts, want in [("vectoriser + caller's", [m, callers], [host, host[8:19]]),
                              ("caller's + vectoriser", [callers, other], [host[8:19], host[20:33]])]:
        mixed = ctx.csr_concat(parts)
        assert mixed.row_norms() is None, what
        _same(mixed.to_scipy(), sp.vstack(want, format="csr", dtype=dtype), what)
        mixed.free()
    n = len(STRINGS)
    views = [m.row_block(0, 17), m.row_block(17, 17), m.row_block(17, n)]
    whole = ctx.csr_concat(views)                            # views of one parent, in order: the parent again
    assert np.array_equal(_bits(whole.row_norms()), _bits(norms))
    _same(whole.to_scipy(), host, "the views of one parent")
    for h in views + [whole, callers, both, other]:
        h.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_selection_gathers_the_norms_past_the_dropped_rows(ctx, dtype):
    vec, m, host, norms = _made(ctx, dtype)
    n = len(STRINGS)
    for what, drop in [("the first row", [0]), ("the last row", [n - 1]), ("two adjacent rows", [4, 5]), ("nothing", [])]:
        d = ctx.upload_sorted_ints(drop)
        sel = ctx.csr_select_rows(m, d)
        keep = np.delete(np.arange(n), drop)
        assert sel.dims() == (len(keep), host.shape[1], host[keep].nnz, N.np_dtype_code(dtype)), what
        assert np.array_equal(_bits(sel.row_norms()), _bits(np.delete(norms, drop))), what
        assert sel.vectoriser_words() is None, what
        _same(sel.to_scipy(), host[keep], what)
        sel.free()
        d.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_taken_rows_never_carry_norms(ctx, dtype):
    vec, m, host, norms = _made(ctx, dtype)
    n = len(STRINGS)
    for what, rows in [("repeats", [5, 5, 2, n - 1, 0, 2, 6]), ("reversed", list(range(n - 1, -1, -1))), ("one row", [9])]:
        d = ctx.upload_ints(rows)
        got = ctx.csr_take_rows(m, d)
        assert got.dims() == (len(rows), host.shape[1], host[rows].nnz, N.np_dtype_code(dtype)), what
        assert got.row_norms() is None, what
        _same(got.to_scipy(), host[rows], what)
        got.free()
        d.free()


@pytest.mark.parametrize("row_blocks", [False, True], ids=["default", "SG_ROW_BLOCKS=1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reweighed_rows_carry_norms_and_words(ctx, dtype, row_blocks):
    if row_blocks:
        ctx.set_option("SG_ROW_BLOCKS", "1")
    try:
        vec = _fitted(ctx, dtype)                            # (its own: a reweigh changes the vocabulary's idf)
        current = STRINGS[::2] + ["", "Delta Freight"]
        m = _rows(vec, current)
        df = m.column_counts().astype(np.int64)
        idf = idf_from_df(df, len(current), vec.dtype)
        out = ctx.vec_reweigh(vec._vocab, m, df, len(current), idf)
    finally:
        ctx.set_option("SG_ROW_BLOCKS", None)
    host = out.to_scipy()
    norms = out.row_norms()
    assert out.dims() == m.dims() and np.array_equal(host.indptr, m.to_scipy().indptr)
    assert norms is not None and len(norms) == len(current)
    length = np.diff(host.indptr)
    assert (norms[length == 0] == 0.0).all() and (norms[length > 0] > 0.0).all() and (length == 0).any()
    # every value is x / norm rounded once to dtype (relative error eps / 2), the norm itself a sum of k squares: the
    # row's length in exact arithmetic lies within (k + 4) eps of 1 for the longest row's k
    got = np.sqrt(np.asarray(host.astype(np.float64).multiply(host.astype(np.float64)).sum(axis=1)).ravel())
    tol = (int(length.max()) + 4) * float(np.finfo(dtype).eps)
    print(f"reweigh {np.dtype(dtype).name}: largest | ||row|| - 1 | = {np.abs(got[length > 0] - 1.0).max():.3e}, bound {tol:.3e}")
    assert (np.abs(got[length > 0] - 1.0) <= tol).all()
    words = out.vectoriser_words()
    assert words is not None and words[0] == 0 and words[2] == int(length.max())
    out.free()
    m.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_as_left_matrix_neither_shares_nor_frees_the_parents_groups(ctx, dtype):
    vec, right, right_host, _ = _made(ctx, dtype)
    left_strings = STRINGS[8:30] + STRINGS[8:30] + ["Delta Freight"] * 5          # repeats: groups of identical left rows
    left = _rows(vec, left_strings)
    left_host = left.to_scipy()
    post = ctx.postings_build(right)
    top_n, thr, r0, r1 = 4, 0.3, 6, 40
    start = N.live_handles()
    ctx.set_option("SG_COLLAPSE_LEFT", "1")                  # the left rows grouped from two rows on
    view = left.row_block(r0, r1)
    of_view = ctx.spgemm_topn(view, post, top_n, thr, True)
    of_parent = ctx.spgemm_topn(left, post, top_n, thr, True)
    again = ctx.spgemm_topn(view, post, top_n, thr, True)    # the view's own groups, kept from its first multiply
    _same(of_view.to_scipy(), P.sp_matmul_topn_port(left_host[r0:r1], right_host.T, top_n, thr, True), "the view")
    _same(of_parent.to_scipy(), P.sp_matmul_topn_port(left_host, right_host.T, top_n, thr, True), "the parent")
    _same(again.to_scipy(), of_view.to_scipy(), "the view again")
    for h in (again, of_view, of_parent):
        h.free()
    view.free()                                              # the view first ...
    assert N.live_handles() == start
    after = ctx.spgemm_topn(left, post, top_n, thr, True)    # ... and the parent's groups are still the parent's
    _same(after.to_scipy(), P.sp_matmul_topn_port(left_host, right_host.T, top_n, thr, True), "the parent after the view went")
    after.free()
    left.free()                                              # ... then the parent
    post.free()
    assert N.live_handles() == start - 2
