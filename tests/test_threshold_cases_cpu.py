"""The inputs of tests/_threshold_cases.py BITE: without a GPU, the port alone shows that on them `>=` for `>` changes the
answer at every threshold, that the arrival-order tie rule keeps other columns than the canonical one at every cut, and that
the port's scores are the arithmetic ones (the same product in integers).  tests/test_multiply_threshold_gpu.py then asks
every form of the multiply for the port's bits on the same inputs.  These are conditions on the inputs, not measurements:
seed and sizes are chosen so that they hold."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import _threshold_cases as T

dtypes = pytest.mark.parametrize("dtype", T.DTYPES, ids=lambda d: np.dtype(d).name)


@functools.lru_cache(maxsize=None)
def integer_product(case: str, scale: int) -> sp.csr_matrix:
    """A @ A.T with the entries scaled to integers (int64 matmul): scores times scale^2, exactly."""
    A = T.matrix(case, np.float64)
    ints = A.data * scale
    assert np.array_equal(ints, np.round(ints)) and ints.min() >= 1
    Ai = sp.csr_matrix((ints.astype(np.int64), A.indices, A.indptr), shape=A.shape)
    P = (Ai @ Ai.T).tocsr()
    P.sort_indices()
    return P


@functools.lru_cache(maxsize=None)
def no_cut(case: str, scale: int, floor: float) -> int:
    """A top_n that cuts no row of the product above ``floor``."""
    P = integer_product(case, scale)
    above = sp.csr_matrix((P.data > floor * scale * scale, P.indices, P.indptr), shape=P.shape)
    return int(above.sum(axis=1).max()) + 1


def sorted_rows(C: sp.csr_matrix) -> sp.csr_matrix:
    C = C.copy()
    C.sort_indices()
    return C


@pytest.mark.parametrize("case,scale,unit", [("ladder", 8, 64), ("long", 16, 256)])
@dtypes
def test_dyadic_scores_are_exact_and_the_port_computes_them(case, scale, unit, dtype):
    """Rows of squared norm exactly 1; every score of the full product a multiple of 1/64 (1/256), equal to the product in
    integer arithmetic -- for scipy's float product of all pairs and for the port's product above 0.25."""
    A = T.matrix(case, dtype)
    assert A.dtype == dtype and A.has_sorted_indices
    assert np.array_equal(np.asarray(A.multiply(A).sum(axis=1)).ravel(), np.ones(A.shape[0], dtype))
    P = integer_product(case, scale)
    F = (A @ A.T).tocsr()
    F.sort_indices()
    assert F.dtype == dtype and np.array_equal(F.indptr, P.indptr) and np.array_equal(F.indices, P.indices)
    assert np.array_equal(F.data * unit, P.data)                                  # (scale^2 = unit)
    top_n = no_cut(case, scale, 0.25)
    C = sorted_rows(T.port(case, dtype, top_n, 0.25))
    assert np.diff(C.indptr).max() < top_n
    keep = P.data > unit // 4
    rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))[keep]
    assert np.array_equal(np.diff(C.indptr), np.bincount(rows, minlength=P.shape[0]))
    assert np.array_equal(C.indices, P.indices[keep]) and np.array_equal(C.data * unit, P.data[keep])


@dtypes
def test_the_long_rows_meet_the_wide_launch(dtype):
    """Rows of 112 entries (the wide launch) and 8 of 256 (the exact kernel inside a pruned pass); in every row of 112 the 64
    light entries lie on its most frequent columns, each in at least 0.5 % of the rows, so that the suffix of frequent terms
    holds 51 of them at 0.5 and no more than 61 terms stay outside (sg_spgemm_pruned.hip: 64 at most)."""
    A = T.ladder_long(dtype)
    length = np.diff(A.indptr)
    assert set(np.unique(length)) == {112, 256} and (length == 256).sum() == T.LONG_XLONG_ROWS
    assert A.shape[0] > 2 * T.TILE_ROWS + 200
    df = np.bincount(A.indices, minlength=A.shape[1])
    for r in np.flatnonzero(length == 112):
        cols, vals = A.indices[A.indptr[r]:A.indptr[r + 1]], A.data[A.indptr[r]:A.indptr[r + 1]]
        light = vals == 0.0625
        assert light.sum() == T.LONG_LIGHT
        assert df[cols[light]].min() > df[cols[~light]].max() and df[cols[light]].min() >= 0.005 * A.shape[0] + 1
    assert 51 / 256 * 1.00001 < (0.45 / 1.00001) ** 2 * (1 - 1e-6) < 52 / 256


@pytest.mark.parametrize("case,scale,thresholds", [("ladder", 8, T.LADDER_THRESHOLDS), ("long", 16, T.LONG_THRESHOLDS)])
@dtypes
def test_thousands_of_pairs_sit_exactly_at_every_threshold(case, scale, thresholds, dtype):
    """kept(number below t) - kept(t) = the pairs exactly at t, at least 1 000 of them; and the reference restated with >=
    is another matrix than the port's at every t, cut or not."""
    P = integer_product(case, scale)
    A = T.matrix(case, dtype)
    top_n = no_cut(case, scale, 0.25)
    full = T.port(case, dtype, top_n, 0.25)
    for t in thresholds:
        at = int((P.data == t * scale * scale).sum())
        assert at >= 1000, (t, at)
        kept, kept_below = T.port(case, dtype, top_n, t), T.port(case, dtype, top_n, T.pred(t, dtype))
        assert np.diff(kept_below.indptr).max() < top_n
        assert kept_below.nnz - kept.nnz == at
        assert kept.nnz == int((P.data > t * scale * scale).sum())
        for cut in (top_n, 5):
            wrong = T.ref_topn_ge(A, cut, t, full)
            right = T.port(case, dtype, cut, t)
            assert wrong.nnz != right.nnz or not np.array_equal(wrong.indices, right.indices), (t, cut)
            # (the restated reference is the port's with the one thing put right: it is a reference, not a strawman)
            same = T.ref_topn_ge(A, cut, T.pred(t, dtype), full)
            below = T.port(case, dtype, cut, T.pred(t, dtype))
            assert np.array_equal(same.indptr, below.indptr) and np.array_equal(same.indices, below.indices)
            assert np.array_equal(same.data, below.data)


@pytest.mark.parametrize("t", T.FULL_CUT_THRESHOLDS)
@dtypes
def test_every_cut_falls_inside_blocks_of_equal_scores(t, dtype):
    """At every cut at least 100 rows are cut inside a block of equal scores; in at least 100 of them the arrival-order rule
    keeps other columns than the canonical one; and the tied members of some such row lie in more than one 4 096-row tile and
    in both 32 768-row super-tiles of the index."""
    thr = T.pred(t, dtype)
    top_n = no_cut("ladder", 8, 0.25)
    full = T.port("ladder", dtype, top_n, thr)
    count = np.diff(full.indptr)
    assert full.shape[0] > T.SUPER_TILE_ROWS + 444          # two super-tiles with the 444 duplicates grouped, too
    for cut in T.CUTS:
        cand = np.flatnonzero(count > cut)
        lo = full.indptr[cand]
        inside = cand[full.data[lo + cut - 1] == full.data[lo + cut]]
        assert len(inside) >= 100, (cut, len(inside))
        canonical = T.port("ladder", dtype, cut, thr, True, 0)
        arrival = T.port("ladder", dtype, cut, thr, True, 1)
        assert np.array_equal(canonical.indptr, arrival.indptr)
        other = [r for r in inside
                 if set(canonical.indices[canonical.indptr[r]:canonical.indptr[r + 1]]) != set(arrival.indices[arrival.indptr[r]:arrival.indptr[r + 1]])]
        assert len(other) >= 100, (cut, len(other))
        spread = False
        for r in inside:
            a, b = full.indptr[r], full.indptr[r + 1]
            tied = full.indices[a:b][full.data[a:b] == full.data[a + cut]]
            spread = len(np.unique(tied // T.TILE_ROWS)) > 1 and len(np.unique(tied // T.SUPER_TILE_ROWS)) == 2
            if spread:
                break
        assert spread, cut


@dtypes
def test_the_ladder_keeps_the_grouping_of_identical_rows_honest(dtype):
    A = T.ladder(dtype)
    distinct = len({(A.indices[a:b].tobytes(), A.data[a:b].tobytes()) for a, b in zip(A.indptr[:-1], A.indptr[1:])})
    assert 100 <= A.shape[0] - distinct and distinct > T.SUPER_TILE_ROWS


@dtypes
def test_name_thresholds_flip_the_chosen_pair(dtype):
    """The pair a threshold was made from is no match at thr = s and a match at the number below s; for float32 the doubles
    between the two decide as np.float32(thr) does -- the midpoint and its neighbours fall on both sides.  The low bands
    leave rows of 64 matches and more (the forms that hand full lists on), the others do not."""
    ths = T.name_thresholds(dtype)
    assert len(ths) == len(T.NAME_BANDS) * T.NAME_SCORES_PER_BAND * (5 if dtype == np.float32 else 2) + (dtype == np.float32)
    for nt in ths:
        C = T.port("names", dtype, 64, nt.thr, True, 0, slice(nt.row, nt.row + 1))
        assert (nt.col in C.indices) == nt.present, nt
        if nt.how == "at":
            assert not nt.present
        if nt.how == "below":
            assert nt.present
    if dtype == np.float32:
        for how in ("mid-", "mid+"):
            assert len({nt.present for nt in ths if nt.how == how}) == 1
        assert {nt.present for nt in ths if nt.how == "mid-"} != {nt.present for nt in ths if nt.how == "mid+"}
        assert all(float(np.float32(nt.thr)) != nt.thr for nt in ths if nt.how in ("mid", "mid-", "mid+", "plain"))
    low = max(nt.thr for nt in ths if nt.thr <= 0.45)
    for rows in (None, T.LEFT_SLICE["names"]):
        assert (np.diff(T.port("names", dtype, 65, low, True, 0, rows).indptr) >= 64).sum() >= 1
