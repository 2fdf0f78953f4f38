"""The inputs of tests/_offnorm_cases.py BITE: without a GPU, the port alone shows that their scores are the arithmetic ones
(the same product in integers), that hundreds of pairs sit exactly at every threshold, that `>=` for `>` changes the answer
at every one of them and arrival order for column order changes it at the cut, and that the index over them crosses a tile
boundary.  tests/test_multiply_offnorm_gpu.py then asks every form of the multiply for the port's bits on the same inputs.
These are conditions on the inputs, not measurements: seed and sizes are chosen so that they hold (three_quarter: 4 310 and
2 840 pairs at its thresholds; mixed: 1 376, 1 472 and 400; half_*: 720 and 2 833)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import _offnorm_cases as F
from tests import _threshold_cases as T

dtypes = pytest.mark.parametrize("dtype", F.DTYPES, ids=lambda d: np.dtype(d).name)
dyadic = pytest.mark.parametrize("case", F.DYADIC)

FLOOR = 0.125          # every threshold lies above it; the port's product above it is "every pair that matters"
# what turns the entries of (left, right) into integers: the two factors multiply to UNIT[case][0]
INT_SCALE = {"three_quarter": (32, 32), "mixed": (32, 32), "half_right": (8, 16), "half_left": (16, 8)}


@functools.lru_cache(maxsize=None)
def integer_product(case: str) -> sp.csr_matrix:
    """left @ right.T with the entries scaled to integers (int64 matmul): scores times UNIT, exactly."""
    left, right = F.operands(case, np.float64)
    out = []
    for m, scale in zip((left, right), INT_SCALE[case]):
        ints = m.data * scale
        assert np.array_equal(ints, np.round(ints)) and ints.min() >= 1
        out.append(sp.csr_matrix((ints.astype(np.int64), m.indices, m.indptr), shape=m.shape))
    P = (out[0] @ out[1].T).tocsr()
    P.sort_indices()
    return P


@functools.lru_cache(maxsize=None)
def no_cut(case: str) -> int:
    """A top_n that cuts no row of the product above FLOOR."""
    P = integer_product(case)
    above = sp.csr_matrix((P.data > FLOOR * F.UNIT[case][0], P.indices, P.indptr), shape=P.shape)
    return int(above.sum(axis=1).max()) + 1


def test_the_small_ladder_crosses_a_tile_boundary_grouped_or_not():
    """More than two tiles of rows (8 192): the index is built over the row permutation; more than 4 096 DISTINCT rows,
    so the index has two tiles with identical rows grouped (SG_COLLAPSE=1) and without; and some rows are identical, so
    that grouping does something.  Scaling keeps both: distinct rows stay distinct.  The gate tests' base: 5 812 rows = 22
    blocks of 256 and 180 (the gate's last wave is a partial one in a partial block)."""
    A = F.small(np.float32)
    assert A.shape[0] == F.SMALL_ROWS > 2 * F.TILE_ROWS and (np.diff(A.indptr) == 16).all()
    assert F.small(np.float32, F.GATE_FILLER_ROWS, F.GATE_CANDIDATES).shape[0] == F.GATE_ROWS == 22 * 256 + 180
    assert F.BAND_ROWS > 2 * F.TILE_ROWS
    for m in (A, F.mixed(np.float32), F.three_quarter(np.float32)):
        distinct = len({(m.indices[a:b].tobytes(), m.data[a:b].tobytes()) for a, b in zip(m.indptr[:-1], m.indptr[1:])})
        assert F.TILE_ROWS < distinct < m.shape[0] - 50
    B = F.band(np.float32)
    distinct = len({(B.indices[a:b].tobytes(), B.data[a:b].tobytes()) for a, b in zip(B.indptr[:-1], B.indptr[1:])})
    assert F.TILE_ROWS < distinct < B.shape[0]


@dtypes
def test_the_row_norms_are_what_the_cases_say(dtype):
    """Squared norms exactly 0.5625 (three_quarter), 1, 1/4 and 1/16 in one matrix (mixed), 1/4 (half); the band's largest
    lies in (1, 1.0001] as the gate computes it -- summed in double, rounded up to float32."""
    n2 = lambda m: np.asarray(m.multiply(m).sum(axis=1)).ravel()
    assert np.array_equal(n2(F.small(dtype)), np.ones(F.SMALL_ROWS, dtype))
    assert np.array_equal(n2(F.three_quarter(dtype)), np.full(F.SMALL_ROWS, 0.5625, dtype))
    assert np.array_equal(n2(F.half(dtype)), np.full(F.SMALL_ROWS, 0.25, dtype))
    e = F.mixed_exponents()
    assert np.array_equal(n2(F.mixed(dtype)), (0.25 ** e).astype(dtype)) and all((e == x).sum() > 1500 for x in (0, 1, 2))
    assert set(np.unique(F.three_quarter(dtype).data)) == {0.375, 0.1875, 0.09375}
    top = F.max_norm2_as_the_gate_sees_it(F.band(dtype))
    assert np.float32(1.00007) < top <= np.float32(1.0001), top
    assert F.band(dtype).dtype == dtype and F.band(dtype).has_sorted_indices


@dyadic
@dtypes
def test_dyadic_scores_are_exact_and_the_port_computes_them(case, dtype):
    """Every score is a multiple of 9/1024 (three_quarter), 1/1024 (mixed: 1/256 between rows whose exponents add up to 2
    at most) or 1/128 (half_*), equal to the product in integer arithmetic -- for scipy's float product of all pairs and
    for the port's product above FLOOR."""
    unit, step = F.UNIT[case]
    left, right = F.operands(case, dtype)
    assert left.dtype == dtype and right.dtype == dtype and left.has_sorted_indices and right.has_sorted_indices
    P = integer_product(case)
    assert (P.data % step == 0).all()
    G = (left @ right.T).tocsr()
    G.sort_indices()
    assert G.dtype == dtype and np.array_equal(G.indptr, P.indptr) and np.array_equal(G.indices, P.indices)
    assert np.array_equal(G.data * unit, P.data)
    if case == "mixed":
        e = F.mixed_exponents()
        rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
        low = e[rows] + e[P.indices] <= 2
        assert low.sum() > 1000 and (P.data[low] % 4 == 0).all()
    top_n = no_cut(case)
    C = F.port(case, dtype, top_n, FLOOR).copy()
    C.sort_indices()
    assert np.diff(C.indptr).max() < top_n
    keep = P.data > FLOOR * unit
    rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))[keep]
    assert np.array_equal(np.diff(C.indptr), np.bincount(rows, minlength=P.shape[0]))
    assert np.array_equal(C.indices, P.indices[keep]) and np.array_equal(C.data * unit, P.data[keep])


@dyadic
@dtypes
def test_hundreds_of_pairs_sit_exactly_at_every_threshold(case, dtype):
    """kept(number below t) - kept(t) = the pairs exactly at t, at least 300 of them; and the reference restated with >=
    is another matrix than the port's at every t, cut or not -- while with the threshold one ulp lower it is the port's."""
    unit, _ = F.UNIT[case]
    P = integer_product(case)
    left, _ = F.operands(case, dtype)
    top_n = no_cut(case)
    full = F.port(case, dtype, top_n, FLOOR)
    for t in F.THRESHOLDS[case]:
        assert t * unit == int(t * unit) and float(dtype(t)) == t
        at = int((P.data == t * unit).sum())
        assert at >= 300, (t, at)
        kept, kept_below = F.port(case, dtype, top_n, t), F.port(case, dtype, top_n, F.pred(t, dtype))
        assert kept_below.nnz - kept.nnz == at
        assert kept.nnz == int((P.data > t * unit).sum())
        for cut in (top_n, 5):
            wrong = T.ref_topn_ge(left, cut, t, full)
            right = F.port(case, dtype, cut, t)
            assert wrong.nnz != right.nnz or not np.array_equal(wrong.indices, right.indices), (t, cut)
            same = T.ref_topn_ge(left, cut, F.pred(t, dtype), full)
            below = F.port(case, dtype, cut, F.pred(t, dtype))
            assert np.array_equal(same.indptr, below.indptr) and np.array_equal(same.indices, below.indices)
            assert np.array_equal(same.data, below.data)


@dtypes
def test_the_cuts_fall_inside_blocks_of_equal_scores_on_mixed(dtype):
    """mixed at the number below 0.4375: at least 50 rows are cut by top_n = 5 and by top_n = 64 inside a block of equal
    scores, and in at least 50 of them the arrival-order rule keeps other columns than the canonical one."""
    thr = F.pred(0.4375, dtype)
    full = F.port("mixed", dtype, no_cut("mixed"), thr)
    count = np.diff(full.indptr)
    for cut in F.CUTS_EVERYWHERE:
        cand = np.flatnonzero(count > cut)
        lo = full.indptr[cand]
        inside = cand[full.data[lo + cut - 1] == full.data[lo + cut]]
        assert len(inside) >= 50, (cut, len(inside))
        canonical = F.port("mixed", dtype, cut, thr, True, 0)
        arrival = F.port("mixed", dtype, cut, thr, True, 1)
        assert np.array_equal(canonical.indptr, arrival.indptr)
        other = [r for r in inside
                 if set(canonical.indices[canonical.indptr[r]:canonical.indptr[r + 1]]) != set(arrival.indices[arrival.indptr[r]:arrival.indptr[r + 1]])]
        assert len(other) >= 50, (cut, len(other))


def _group_of_row(m: sp.csr_matrix) -> np.ndarray:
    seen = {}
    return np.array([seen.setdefault((m.indices[a:b].tobytes(), m.data[a:b].tobytes()), len(seen))
                     for a, b in zip(m.indptr[:-1], m.indptr[1:])])


@pytest.mark.parametrize("case", F.CASES)
@dtypes
def test_every_case_fills_lists_of_64_grouped_or_not(case, dtype):
    """At its lowest threshold every case has left rows with 64 matches and more -- in the self-product and in the slice
    that is the left matrix of its one-sided run -- and, what the form that hands FULL LISTS on needs with identical rows
    grouped (the pruned kernel's list then holds one entry per group of identical right-hand rows), 64 DISTINCT matches
    and more; no dyadic row has more than 128."""
    thr = min(F.thresholds(case, dtype))
    group = _group_of_row(F.operands(case, dtype)[1])
    for rows in ((None,) if case in ("half_right", "half_left") else (None, F.left_slice(case))):
        C = F.port(case, dtype, 200, thr, True, 0, rows)
        count = np.diff(C.indptr)
        distinct = np.array([len(set(group[C.indices[a:b]])) for a, b in zip(C.indptr[:-1], C.indptr[1:])])
        assert (count >= 64).sum() >= 2 and (distinct >= 64).sum() >= 2, (rows, (count >= 64).sum(), (distinct >= 64).sum())
        assert case == "band" or count.max() <= 128


@dtypes
def test_band_thresholds_flip_the_chosen_pair_and_one_keeps_the_diagonal(dtype):
    """The pair a threshold was made from is no match at thr = s and a match at the number below s; two scores per band
    at 0.5, 0.8 and 1.0 -- the last two are scores ABOVE 1, which only a matrix off the unit norm has.  A threshold of
    exactly 1.0 keeps the diagonal of every row that has entries: it scores the row's squared norm, ~1.00008.  The lowest
    threshold leaves rows of 64 matches and more (counted below)."""
    ths = F.band_thresholds(dtype)
    assert len(ths) == len(F.BAND_BANDS) * F.BAND_SCORES_PER_BAND * 2 + 1
    for bt in ths[:-1]:
        C = F.port("band", dtype, 64, bt.thr, True, 0, slice(bt.row, bt.row + 1))
        assert (bt.col in C.indices) == bt.present == (bt.how == "below"), bt
    assert sum(bt.thr > 1.0 for bt in ths) == 4 and ths[-1].thr == 1.0
    A = F.band(dtype)
    C = F.port("band", dtype, 64, 1.0)
    assert np.diff(C.indptr).max() < 64
    rows = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr))
    has_entries = np.diff(A.indptr) > 0
    assert has_entries.sum() >= A.shape[0] - 5
    assert np.array_equal(np.bincount(rows[rows == C.indices], minlength=A.shape[0]), has_entries.astype(np.int64))
    assert (C.data[rows == C.indices] > 1.00007).all()
