"""The three routes that score a NAMED pair give the same bits for the same pair: ``Context.pairs_dot``, the value
``Context.topn_union`` fills in for a column part 0 does not hold, and ``Context.topn_rescore``'s field score -- one walk
(csrc/sg_pairs_device.h), so one value, which is the numpy statement of tests/_pair_cases.py.  No tolerance.

Rows of 0, 1, 7, 8, 9 and 17 entries (the edges of the walk's chunk of eight) over 40 columns, strictly positive values and
column 0 in every row that has entries, so every score of two such rows is above zero; one dead row inside each matrix for the
two routes that take dead lists.  Every row has at most 64 candidates: the eight-lane kernels alone run."""
import numpy as np
import pytest

from string_grouper_amd import _native as N
from tests import _pair_cases as P

pytestmark = pytest.mark.gpu
N_COLS = 40
LENGTHS = (0, 1, 7, 8, 9, 17)


def _matrix(rng, dtype, dead_at):
    """The physical rows: LENGTHS in this order, and a row that is dead at ``dead_at``."""
    def row(n):
        cols = np.r_[0, 1 + np.sort(rng.choice(N_COLS - 1, n - 1, replace=False))] if n else np.zeros(0, np.int64)
        return cols, rng.uniform(0.1, 1.0, n).astype(dtype)

    rows = [row(n) for n in LENGTHS]
    rows.insert(dead_at, row(12))
    return P.csr_of(rows, dtype, N_COLS)


def _physical(live, dead):
    return live + np.searchsorted(dead - np.arange(len(dead)), live, side="right")     # CorpusState.physical_rows


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_pairs_dot_union_fill_and_rescore_agree_to_the_bit(ctx, dtype):
    rng = np.random.default_rng(7 + np.dtype(dtype).itemsize)
    dead_a, dead_b = np.array([3], np.int64), np.array([1], np.int64)
    A, B = _matrix(rng, dtype, 3), _matrix(rng, dtype, 1)
    R = C = len(LENGTHS)                                            # live rows of A, of B: the results' rows and columns
    ii, jj = [x.ravel() for x in np.meshgrid(np.arange(R), np.arange(C), indexing="ij")]
    left, right = _physical(ii, dead_a), _physical(jj, dead_b)
    assert 3 not in left and 1 not in right
    want = P.ref_pairs_dot(A, B, left, right).reshape(R, C)
    both = np.outer(np.array(LENGTHS) > 0, np.array(LENGTHS) > 0)
    assert np.all(want[both] > 0) and np.all(P.bits(want[~both]) == 0)          # no score is trivially zero, but an empty row's
    every = np.tile(np.arange(C, dtype=np.int32), (R, 1))
    with N.Scope() as s:
        a, b = s.own(ctx.csr_from_scipy(A)), s.own(ctx.csr_from_scipy(B))
        da, db = s.own(ctx.upload_sorted_ints(dead_a)), s.own(ctx.upload_sorted_ints(dead_b))

        by_pairs = ctx.pairs_dot(a, b, left, right).reshape(R, C)                # (a) physical rows, no dead lists
        assert P.same_bits(by_pairs, want)

        empty = s.own(ctx.topn_from_host(np.zeros((R, 1), np.int32), np.zeros((R, 1), dtype), np.zeros(R, np.int32), C))
        named = s.own(ctx.topn_from_host(every, np.full((R, C), 9, dtype), np.full(R, C, np.int32), C))
        cols, vals, counts = s.own(ctx.topn_union([empty, named], (a, b, da, db))).to_host()    # (b) every value is filled in
        assert np.array_equal(counts, np.full(R, C)) and np.array_equal(cols, every)
        assert P.same_bits(vals, want)

        cand = s.own(ctx.topn_from_host(every, np.ones((R, C), dtype), np.full(R, C, np.int32), C))
        res = s.own(ctx.topn_rescore(cand, 0.0, [(a, b, 1.0, da, db)], -1.0, C))            # (c) c = rn(+0 + rn(1 * s)) = s
        cols, vals, counts = res.to_host()
        assert np.array_equal(counts, np.full(R, C)) and np.array_equal(np.sort(cols, axis=1), every)
        by_column = np.empty_like(vals)
        np.put_along_axis(by_column, cols.astype(np.int64), vals, axis=1)
        assert P.same_bits(by_column, want)
