"""Constructed inputs, a plain reference and deliberately wrong references ("mutants") for sg_topn_transpose_select
(csrc/sg_corpus.hip): the reverse path's "top-n per corpus row" out of a pair list "new rows x corpus rows".  TEST
INFRASTRUCTURE ONLY: host arrays and numpy, no GPU and no library.  tests/test_transpose_select_cases_cpu.py proves that
the inputs tell every mutant from the reference; tests/test_transpose_select_gpu.py feeds the same inputs to the kernels and
expects the reference's bits.

The operation has two kernels.  A corpus row of at most 1 024 candidates is ranked by one wave (64 x 64 compares); a larger
one is queued for a workgroup, which finds the top_n-th best (score, pair row) by a radix select, 8 bits a pass, over the
bytes of the score (4 for float32, 8 for float64) and then the 4 bytes of the pair row, and ranks the selected set (at most
2 048 entries, in LDS).  512 workgroups loop over the queue.  The families below put a decision at every one of those bytes
and limits.

The reference is the order of the multiply (oracle/sdtn_port.c, the bounded insertion): by VALUE descending -- zeros of
either sign compare equal -- then by pair row ascending, cut at top_n.  What is written out is the input's bits, the sign of
a zero included, so results are compared as bit patterns.

A case is built from {corpus row m: (pair rows d, scores)}; every builder is seeded and cached: the arrays it returns are
shared and must not be written to.
"""
import functools
from typing import NamedTuple

import numpy as np

from tests import _tail_cases as T
from tests._tail_cases import TopN

DTYPES = T.DTYPES
WAVE_MAX = 1024      # csrc/sg_corpus.hip: TSEL_WAVE_MAX, the largest row a wave ranks by itself
MAX_TOP_N = 2048     # TSEL_MAX_TOPN, the LDS arrays of the workgroup kernel
BIG_GRID = 512       # TSEL_BIG_GRID, the workgroups that share the queue of larger rows
FILL_COLUMN = -7     # what the builder leaves behind a pair row's count (with a NaN score): never to be read


class Case(NamedTuple):
    name: str
    pairs: dict          # corpus row m -> (pair rows d: int64 [c], distinct; scores [c]), in no particular order
    n_in: int            # rows of the pair list = columns of the result
    n_out: int           # rows of the result (n_rows_out)
    top_n: tuple         # the values of top_n to run
    n_cols: int          # columns the pair list declares (<= n_out)


def _case(name, pairs, n_in, n_out, top_n, n_cols=None) -> Case:
    return Case(name, pairs, int(n_in), int(n_out), tuple(top_n), int(n_out if n_cols is None else n_cols))


def _uint(dtype):
    return np.uint32 if np.dtype(dtype) == np.float32 else np.uint64


def bits(v: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(v).view(_uint(v.dtype))


# ===================================================================================================== the builder
def pair_list(pairs, n_in, n_cols, dtype, seed=0) -> TopN:
    """The pair list as sg_topn_from_host takes it: row d names every corpus row m that lists d, in shuffled order; the
    stride is the longest pair row; every slot behind a row's count holds column -7 and a NaN score."""
    rng = np.random.default_rng(seed)
    for d, s in pairs.values():
        assert s.dtype == np.dtype(dtype) and len(d) == len(s)
    m = np.concatenate([np.full(len(d), m, np.int64) for m, (d, _) in pairs.items()] + [np.zeros(0, np.int64)])
    d = np.concatenate([np.asarray(d, np.int64) for d, _ in pairs.values()] + [np.zeros(0, np.int64)])
    s = np.concatenate([s for _, s in pairs.values()] + [np.zeros(0, dtype)])
    order = rng.permutation(len(d))
    order = order[np.argsort(d[order], kind="stable")]          # by pair row, shuffled inside one
    m, d, s = m[order], d[order], s[order]
    counts = np.bincount(d, minlength=n_in).astype(np.int32)
    assert len(counts) == n_in, "a pair row outside [0, n_in)"
    stride = max(1, int(counts.max()) if n_in else 1)
    slot = np.arange(len(d)) - np.repeat(np.cumsum(counts) - counts, counts)
    cols = np.full((n_in, stride), FILL_COLUMN, np.int32)
    vals = np.full((n_in, stride), np.nan, dtype)
    cols[d, slot] = m
    vals[d, slot] = s
    return TopN(cols, vals, counts, int(n_cols))


def build(case: Case, dtype) -> TopN:
    return pair_list(case.pairs, case.n_in, case.n_cols, dtype, seed=len(case.name) + 31 * case.n_in)


def check_pair_list(t: TopN):
    """check_preconditions of _tail_cases on the counted entries (no pair row names a column twice, every column inside the
    list's columns), and the filler everywhere else."""
    mask = np.arange(t.cols.shape[1])[None, :] < t.counts[:, None]
    assert (t.cols[~mask] == FILL_COLUMN).all() and np.isnan(t.vals[~mask]).all()
    assert not np.isnan(t.vals[mask]).any()
    T.check_preconditions(TopN(np.where(mask, t.cols, 0), np.where(mask, t.vals, 0), t.counts, t.n_cols))
    assert t.cols.shape[1] == max(1, int(t.counts.max()) if len(t.counts) else 1)


# ===================================================================================================== the reference
def value_order(d, s):
    """Score descending by value, then pair row ascending (np.lexsort sorts by its LAST key first; -0.0 == +0.0)."""
    return np.lexsort((d, -s))


def whole_cut(order, keep, c):
    return order[:keep]


def select(case: Case, dtype, top_n, order=value_order, cut=whole_cut) -> TopN:
    """Per corpus row: its candidates in `order`, cut at min(top_n, n_in) by `cut`.  n_out rows, n_in columns, stride
    min(top_n, max(n_in, 1))."""
    stride = min(top_n, max(case.n_in, 1))
    out = TopN(np.zeros((case.n_out, stride), np.int32), np.zeros((case.n_out, stride), dtype),
               np.zeros(case.n_out, np.int32), case.n_in)
    for m, (d, s) in case.pairs.items():
        kept = cut(order(d, s), min(len(d), top_n, case.n_in), len(d))
        out.cols[m, :len(kept)] = d[kept]
        out.vals[m, :len(kept)] = s[kept]
        out.counts[m] = len(kept)
    return out


def same(a: TopN, b: TopN) -> bool:
    return not len(rows_that_differ(a, b)) and a.n_cols == b.n_cols


def rows_that_differ(a: TopN, b: TopN) -> np.ndarray:
    """Rows whose count, columns or score BITS differ among the first counts[m] entries."""
    assert a.cols.shape == b.cols.shape and a.vals.dtype == b.vals.dtype
    mask = np.arange(a.cols.shape[1])[None, :] < np.minimum(a.counts, b.counts)[:, None]
    bad = (a.counts != b.counts) | ((a.cols != b.cols) & mask).any(axis=1) | ((bits(a.vals) != bits(b.vals)) & mask).any(axis=1)
    return np.flatnonzero(bad)


# ===================================================================================================== mutants
def bit_key(s):
    """The kernels' unsigned key with the order of the value: a negative's bits inverted, the sign bit set otherwise."""
    b = bits(s)
    top = b.dtype.type(1) << b.dtype.type(8 * b.itemsize - 1)
    return np.where(b & top, ~b, b | top)


def order_bit_key(d, s):                        # (a) +0.0 strictly before -0.0
    return np.lexsort((d, ~bit_key(s)))


def order_high_row_first(d, s):                 # (b) equal scores by pair row descending
    return np.lexsort((-d, -s))


def order_arrival(d, s):                        # (c) equal scores in the order they lie in the bucket
    return np.argsort(-s, kind="stable")


def order_rounded_to_float32(d, s):             # (d) float64 scores compared after rounding to float32
    with np.errstate(over="ignore"):
        return np.lexsort((d, -s.astype(np.float32)))


def order_without_lowest_byte(d, s):            # (e) the last pass over the score never decides
    k = bit_key(s)
    return np.lexsort((d, ~(k & ~k.dtype.type(0xff))))


def order_row_modulo_2_24(d, s):                # (f) the top byte of the pair row never decides
    return np.lexsort((d % (1 << 24), -s))


def order_raw_bits(d, s):                       # (g) score bits compared unsigned without the sign fix-up
    return np.lexsort((d, ~bits(s)))


def cut_big_rows_at_wave_max(order, keep, c):   # (h) a row for the workgroup kernel keeps what a wave could
    return order[:min(keep, WAVE_MAX) if c > WAVE_MAX else keep]


def cut_without_pivot(order, keep, c):          # (i) where a row is cut, the keep-th entry itself is left out
    return order[:keep - 1] if keep < c else order[:keep]


MUTANTS = {
    "a_bit_key_order": dict(order=order_bit_key),
    "b_high_row_first": dict(order=order_high_row_first),
    "c_arrival_order": dict(order=order_arrival),
    "d_rounded_to_float32": dict(order=order_rounded_to_float32),
    "e_without_lowest_byte": dict(order=order_without_lowest_byte),
    "f_row_modulo_2_24": dict(order=order_row_modulo_2_24),
    "g_raw_bits": dict(order=order_raw_bits),
    "h_big_rows_at_wave_max": dict(cut=cut_big_rows_at_wave_max),
    "i_without_pivot": dict(cut=cut_without_pivot),
}


# ===================================================================================================== families
BUCKET_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1026, 1087, 1088, 2047, 2048, 2049, 3000)


def _rng(family, dtype):
    return np.random.default_rng(4100 + 2 * sorted(FAMILIES).index(family) + (np.dtype(dtype) == np.float64))


def bucket_sizes(dtype):
    """One corpus row per candidate count around every limit: the wave's 64 lanes, the hand-over to the workgroup kernel
    (1 024 / 1 025), a second round of its 256 threads x 4 (1 087 / 1 088 = 1 024 + 63 / + 64), and its LDS arrays (2 047 /
    2 048 / 2 049): with the top_n values keep is c - 1, c and below it on either kernel, and 2 048 of more than 2 048."""
    rng = _rng("bucket_sizes", dtype)
    n_in = 3000
    pairs = {m: (rng.choice(n_in, c, replace=False).astype(np.int64), T._mixed_scores(rng, c, dtype))
             for m, c in enumerate(BUCKET_SIZES)}
    return (_case("bucket_sizes", pairs, n_in, len(BUCKET_SIZES), (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048)),)


SCORE_BYTE_HUB = 1500
SCORE_BYTE_WAVE_ROW = 300


def _scores_deciding_at(rng, b, dtype, n):
    """n distinct positive finite scores whose bit patterns agree in every byte above byte b (0: the sign's) and are
    random from byte b down.  The lowest byte: n neighbouring floats, one unit in the last place apart (beyond 256 of them
    the byte above counts on)."""
    u = _uint(dtype)
    nb = np.dtype(dtype).itemsize
    low = 8 * (nb - b)                                           # bits from byte b down
    if b == nb - 1:
        out = bits(np.array([0.75], dtype))[0] + np.arange(n, dtype=u)
    else:
        # distinct low parts; the sign's byte: sign clear, not inf / NaN, not a denormal, 0x01 .. 0x7e
        fixed = 0 if b == 0 else (int(bits(np.array([0.6180339887498949], dtype))[0]) >> low) << low
        if b == 0:
            low -= 8
        rest = rng.choice(1 << low, n, replace=False) if low <= 32 else rng.integers(0, 1 << low, n, dtype=np.uint64)
        out = np.uint64(fixed) | rng.permutation(rest.astype(np.uint64))
        if b == 0:
            out |= rng.integers(1, 0x7f, n, dtype=np.uint64) << np.uint64(low)
        assert len(np.unique(out)) == n
    return rng.permutation(out.astype(u)).view(dtype)


def deciding_score_byte(dtype):
    """Corpus row b, a hub of 1 500: the scores differ from byte b of their bits down, so the radix select's pass over
    byte b is the first whose histogram has more than one bin, and every pass below it still cuts.  One more row of 300
    neighbouring floats for the wave kernel."""
    rng = _rng("deciding_score_byte", dtype)
    nb = np.dtype(dtype).itemsize
    n_in = SCORE_BYTE_HUB
    pairs = {b: (rng.permutation(n_in).astype(np.int64), _scores_deciding_at(rng, b, dtype, n_in)) for b in range(nb)}
    pairs[nb] = (rng.choice(n_in, SCORE_BYTE_WAVE_ROW, replace=False).astype(np.int64),
                 _scores_deciding_at(rng, nb - 1, dtype, SCORE_BYTE_WAVE_ROW))
    return (_case("deciding_score_byte", pairs, n_in, nb + 1, (1, 255, 256, 257, 749, 1499, 1500)),)


# pair rows whose numbers differ first in byte 3 (the lowest), 2, 1 and 0 of the row: (low, high, how many).  [0, 256) cannot
# hold 400 distinct rows; it gives 200, so that with the blocks of 400 behind it the top_n values 200 / 600 / 1000 cut exactly
# at a range's end and 100 / 400 / 800 / 1200 / 1400 inside one.
ROW_BYTE_RANGES = ((0, 1 << 8, 200), (1 << 8, 1 << 16, 400), (1 << 16, 1 << 24, 400), (1 << 24, (1 << 24) + 2048, 600))
ROW_BYTE_HUB, ROW_BYTE_WAVE_ROW = 3, 6


def deciding_row_byte(dtype):
    """All scores equal, so the pair row alone orders a corpus row: the select runs through the score's bytes without a
    cut and decides in the bytes of ~row.  float32 only: 2^24 + 2 048 pair rows of stride 1."""
    assert np.dtype(dtype) == np.float32
    rng = _rng("deciding_row_byte", dtype)
    n_in = (1 << 24) + 2048

    def rows(scale):
        return np.concatenate([lo + rng.choice(hi - lo, n // scale, replace=False) for lo, hi, n in ROW_BYTE_RANGES]).astype(np.int64)
    hub, small = rows(1), rows(10)
    small = np.setdiff1d(small, hub)                             # (a pair row of stride 1 names one corpus row)
    pairs = {ROW_BYTE_HUB: (rng.permutation(hub), np.full(len(hub), 0.625, dtype)),
             ROW_BYTE_WAVE_ROW: (rng.permutation(small), np.full(len(small), 0.625, dtype))}
    return (_case("deciding_row_byte", pairs, n_in, 8, (100, 200, 400, 600, 800, 1000, 1200, 1400)),)


class SignsLayout(NamedTuple):
    n: int
    positive: int        # full-mantissa values above zero; +inf and the largest finite value come on top
    denormal: int        # of either sign
    zeros: int

    @property
    def before_zeros(self):
        """Entries that come before the block of zeros in value order."""
        return 2 + self.positive + self.denormal


SIGNS_HUB = SignsLayout(1500, 600, 20, 40)        # zeros at positions 622 .. 661
SIGNS_WAVE_ROW = SignsLayout(100, 30, 4, 12)      # zeros at positions 36 .. 47


def _signed_scores(rng, layout: SignsLayout, dtype):
    """Scores in value order: +inf, the largest finite value, positive full-mantissa values, positive denormals, the zeros,
    negative denormals, negative full-mantissa values."""
    info = np.finfo(dtype)
    n_denormal, n_positive = layout.denormal, layout.positive
    n_negative = layout.n - layout.before_zeros - layout.zeros - n_denormal
    denormal = info.smallest_subnormal * rng.choice(np.arange(1, 1000), 2 * n_denormal, replace=False).astype(dtype)
    return np.concatenate([np.array([np.inf, info.max], dtype), (0.001 + 1000 * rng.random(n_positive)).astype(dtype),
                           denormal[:n_denormal].astype(dtype), np.zeros(layout.zeros, dtype),
                           -denormal[n_denormal:].astype(dtype), -(0.001 + 1000 * rng.random(n_negative)).astype(dtype)])


def signs(dtype):
    """A hub (row 0) and a wave row (row 1) with scores of both signs.  Among the zeros the signs alternate along the pair
    rows, -0.0 at the lowest: by value then row they interleave, by bit pattern every +0.0 comes before every -0.0."""
    rng = _rng("signs", dtype)
    n_in = 1500
    pairs = {}
    for m, layout in enumerate((SIGNS_HUB, SIGNS_WAVE_ROW)):
        n = layout.n
        s = _signed_scores(rng, layout, dtype)
        d = rng.choice(n_in, n, replace=False).astype(np.int64)
        z = slice(layout.before_zeros, layout.before_zeros + layout.zeros)
        d[z] = np.sort(d[z])
        s[z] = np.where(np.arange(layout.zeros) % 2 == 0, -0.0, 0.0).astype(dtype)
        shuffle = rng.permutation(n)
        pairs[m] = (d[shuffle], s[shuffle])
    top_n = sorted({1, 1500} | {lay.before_zeros + k for lay in (SIGNS_HUB, SIGNS_WAVE_ROW)
                                for k in (-1, 0, 1, 2, lay.zeros // 2, lay.zeros - 1, lay.zeros, lay.zeros + 1)})
    return (_case("signs", pairs, n_in, 2, top_n),)


TIE_RUNS = ((60, 68), (1020, 1030), (2044, 2052))    # positions of equal scores, across 63 / 64 / 65, 1023 / 1024 / 1025, 2047 / 2048
TIE_BUCKETS = (1024, 1025, 2049, 5000)


def tie_blocks(dtype):
    """Distinct scores except for runs of equal ones across the cuts (which then fall to the pair row), in buckets on both
    sides of the hand-over and of the LDS arrays; row 4: 5 000 equal scores."""
    rng = _rng("tie_blocks", dtype)
    n_in = 5000
    pairs = {}
    for m, c in enumerate(TIE_BUCKETS):
        s = np.sort(np.unique((0.01 + 0.98 * rng.random(2 * c)).astype(dtype))[:c])[::-1].copy()
        assert len(s) == c
        for lo, hi in TIE_RUNS:
            if lo < c:
                s[lo:hi] = s[lo]
        shuffle = rng.permutation(c)
        pairs[m] = (rng.choice(n_in, c, replace=False).astype(np.int64), s[shuffle])
    pairs[len(TIE_BUCKETS)] = (rng.permutation(n_in).astype(np.int64), np.full(n_in, 0.5, dtype))
    return (_case("tie_blocks", pairs, n_in, len(TIE_BUCKETS) + 1, (64, 1024, 2047, 2048)),)


MANY_HUBS_ROWS, MANY_HUBS_BIG = 1100, 600


def many_hubs(dtype):
    """600 corpus rows of 1 025 .. 1 100 candidates among 1 100: more queued rows than workgroups, so 88 workgroups take a
    second row and re-initialise their select state.  With top_n = 1 030 a queued row of at most 1 030 candidates is taken
    whole and its neighbour in the queue is selected from."""
    rng = _rng("many_hubs", dtype)
    n = MANY_HUBS_ROWS
    big = np.zeros(n, bool)
    big[rng.choice(n, MANY_HUBS_BIG, replace=False)] = True
    c = np.where(big, rng.integers(WAVE_MAX + 1, n + 1, n), rng.integers(1000, WAVE_MAX + 1, n))
    assert (c > WAVE_MAX).sum() > BIG_GRID
    pairs = {m: (rng.choice(n, c[m], replace=False).astype(np.int64), T._mixed_scores(rng, c[m], dtype)) for m in range(n)}
    return (_case("many_hubs", pairs, n, n, (1, 1030, 2048)),)


def shapes(dtype):
    """Result shapes at their ends: more result rows than the pair list has columns; fewer pair rows than top_n (the stride
    is the pair rows); one pair row; a pair list without entries; no pair rows at all, with and without result rows."""
    rng = _rng("shapes", dtype)

    def some(n_in, rows):
        return {m: (rng.choice(n_in, c, replace=False).astype(np.int64), T._mixed_scores(rng, c, dtype)) for m, c in rows.items()}
    return (_case("extra_rows", some(1200, {0: 3, 2: 1100, 4: 70}), 1200, 9, (1, 70, 2048), n_cols=5),
            _case("five_pair_rows", some(5, {0: 5, 1: 1, 3: 4, 6: 5}), 5, 7, (1, 4, 5, 2048)),
            _case("one_pair_row", some(1, {0: 1, 2: 1}), 1, 4, (1, 2, 2048)),
            _case("no_entries", {}, 7, 4, (1, 2048)),
            _case("no_pair_rows_no_result_rows", {}, 0, 0, (1, 2048)),
            _case("no_pair_rows", {}, 0, 3, (1, 2048)))


FAMILIES = {"bucket_sizes": bucket_sizes, "deciding_score_byte": deciding_score_byte, "deciding_row_byte": deciding_row_byte,
            "signs": signs, "tie_blocks": tie_blocks, "many_hubs": many_hubs, "shapes": shapes}


@functools.lru_cache(maxsize=None)
def family(name, dtype) -> tuple:
    """The cases of a family (most have one)."""
    return FAMILIES[name](dtype)


def family_dtypes(name):
    return (np.float32,) if name == "deciding_row_byte" else DTYPES


@functools.lru_cache(maxsize=None)
def reference(name, dtype, index, top_n) -> TopN:
    """The reference's answer for case `index` of a family, computed once."""
    return select(family(name, dtype)[index], dtype, top_n)
