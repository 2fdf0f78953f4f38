"""Constructed inputs for the top-n multiply (sg_spgemm_topn, sg_selfjoin_range / sg_selfjoin_merge) whose scores sit EXACTLY
at the threshold and at the cut, and the table of the multiply's forms.  TEST INFRASTRUCTURE ONLY: host arrays, numpy / scipy,
the oracle's port; no GPU and no library.  tests/test_threshold_cases_cpu.py proves without a GPU that the inputs decide the
two rules every form promises -- strictly greater than the threshold; score descending, then column ascending --
tests/test_multiply_threshold_gpu.py runs every form on them and expects the port's bits.

ladder / ladder_long: every entry is a power of two, every row has squared norm exactly 1 (sg_csr_props: cosine-like, the
pruned kernels take it), so every product and every partial sum is exact in float32 and float64 whatever the order of the
additions: a form that differs from the port on them broke a RULE, not a rounding.  name_thresholds: the 20 000-name TF-IDF
matrix of the parity tests with thresholds taken from its own scores, for what dyadic numbers cannot show: inexact
products and the order of summation next to the threshold.

Every builder is seeded and cached: the arrays it returns are shared and must not be written to.
"""
import functools
from typing import Callable, NamedTuple, Optional

import numpy as np
import scipy.sparse as sp

DTYPES = (np.float32, np.float64)

# the left rows of the true one-sided products: a slice of the matrix uploaded as a matrix of its own
LEFT_SLICE = {"ladder": slice(3000, 9000), "long": slice(500, 1700), "names": slice(2000, 6000)}

TILE_ROWS = 4096          # index rows per tile of the stream form (sg_postings.hip)
SUPER_TILE_ROWS = 32768   # ... folded eight to an accumulator tile

# ---------------------------------------------------------------------------------------------------- the ladder
# 16 entries a row, squared norm 2/4 + 6/16 + 8/64 = 1.  Products are 1/4, 1/8, 1/16, 1/32 or 1/64: every score is k/64.
LADDER_VALUES = np.array([0.5] * 2 + [0.25] * 6 + [0.125] * 8)
LADDER_COLS = 65536
LADDER_ANCHORS = 24
LADDER_CANDIDATES = 200          # per anchor: cuts at 127 / 128 / 129 bite too
LADDER_FILLER_ROWS = 36000       # more than 32 768 index rows with the duplicates of the anchors grouped: two super-tiles
LADDER_SEED = 3
# thresholds that thousands of pairs hit exactly (counted in tests/test_threshold_cases_cpu.py)
LADDER_THRESHOLDS = (0.375, 0.4375, 0.5, 0.625, 0.75, 0.8125, 0.875)
CUTS = (1, 5, 10, 63, 64, 65, 100, 127, 128, 129)
CUTS_EVERYWHERE = (5, 64)               # at every ladder threshold
FULL_CUT_THRESHOLDS = (0.4375, 0.75)    # the whole of CUTS


def pred(t: float, dtype) -> float:
    """The largest number of ``dtype`` below ``t``, as a Python float: a score equal to ``t`` is a match above it by one ulp."""
    return float(np.nextafter(dtype(t), dtype(0)))


def _rows_to_csr(cols, vals, n_cols, dtype):
    n, k = cols.shape
    order = np.argsort(cols, axis=1, kind="stable")
    cols = np.take_along_axis(cols, order, axis=1)
    vals = np.take_along_axis(vals, order, axis=1)
    assert (np.diff(cols, axis=1) > 0).all(), "a row names a column twice"
    m = sp.csr_matrix((vals.ravel().astype(dtype), cols.ravel().astype(np.int32), np.arange(0, n * k + 1, k, dtype=np.int64)),
                      shape=(n, n_cols))
    m.has_sorted_indices = True
    return m


def _distinct_draws(rng, lo, hi, n, k):
    """n rows of k distinct integers of [lo, hi)"""
    out = rng.integers(lo, hi, size=(n, k))
    while True:
        s = np.sort(out, axis=1)
        bad = np.flatnonzero((np.diff(s, axis=1) == 0).any(axis=1))
        if not len(bad):
            return out
        out[bad] = rng.integers(lo, hi, size=(len(bad), k))


@functools.lru_cache(maxsize=None)
def _ladder_rows(seed=LADDER_SEED, anchors=LADDER_ANCHORS, candidates=LADDER_CANDIDATES, filler_rows=LADDER_FILLER_ROWS):
    """(columns, values) of the ladder's rows, 16 a row; the defaults are ``ladder()``'s, tests/_offnorm_cases.py asks for a
    smaller one."""
    rng = np.random.default_rng(seed)
    k = len(LADDER_VALUES)
    n_anchor_cols = anchors * k
    # anchors on disjoint column blocks, their values in a random order over the block
    anchor_cols = rng.permutation(n_anchor_cols).reshape(anchors, k)
    anchor_vals = np.stack([rng.permutation(LADDER_VALUES) for _ in range(anchors)])
    cols, vals = [anchor_cols], [anchor_vals]
    for a in range(anchors):
        for c in range(candidates):
            # 6 .. 16 of the anchor's columns; every third anchor is a tight family (13 .. 16, values in place for three of
            # four members) so that rows have more than 129 matches at 0.75 too
            tight = a % 3 == 0
            shared = int(rng.integers(13 if tight else 6, k + 1))
            keep = rng.permutation(k)[:shared]
            private = _distinct_draws(rng, n_anchor_cols, LADDER_COLS, 1, k - shared)[0]
            row_cols = np.concatenate([anchor_cols[a, keep], private])
            if c % 4 == 1 if tight else c % 2:            # the values permuted over the row
                row_vals = rng.permutation(LADDER_VALUES)
            else:                                         # the anchor's values in place; what is left of the ladder fills up
                rest = np.delete(anchor_vals[a], keep)    # (shared = 16: a duplicate of the anchor)
                row_vals = np.concatenate([anchor_vals[a, keep], rng.permutation(rest)])
            cols.append(row_cols[None, :])
            vals.append(row_vals[None, :])
    filler_cols = _distinct_draws(rng, n_anchor_cols, LADDER_COLS, filler_rows, k)
    filler_vals = np.stack([rng.permutation(LADDER_VALUES) for _ in range(filler_rows)])
    cols = np.concatenate(cols + [filler_cols])
    vals = np.concatenate(vals + [filler_vals])
    shuffle = rng.permutation(len(cols))                  # the members of a tie lie in different tiles
    return cols[shuffle], vals[shuffle]


@functools.lru_cache(maxsize=None)
def ladder(dtype) -> sp.csr_matrix:
    cols, vals = _ladder_rows()
    return _rows_to_csr(cols, vals, LADDER_COLS, dtype)


# ---------------------------------------------------------------------------------------------------- long rows
# 48 x 2^-3 ("heavy") + 64 x 2^-4 ("light"): 112 entries, squared norm 48/64 + 64/256 = 1 -- the pruned kernel's wide launch
# (65 .. 128 entries); 256 x 2^-4: squared norm 1, beyond the pruned kernel: the exact kernel scores such rows inside a
# pruned pass.  Products are 1/64, 1/128 or 1/256: every score is k/256.
#
# The wide launch takes a row only if at most 64 of its terms are left outside the suffix of its most frequent terms
# (sg_spgemm_pruned.hip: the suffix holds squared mass up to (threshold - delta)^2, 0.2025 at 0.5 with delta 0.05: 51 light
# entries, so 13 light + 48 heavy = 61 stay outside).  Every row therefore has its LIGHT entries on its most frequent columns:
# a family's members keep all 64 light columns of their anchor and 8 .. 48 of its heavy ones (the values in place; the other
# heavy entries on private columns), an unrelated row draws its light columns from a pool of 2048 (each in ~240 rows).  Members of a family
# score 1/4 + (heavy columns in common) / 64 with one another: 0.5, 0.625 and 0.75 at 16, 24 and 32.
LONG_HEAVY, LONG_LIGHT = 48, 64
LONG_COLS = 32768
LONG_ANCHORS = 6
LONG_CANDIDATES = 150
LONG_POOL_COLS = 2048
LONG_FILLER_ROWS = 7600         # more than 8 192 rows with the duplicates grouped: the index is built over the row permutation
LONG_XLONG_ROWS = 8
LONG_SEED = 5
LONG_THRESHOLDS = (0.5, 0.625, 0.75)
LONG_CUTS = (5, 64, 100)


@functools.lru_cache(maxsize=None)
def _ladder_long_rows(seed=LONG_SEED):
    rng = np.random.default_rng(seed)
    k = LONG_HEAVY + LONG_LIGHT
    n_anchor_cols = LONG_ANCHORS * k
    pool_lo, pool_hi = n_anchor_cols, n_anchor_cols + LONG_POOL_COLS
    anchor_cols = rng.permutation(n_anchor_cols).reshape(LONG_ANCHORS, k)       # [:, :48] heavy, [:, 48:] light
    values = np.array([0.125] * LONG_HEAVY + [0.0625] * LONG_LIGHT)
    rows = [(anchor_cols[a], values) for a in range(LONG_ANCHORS)]
    for a in range(LONG_ANCHORS):
        for c in range(LONG_CANDIDATES):
            shared = int(rng.integers(8, LONG_HEAVY + 1)) if c % 5 else LONG_HEAVY    # every fifth is a duplicate of the anchor
            keep = rng.permutation(LONG_HEAVY)[:shared]
            private = _distinct_draws(rng, pool_hi, LONG_COLS, 1, LONG_HEAVY - shared)[0]
            rows.append((np.concatenate([anchor_cols[a, keep], private, anchor_cols[a, LONG_HEAVY:]]), values))
    heavy = _distinct_draws(rng, pool_hi, LONG_COLS, LONG_FILLER_ROWS, LONG_HEAVY)
    light = pool_lo + np.argsort(rng.random((LONG_FILLER_ROWS, LONG_POOL_COLS)), axis=1)[:, :LONG_LIGHT]      # 64 distinct of the pool
    rows += [(np.concatenate([heavy[i], light[i]]), values) for i in range(LONG_FILLER_ROWS)]
    # rows of 256 entries over the columns of two anchors and 32 private ones: they match the members of both families
    # (1/4 + heavy columns in common / 128) and one another
    xvalues = np.full(256, 0.0625)
    for x in range(LONG_XLONG_ROWS):
        own = np.concatenate([anchor_cols[0], anchor_cols[1 + x % 2]])
        private = _distinct_draws(rng, pool_hi, LONG_COLS, 1, len(xvalues) - len(own))[0]
        rows.append((np.concatenate([own, private]), xvalues))
    shuffle = rng.permutation(len(rows))
    return [rows[i] for i in shuffle]


@functools.lru_cache(maxsize=None)
def ladder_long(dtype) -> sp.csr_matrix:
    rows = _ladder_long_rows()
    indptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(c) for c, _ in rows], out=indptr[1:])
    cols = np.concatenate([c for c, _ in rows])
    vals = np.concatenate([v for _, v in rows])
    m = sp.csr_matrix((vals.astype(dtype), cols.astype(np.int32), indptr), shape=(len(rows), LONG_COLS))
    m.sort_indices()
    assert m.nnz == len(cols) and all(np.all(np.diff(m.indices[a:b]) > 0) for a, b in zip(m.indptr[:-1], m.indptr[1:]))
    return m


# ---------------------------------------------------------------------------------------------------- names
NAME_ROWS = 20000
NAME_SEED = 1234
NAME_BANDS = (0.3, 0.42, 0.5, 0.62, 0.7, 0.8, 0.9)
NAME_SCORES_PER_BAND = 2
NAME_TOP_N = 10


class NameThreshold(NamedTuple):
    thr: float            # what the caller passes (a double)
    row: int              # the pair (row, col) whose score s the threshold was made from
    col: int
    present: bool         # is the pair a match at thr: s > (dtype)thr
    how: str              # "at", "below", "mid", "mid-", "mid+", "plain"


@functools.lru_cache(maxsize=None)
def name_matrix(dtype) -> sp.csr_matrix:
    from oracle import oracle as O
    from string_grouper_amd.synth import synth_names
    names = synth_names(NAME_ROWS, NAME_SEED)
    (m,), _, _ = O.tfidf_sklearn(names, [names], dtype=dtype)
    return m


@functools.lru_cache(maxsize=None)
def name_thresholds(dtype) -> tuple:
    """Thresholds made from scores of the port's own product of ``name_matrix(dtype)``: for a few scores s per band
    thr = s (the pair is no match) and thr = nextafter(s, 0) in the matrix's type (a match by one ulp).  float32 adds doubles
    that are no float32 values -- the port compares with np.float32(thr), the library plans and filters on the double and
    compares with (float)thr --: the midpoint of s and its float32 predecessor (ties to even), one double ulp either side
    of it, and plain 0.8."""
    from oracle import port as P
    A = name_matrix(dtype)
    C = P.sp_matmul_topn_port(A, A.T, 64, NAME_BANDS[0] - 0.02, True, 8)
    rows = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr))
    off = rows != C.indices                                   # (a diagonal is 1 up to rounding: not in any band)
    r, c, s = rows[off], C.indices[off], C.data[off]
    out = []
    for band in NAME_BANDS:
        near = np.argsort(np.abs(s.astype(np.float64) - band), kind="stable")
        seen = set()
        for i in near:
            if float(s[i]) in seen:                           # (a pair and its mirror image score the same)
                continue
            seen.add(float(s[i]))
            si = dtype(s[i])
            below = np.nextafter(si, dtype(0))
            out.append(NameThreshold(float(si), int(r[i]), int(c[i]), False, "at"))
            out.append(NameThreshold(float(below), int(r[i]), int(c[i]), True, "below"))
            if dtype == np.float32:
                mid = (float(si) + float(below)) / 2.0        # exact in a double
                for thr, how in ((mid, "mid"), (float(np.nextafter(mid, 0.0)), "mid-"), (float(np.nextafter(mid, 1.0)), "mid+")):
                    out.append(NameThreshold(thr, int(r[i]), int(c[i]), bool(si > np.float32(thr)), how))
            if len(seen) == NAME_SCORES_PER_BAND:
                break
    if dtype == np.float32:
        i = int(np.argmin(np.abs(s.astype(np.float64) - 0.8)))
        out.append(NameThreshold(0.8, int(r[i]), int(c[i]), bool(s[i] > np.float32(0.8)), "plain"))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------- references
_PORT_CACHE = {}


def port(case: str, dtype, top_n: int, thr: float, sort: bool = True, tie_rule: int = 0, rows: Optional[slice] = None):
    """The port's answer for ``matrix(case, dtype)`` (rows ``rows`` of it on the left) against the whole matrix, computed
    once per argument tuple and shared: do not write to it."""
    from oracle import port as P
    key = (case, np.dtype(dtype).name, int(top_n), float(thr), bool(sort), int(tie_rule), None if rows is None else (rows.start, rows.stop))
    if key not in _PORT_CACHE:
        A = matrix(case, dtype)
        left = A if rows is None else A[rows]
        _PORT_CACHE[key] = P.sp_matmul_topn_port(left, A.T, top_n, thr, sort, 8, tie_rule)
    return _PORT_CACHE[key]


def matrix(case: str, dtype) -> sp.csr_matrix:
    return {"ladder": ladder, "long": ladder_long, "names": name_matrix}[case](dtype)


def ref_topn_ge(A: sp.csr_matrix, top_n: int, thr: float, full: sp.csr_matrix) -> sp.csr_matrix:
    """The reference restated with ONE thing wrong: ``>=`` where the port has ``>``.  ``full``: every pair of the product
    with its score (rows in any order).  Score descending, then column ascending, cut at top_n."""
    keep = full.data >= A.dtype.type(thr)
    rows = np.repeat(np.arange(full.shape[0]), np.diff(full.indptr))[keep]
    cols, vals = full.indices[keep], full.data[keep]
    order = np.lexsort((cols, -vals.astype(np.float64), rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    start = np.searchsorted(rows, np.arange(full.shape[0]))
    rank = np.arange(len(rows)) - start[rows]
    sel = rank < top_n
    indptr = np.zeros(full.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(rows[sel], minlength=full.shape[0]), out=indptr[1:])
    return sp.csr_matrix((vals[sel], cols[sel].astype(np.int32), indptr), shape=full.shape)


# ---------------------------------------------------------------------------------------------------- the forms
class Form(NamedTuple):
    """One form of the multiply: the switches that force it and what ``ctx.stats()`` must say afterwards.
    build: options read by postings_build; run: options read by the multiply (both are set before the build and stay set);
    proof(stats, info) -> bool, info = dict(n = rows multiplied: the index's rows in a self-product -- the groups where
    identical rows are grouped --, n_left, long_rows = left rows beyond 128 entries, top_n, thr); self_join: the left matrix
    must be the one the index was built from; cuts: None = cuts up to 64, else the top_n values this form is about;
    cases: where the form can be reached; max_name_thr: the name thresholds it can be reached at."""
    name: str
    build: dict
    run: dict
    proof: Callable
    self_join: bool = False
    cuts: Optional[tuple] = None
    cases: tuple = ("ladder", "long", "names")
    max_name_thr: float = 2.0


# The pruned kernels are reachable at every threshold used here with SG_PRUNE_MIN_THRESHOLD=0.25 (the rule is
# string_grouper_amd/csrc/sg_plan.h, held at its bars by tests/test_multiply_plan_cpu.py: the bar is a tuning, 0.40 / 0.45 by
# default -- sg_plan_min_threshold); the stream form below 0.65 needs SG_ALT_FORM=0, the tile-by-tile form from 0.65 up
# SG_ALT_FORM_BELOW=2 (sg_plan_wants_tile_form).  SG_PRUNE_PILOT=0: the pruned-or-exact pilot is a tuning of its own and would hand a dense case to the
# exact kernel.
_PRUNED = {"SG_PRUNE_MIN_THRESHOLD": "0.25", "SG_PRUNE_PILOT": "0"}
_STREAM = dict(_PRUNED, SG_ALT_FORM="0")
_TILE = dict(_PRUNED, SG_ALT_FORM_BELOW="2")

def _pruned(st, i, symmetric):
    """The pruned kernel took the product, one-sided or in the self-join form; the rows beyond its reach (more than 128
    entries) went to the exact kernel."""
    return st["prune_rows"] > 0 and st["prune_symmetric"] == symmetric and st["exact_rows"] >= i["long_rows"]


FORMS = (
    Form("exact-one-sided", {"SG_PRUNE": "0"}, {"SG_PRUNE": "0"},
         lambda st, i: st["prune_rows"] == 0 and st["prune_symmetric"] == 0),
    Form("exact-selfjoin", {}, {"SG_SYM": "1", "SG_PRUNE_MIN_THRESHOLD": "1.5"},
         lambda st, i: st["prune_rows"] == 0 and st["prune_symmetric"] == 1 and st["exact_rows"] == i["n"], self_join=True),
    # (rows beyond 60 entries have no 8-bit copy and pass the second filter unseen -- sg_postings.hip --: on the long rows
    #  it cannot reject anything, the form is the next line's there)
    Form("stream-one-sided-q8", {"SG_Q8": "1"}, dict(_STREAM, SG_SYM="0", SG_Q8_MIN_THRESHOLD="0"),
         lambda st, i: _pruned(st, i, 0) and st["prune_scored"] < st["prune_survivors"], cases=("ladder", "names")),
    Form("stream-one-sided-noq8", {"SG_Q8": "0"}, dict(_STREAM, SG_SYM="0", SG_Q8="0"),
         lambda st, i: _pruned(st, i, 0) and st["prune_scored"] == st["prune_survivors"]),
    Form("stream-selfjoin", {"SG_Q8": "1"}, dict(_STREAM, SG_SYM="1", SG_Q8_MIN_THRESHOLD="0"),
         lambda st, i: _pruned(st, i, 1), self_join=True),
    Form("tile-one-sided", {}, dict(_TILE, SG_SYM="0"), lambda st, i: _pruned(st, i, 0)),
    Form("tile-selfjoin", {}, dict(_TILE, SG_SYM="1"), lambda st, i: _pruned(st, i, 1), self_join=True),
    Form("round2-loop-one-sided", {"SG_K4_STREAM": "0"}, dict(_PRUNED, SG_K4_STREAM="0", SG_SYM="0", SG_ALT_FORM="0"),
         lambda st, i: _pruned(st, i, 0)),
    Form("round2-loop-selfjoin", {"SG_K4_STREAM": "0"}, dict(_PRUNED, SG_K4_STREAM="0", SG_SYM="1", SG_ALT_FORM="0"),
         lambda st, i: _pruned(st, i, 1), self_join=True),
    # top_n of 65 .. 128 in the self-join forms: the second pass selects with two register lists, nobody goes to the exact
    # kernel for a full list -- only the rows beyond 128 entries
    Form("two-lists-stream-selfjoin", {}, dict(_STREAM, SG_SYM="1"),
         lambda st, i: _pruned(st, i, 1) and st["exact_rows"] == i["long_rows"], self_join=True, cuts=(65, 100, 127, 128)),
    Form("two-lists-tile-selfjoin", {}, dict(_TILE, SG_SYM="1"),
         lambda st, i: _pruned(st, i, 1) and st["exact_rows"] == i["long_rows"], self_join=True, cuts=(65, 100, 127, 128)),
    # ... one-sided: the pruned kernel keeps a row's best 64, rows whose list comes out full are redone by the exact kernel
    # (among the names only low thresholds leave rows with 64 matches and more -- tests/test_threshold_cases_cpu.py counts them)
    Form("full-lists-handed-on", {}, dict(_STREAM, SG_SYM="0"),
         lambda st, i: _pruned(st, i, 0) and st["exact_rows"] > i["long_rows"], cuts=(65, 100, 127, 128), max_name_thr=0.45),
    Form("more-than-128", {}, dict(_PRUNED), lambda st, i: st["prune_rows"] == 0, cuts=(129, 200)),
    # the stream + self-join form with rows of two rounds and more set aside and worked off in parts by a second launch
    Form("rows-in-parts", {}, dict(_STREAM, SG_SYM="1", SG_HEAVY_ROUNDS="2"), lambda st, i: _pruned(st, i, 1), self_join=True),
)
FORM_NAMES = tuple(f.name for f in FORMS)


def form(name: str) -> Form:
    return FORMS[FORM_NAMES.index(name)]
