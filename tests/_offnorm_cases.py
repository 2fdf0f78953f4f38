"""Constructed inputs for the top-n multiply whose ROW NORMS ARE NOT 1.  TEST INFRASTRUCTURE ONLY: host arrays, numpy / scipy,
the oracle's port; no GPU and no library.  Everything tests/_threshold_cases.py multiplies has rows of norm 1, where the
scale norm_up -- K3 (the index build) divides every quantised bound by it, K4p (the pruned multiply) multiplies by it -- is
1.000001 and a mismatch between the two cannot show.  tests/test_offnorm_cases_cpu.py proves without a GPU that these
inputs decide the multiply's two rules, tests/test_multiply_offnorm_gpu.py runs every form on them and expects the port's
bits, tests/test_cosine_gate_gpu.py takes the small ladder to the edges of the gate (sg_csr_props).

  small          the ladder of _threshold_cases.py at a fifth of its size: 12 anchors x 160 candidates + 6 381 filler
                 rows = 8 313 rows of 16 power-of-two entries, squared norm exactly 1 (why these counts: below); more
                 than 4 096 distinct rows, so the index crosses a tile boundary with identical rows grouped, too.
                 (With 150 candidates and 4 000 filler rows, 5 812 = 22 * 256 + 180 rows, it is the gate tests' base.)
  three_quarter  small x 0.75: entries 3/8, 3/16, 3/32, squared norm 0.5625, norm_up ~ 0.75; every score is 9k/1024
  mixed          row i of small x 2^-e_i, e_i of {0, 1, 2}: norms 1, 1/2 and 1/4 in ONE matrix (norm_up ~ 1, but most
                 rows far below it); every score is k/1024 (k/256 between rows whose exponents add up to 2 at most)
  half_right     rows 1000:3000 of small against small x 0.5: norm_up ~ 0.5 while the left values are unscaled
  half_left      rows 1000:3000 of small x 0.5 against small: the scale on the left only; scores k/128 in both
  band           8 400 names' TF-IDF rows x 1.00004: squared norms up to ~1.00008, inside the gate's band (1, 1.0001] --
                 the pruned kernels run with norm_up > 1 -- inexact products, thresholds from the port's own scores

Every product of the dyadic cases is exact in float32 and float64 whatever the order of the additions: a form that
differs from the port on them broke a RULE or a BOUND, not a rounding.  Every builder is seeded and cached: the arrays it
returns are shared and must not be written to."""
import functools
from typing import NamedTuple, Optional

import numpy as np
import scipy.sparse as sp

from tests import _threshold_cases as T
from tests._threshold_cases import DTYPES, TILE_ROWS, pred  # noqa: F401  (re-exported for the tests of these cases)

# Larger than a seventh of the ladder (12 x 150 + 4 000 = 5 812 rows), for two forms' sake:
#  * 6 381 filler rows: the index build makes its copy of the rows in position order (build_permuted, which also writes the
#    packed rows and the 8-bit records the scale goes into) only for MORE than two tiles of rows, 8 192 for the pruned
#    kernels' index -- with fewer no pruned form runs "over the library's row permutation";
#  * 160 candidates per anchor: with 150 no row has 64 DISTINCT matches at 0.875 (0.4375 in half_*) -- 58 at most, the rest
#    are identical rows -- so with identical rows grouped no list of the pruned kernel comes out full there and the form that
#    hands full lists on cannot be reached; 151 .. 159 reach 64 by a row or two or not at all, 160 has 17 such rows in the
#    slice (70 at most).  Filler rows do not help: they match nothing.
SMALL_ANCHORS, SMALL_CANDIDATES, SMALL_FILLER_ROWS = 12, 160, 6381
SMALL_ROWS = SMALL_ANCHORS * (1 + SMALL_CANDIDATES) + SMALL_FILLER_ROWS      # 8 313
GATE_CANDIDATES, GATE_FILLER_ROWS = 150, 4000      # tests/test_cosine_gate_gpu.py: 5 812 rows = 22 * 256 + 180
GATE_ROWS = SMALL_ANCHORS * (1 + GATE_CANDIDATES) + GATE_FILLER_ROWS
LEFT_SLICE = slice(1000, 3000)         # the left rows of the true one-sided products
BAND_LEFT_SLICE = slice(500, 3500)     # ... of the band: rows 927 and 3008 have 64 distinct matches and more at its lowest threshold
MIXED_SEED = 11
BAND_ROWS, BAND_SEED, BAND_FACTOR = 8400, 4321, 1.00004      # (more than 8 192 rows for the same reason)
BAND_BANDS = (0.5, 0.8, 1.0)
BAND_SCORES_PER_BAND = 2
BAND_TOP_N = 10
CUTS_EVERYWHERE = (5, 64)

DYADIC = ("three_quarter", "mixed", "half_right", "half_left")
SELF_CASES = ("three_quarter", "mixed", "band")
CASES = DYADIC + ("band",)
# thresholds that hundreds of pairs hit exactly (counted in tests/test_offnorm_cases_cpu.py); each is passed as t and as
# the number below t
THRESHOLDS = {"three_quarter": (0.421875, 0.4921875), "mixed": (0.4375, 0.5, 0.75), "half_right": (0.4375, 0.5),
              "half_left": (0.4375, 0.5)}
# score * UNIT is an integer, a multiple of STEP
UNIT = {"three_quarter": (1024, 9), "mixed": (1024, 1), "half_right": (128, 1), "half_left": (128, 1)}


@functools.lru_cache(maxsize=None)
def small(dtype, filler_rows=SMALL_FILLER_ROWS, candidates=SMALL_CANDIDATES) -> sp.csr_matrix:
    cols, vals = T._ladder_rows(T.LADDER_SEED, SMALL_ANCHORS, candidates, filler_rows)
    assert len(cols) == SMALL_ANCHORS * (1 + candidates) + filler_rows
    return T._rows_to_csr(cols, vals, T.LADDER_COLS, dtype)


def scaled(m: sp.csr_matrix, factor) -> sp.csr_matrix:
    """``m`` with every value times ``factor`` (a scalar, or one factor per row) in m's type; the structure is shared."""
    f = np.asarray(factor, m.dtype)
    data = m.data * (np.repeat(f, np.diff(m.indptr)) if f.ndim else f)
    assert data.dtype == m.dtype
    out = sp.csr_matrix((data, m.indices, m.indptr), shape=m.shape)
    out.has_sorted_indices = True
    return out


@functools.lru_cache(maxsize=None)
def mixed_exponents() -> np.ndarray:
    """e_i of {0, 1, 2}, drawn once and shared between the dtypes"""
    return np.random.default_rng(MIXED_SEED).integers(0, 3, SMALL_ROWS)


@functools.lru_cache(maxsize=None)
def three_quarter(dtype) -> sp.csr_matrix:
    return scaled(small(dtype), 0.75)


@functools.lru_cache(maxsize=None)
def mixed(dtype) -> sp.csr_matrix:
    return scaled(small(dtype), 0.5 ** mixed_exponents())


@functools.lru_cache(maxsize=None)
def half(dtype) -> sp.csr_matrix:
    return scaled(small(dtype), 0.5)


@functools.lru_cache(maxsize=None)
def band(dtype) -> sp.csr_matrix:
    from oracle import oracle as O
    from string_grouper_amd.synth import synth_names
    names = synth_names(BAND_ROWS, BAND_SEED)
    (m,), _, _ = O.tfidf_sklearn(names, [names], dtype=dtype)
    m = m.tocsr()
    m.sort_indices()
    return scaled(m, dtype(BAND_FACTOR))


def left_slice(case: str) -> slice:
    """the rows that make the left matrix of a self-product case's true one-sided run"""
    return BAND_LEFT_SLICE if case == "band" else LEFT_SLICE


def max_norm2_as_the_gate_sees_it(m: sp.csr_matrix) -> np.float32:
    """The largest squared row norm the way csr_props_kernel computes it: summed in double, rounded UP to float32."""
    s = np.asarray(m.astype(np.float64).multiply(m.astype(np.float64)).sum(axis=1)).ravel().max()
    f = np.float32(s)
    return f if float(f) >= s else np.nextafter(f, np.float32(2))


def operands(case: str, dtype, rows: Optional[slice] = None):
    """(left, right) of a case.  The self-product cases return the matrix twice (or its rows ``rows`` on the left); the
    half_* cases are one-sided as they are and take no ``rows``."""
    if case in ("half_right", "half_left"):
        assert rows is None
        a, b = small(dtype)[LEFT_SLICE], half(dtype)
        return (a, b) if case == "half_right" else (half(dtype)[LEFT_SLICE], small(dtype))
    A = {"three_quarter": three_quarter, "mixed": mixed, "band": band, "small": small}[case](dtype)
    return (A if rows is None else A[rows]), A


_PORT_CACHE = {}


def port(case: str, dtype, top_n: int, thr: float, sort: bool = True, tie_rule: int = 0, rows: Optional[slice] = None):
    """The port's answer for ``operands(case, dtype, rows)``, computed once per argument tuple and shared: do not write
    to it."""
    from oracle import port as P
    key = (case, np.dtype(dtype).name, int(top_n), float(thr), bool(sort), int(tie_rule), None if rows is None else (rows.start, rows.stop))
    if key not in _PORT_CACHE:
        left, right = operands(case, dtype, rows)
        _PORT_CACHE[key] = P.sp_matmul_topn_port(left, right.T, top_n, thr, sort, 8, tie_rule)
    return _PORT_CACHE[key]


class BandThreshold(NamedTuple):
    thr: float            # what the caller passes
    row: int              # the pair (row, col) whose score s the threshold was made from (-1: none, a plain number)
    col: int
    present: bool         # is the pair a match at thr
    how: str              # "at", "below", "plain"


@functools.lru_cache(maxsize=None)
def band_thresholds(dtype) -> tuple:
    """Thresholds made from scores of the port's own product of ``band(dtype)``, as _threshold_cases.name_thresholds makes
    them: for two scores s per band thr = s (the pair is no match) and thr = the number below s (a match by one ulp); and
    plain 1.0, which must keep every diagonal (a row's score with itself is its squared norm, ~1.00008)."""
    C = port("band", dtype, 64, BAND_BANDS[0] - 0.02)
    rows = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr))
    off = rows != C.indices
    r, c, s = rows[off], C.indices[off], C.data[off]
    out = []
    for b in BAND_BANDS:
        near = np.argsort(np.abs(s.astype(np.float64) - b), kind="stable")
        seen = set()
        for i in near:
            if float(s[i]) in seen:
                continue
            seen.add(float(s[i]))
            si = dtype(s[i])
            out.append(BandThreshold(float(si), int(r[i]), int(c[i]), False, "at"))
            out.append(BandThreshold(float(np.nextafter(si, dtype(0))), int(r[i]), int(c[i]), True, "below"))
            if len(seen) == BAND_SCORES_PER_BAND:
                break
    out.append(BandThreshold(1.0, -1, -1, True, "plain"))
    return tuple(out)


def thresholds(case: str, dtype) -> tuple:
    """every threshold a form is run at on ``case``: t and the number below t, or the band's own"""
    if case == "band":
        return tuple(bt.thr for bt in band_thresholds(dtype))
    return tuple(thr for t in THRESHOLDS[case] for thr in (t, pred(t, dtype)))
