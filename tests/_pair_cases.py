"""What sg_csr_pairs_dot (csrc/sg_pairs.hip) is held to, for the CPU and the GPU tests alike.  TEST INFRASTRUCTURE ONLY.

- ``ref_pairs_dot``: the value in numpy -- acc = +0.0, and for every column both rows hold, ascending, acc = rn(acc + rn(a * b));
- ``wrong_pairs_dot``: the turns a kernel could take instead (numpy's pairwise sum, descending columns, a fused multiply-add,
  a wider accumulator, the first product as the start, zero products left out), each as a ``variant``;
- ``walk_model``: the kernel's own walk -- eight lanes a pair, the rows in chunks of eight entries, a merge by chunks, the
  products of a retired chunk added in lane order -- in plain Python, so that the walk is held to the statement without a GPU;
- ``cases(dtype)``: the matrices and pair lists, built where the walk can go wrong."""
import functools
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

DTYPES = [np.float32, np.float64]
LANES = 8                 # SG_PAIR_LANES: lanes a pair, and entries a chunk
WAVE_PAIRS = 64 // LANES  # pairs a wave
BLOCK_PAIRS = 256 // LANES
N_COLS = 4096


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, want) -> bool:
    """Equal dtype, shape and bit patterns: -0.0 is not +0.0 here, and a NaN equals itself."""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------ the statement
def _row(m, i):
    return m.indices[m.indptr[i]:m.indptr[i + 1]], m.data[m.indptr[i]:m.indptr[i + 1]]


def _common(A, B, i, j):
    (ka, va), (kb, vb) = _row(A, i), _row(B, j)
    _, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)     # ascending column
    return va[ia], vb[ib]


def ref_pairs_dot(A: sp.csr_matrix, B: sp.csr_matrix, left, right) -> np.ndarray:
    """out[p] = (A . B^T)[left[p], right[p]] in the multiply's arithmetic.  ufunc.accumulate adds one after the other, left
    to right, in the array's own type; numpy's multiply rounds every product to it."""
    T = A.dtype.type
    out = np.zeros(len(left), T)
    with np.errstate(all="ignore"):
        for p, (i, j) in enumerate(zip(left, right)):
            a, b = _common(A, B, int(i), int(j))
            out[p] = np.add.accumulate(np.concatenate([np.zeros(1, T), (a * b).astype(T)]), dtype=T)[-1]
    return out


def _np_pairwise(prod, T):
    """K9's sum (sg_reduce.hip): the first product + numpy's pairwise sum of the rest, zero products left out."""
    prod = prod[prod != 0]
    if len(prod) == 0:
        return T(0)
    return prod[0] if len(prod) == 1 else T(prod[0] + np.add.reduce(prod[1:], dtype=T))


def _round_to(frac: Fraction, T):
    """A rational number rounded ONCE to T (float() of a Fraction is correctly rounded; for float32 the double in between
    holds every sum of a float32 and a product of two exactly enough that the second rounding decides alone but on a tie of
    it, which these values do not make)."""
    return T(float(frac))


def wrong_pairs_dot(A, B, left, right, variant: str) -> np.ndarray:
    T = A.dtype.type
    out = np.zeros(len(left), T)
    with np.errstate(all="ignore"):
        for p, (i, j) in enumerate(zip(left, right)):
            a, b = _common(A, B, int(i), int(j))
            prod = (a * b).astype(T)
            if variant == "pairwise":
                out[p] = _np_pairwise(prod, T)
            elif variant == "descending":
                out[p] = np.add.accumulate(np.concatenate([np.zeros(1, T), prod[::-1]]), dtype=T)[-1]
            elif variant == "fma":
                acc = T(0)
                for x, y in zip(a, b):
                    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(acc)):
                        acc = T(acc + x * y)
                    else:
                        acc = _round_to(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(acc)), T)
                out[p] = acc
            elif variant == "wide_accumulator":       # float32: sums in double, rounded once at the end
                out[p] = T(np.add.accumulate(np.concatenate([np.zeros(1), prod.astype(np.float64)]))[-1])
            elif variant == "from_first":
                out[p] = T(0) if len(prod) == 0 else np.add.accumulate(prod, dtype=T)[-1]
            elif variant == "skip_zero":
                kept = prod[prod != 0]
                out[p] = np.add.accumulate(np.concatenate([np.zeros(1, T), kept]), dtype=T)[-1]
            else:
                raise ValueError(variant)
    return out


# ------------------------------------------------------------------------------------------ the kernel's walk
def walk_model(A, B, left, right) -> np.ndarray:
    """csrc/sg_pairs.hip, pairs_dot_kernel, lane by lane: the group holds one chunk of each row, every lane of A's chunk looks
    for its column among B's chunk, the chunk whose last column is the smaller is retired (A's: its products are added, lane 0
    first), and what A's current chunk has met when B runs out is added last."""
    T = A.dtype.type
    G = LANES
    out = np.zeros(len(left), T)
    with np.errstate(all="ignore"):
        for p, (i, j) in enumerate(zip(left, right)):
            (ka_all, va_all), (kb_all, vb_all) = _row(A, int(i)), _row(B, int(j))
            na, nb = len(ka_all), len(kb_all)
            pa = pb = 0
            acc = T(0)
            prod, hit = [T(0)] * G, [False] * G

            def retire(acc):
                for s in range(G):
                    if hit[s]:
                        acc = T(acc + prod[s])
                return acc

            while pa < na and pb < nb:
                ka = [int(ka_all[pa + l]) if pa + l < na else -2 for l in range(G)]
                kb = [int(kb_all[pb + l]) if pb + l < nb else -1 for l in range(G)]
                for l in range(G):
                    for s in range(G):
                        if kb[s] == ka[l]:
                            prod[l], hit[l] = T(va_all[pa + l] * vb_all[pb + s]), True
                last_a, last_b = ka[min(G, na - pa) - 1], kb[min(G, nb - pb) - 1]
                if last_a <= last_b:
                    acc = retire(acc)
                    hit = [False] * G
                    pa += G
                if last_b <= last_a:
                    pb += G
            if pa < na:
                acc = retire(acc)
            out[p] = acc
    return out


# ------------------------------------------------------------------------------------------ the cases
def csr_of(rows, dtype, n_cols=N_COLS) -> sp.csr_matrix:
    """rows: a list of (columns ascending, values).  The arrays as given: nothing is summed, sorted or dropped."""
    indptr = np.cumsum([0] + [len(c) for c, _ in rows]).astype(np.int64)
    cols = np.concatenate([np.asarray(c, np.int32) for c, _ in rows] + [np.zeros(0, np.int32)])
    vals = np.concatenate([np.asarray(v, dtype) for _, v in rows] + [np.zeros(0, dtype)])
    m = sp.csr_matrix((vals, cols, indptr), shape=(len(rows), n_cols))
    m.has_sorted_indices = True
    assert all(np.all(np.diff(np.asarray(c, np.int64)) > 0) for c, _ in rows), "a case row is not strictly ascending"
    return m


def _values(rng, n, dtype):
    """Both signs, magnitudes over six decades: every sum rounds, and the order of the adds shows."""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(dtype)


ROW_LENGTHS = (0, 1, LANES - 1, LANES, LANES + 1, 2 * LANES - 1, 2 * LANES, 2 * LANES + 1, 63, 64, 65, 1023, 1024, 1025, 1100)


def _length_rows(rng, dtype, universe):
    return [(np.sort(rng.choice(universe, n, replace=False)), _values(rng, n, dtype)) for n in ROW_LENGTHS]


def _structured_rows(rng, dtype):
    """(rows of A, rows of B, pairs): the places of the common columns."""
    a_rows, b_rows, pairs = [], [], []

    def add(ca, cb):
        a_rows.append((np.asarray(ca), _values(rng, len(ca), dtype)))
        b_rows.append((np.asarray(cb), _values(rng, len(cb), dtype)))
        pairs.append((len(a_rows) - 1, len(b_rows) - 1))

    for n in (1, LANES, LANES + 1, 2 * LANES + 1, 20):
        lo, hi = np.arange(1, n), np.arange(1001, 1000 + n)
        add(np.r_[500, hi], np.r_[lo, 500])                 # the only common column: A's first entry, B's last
        add(np.r_[lo, 500], np.r_[500, hi])                 # ... A's last, B's first
        add(np.r_[500, hi], np.r_[500, hi + 2000])          # ... the first of both
        add(np.r_[lo, 500], np.r_[lo + 200, 500])           # ... the last of both
        add(np.arange(n) * 3, np.arange(n) * 3)             # all columns common
        add(np.arange(n), np.arange(n) + 2000)              # none common: A wholly before B
        add(np.arange(n) + 2000, np.arange(n))              # ... B wholly before A
        add(np.arange(n) * 2, np.arange(n) * 2 + 1)         # interleaved, none common
        add(np.arange(n) * 2, np.arange(n + 3) * 3)         # interleaved, every third of A common
    add(np.arange(40), np.arange(5, 1100))                  # a short row against a long one, all of the short one's tail common
    add(np.arange(5, 1100), np.arange(40))
    return a_rows, b_rows, pairs


def _arithmetic_rows(rng, dtype):
    """Rows on which every wrong turn of ``wrong_pairs_dot`` changes an answer: 200 common columns (past numpy's blocks of
    128) of values over six decades and both signs; a lone product of -0.0; -0.0 products among others; products that are 0."""
    a_rows, b_rows, pairs = [], [], []

    def add(cols, va, vb):
        a_rows.append((np.asarray(cols), np.asarray(va, dtype)))
        b_rows.append((np.asarray(cols), np.asarray(vb, dtype)))
        pairs.append((len(a_rows) - 1, len(b_rows) - 1))

    for n in (3, 9, 40, 200):
        for _ in range(4):
            add(np.arange(n) * 7, _values(rng, n, dtype), _values(rng, n, dtype))
    add([3], [-1.0], [0.0])                                 # a lone -0.0: +0.0 + -0.0 = +0.0
    add([3, 9], [-1.0, 2.0], [0.0, -0.0])                   # two of them
    add([3, 9, 11], [0.0, 1.5, 0.0], [5.0, 2.5, -1.0])      # zero products around a real one
    add([3, 9], [1.0, -1.0], [0.25, 0.25])                  # x + (-x) = +0.0
    return a_rows, b_rows, pairs


@functools.lru_cache(maxsize=None)
def cases(dtype):
    """name -> (A, B, left, right); A is B (the same object) where the case is a self-join."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(20260 + np.dtype(dtype).itemsize)
    out = {}
    # every length against every length, from a universe small enough that rows overlap; i == j on the diagonal
    M = csr_of(_length_rows(rng, dtype, 2048), dtype)
    M2 = csr_of(_length_rows(rng, dtype, 2048), dtype)
    n = len(ROW_LENGTHS)
    ii, jj = [x.ravel() for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    out["lengths_self"] = (M, M, ii, jj)
    out["lengths_two_sided"] = (M, M2, ii, jj)
    a_rows, b_rows, pairs = _structured_rows(rng, dtype)
    SA, SB = csr_of(a_rows, dtype), csr_of(b_rows, dtype)
    pl, pr = np.array(pairs).T
    out["structured"] = (SA, SB, pl, pr)
    out["same_pair_twice"] = (SA, SB, np.r_[pl[:5], pl[:5], pl[4]], np.r_[pr[:5], pr[:5], pr[4]])
    out["hub_row"] = (M, M2, np.arange(n).repeat(3), np.full(3 * n, 9))
    a_rows, b_rows, pairs = _arithmetic_rows(rng, dtype)
    pl, pr = np.array(pairs).T
    out["arithmetic"] = (csr_of(a_rows, dtype), csr_of(b_rows, dtype), pl, pr)
    # pair counts around the kernel's group (one pair), wave and block sizes; rows of names' lengths
    K = csr_of([(np.sort(rng.choice(300, k, replace=False)), _values(rng, k, dtype)) for k in rng.integers(0, 41, 97)], dtype)
    for count in (1, 2, WAVE_PAIRS - 1, WAVE_PAIRS, WAVE_PAIRS + 1, BLOCK_PAIRS - 1, BLOCK_PAIRS, BLOCK_PAIRS + 1,
                  2 * BLOCK_PAIRS - 1, 2 * BLOCK_PAIRS, 2 * BLOCK_PAIRS + 1, 1000):
        out[f"count_{count}"] = (K, K, rng.integers(0, 97, count), rng.integers(0, 97, count))
    return out


@functools.lru_cache(maxsize=None)
def expected(dtype, name):
    """The reference of a case, computed once."""
    A, B, left, right = cases(dtype)[name]
    want = ref_pairs_dot(A, B, left, right)
    want.setflags(write=False)
    return want


def special_values_case(dtype):
    """NaN and inf flow through, values of any sign: no gate."""
    dtype = np.dtype(dtype).type
    rows_a = [([1, 4, 9], [np.inf, 1.0, -2.0]), ([1, 4], [np.nan, 1.0]), ([2, 3], [-1.0, -3.0]), ([1], [np.inf]), ([5], [0.0])]
    rows_b = [([1, 4, 9], [1.0, 2.0, 3.0]), ([1, 4], [1.0, 1.0]), ([2, 3], [4.0, -0.5]), ([1], [-np.inf]), ([5], [np.inf])]
    A, B = csr_of(rows_a, dtype), csr_of(rows_b, dtype)
    left = np.array([0, 1, 2, 3, 4, 0, 3])
    right = np.array([0, 1, 2, 3, 4, 3, 0])
    return A, B, left, right
