"""Caller-made CSR matrices whose rows pin down how the pruned multiply deals a wave's 64 lanes to a row's prefix terms
(string_grouper_amd/csrc/sg_k4_device.h).  TEST INFRASTRUCTURE ONLY: host arrays, numpy / scipy, the oracle's port; no GPU
and no library.  tests/test_lane_dealing_gpu.py multiplies each matrix with itself in every form and dealing and expects
the port's bits.

Every matrix is made of FAMILIES: rows over the same columns whose values are one base vector times a few per cent of
noise, normalised to length 1 (rounded to the dtype: the squared norms differ from 1 by a few ulp).  The members of a
family score 0.99 and more with each other -- the planted near-duplicates: matches above 0.8 in every case -- and nothing
or one shared term's worth (below 0.2) with anybody else.  A column's posting list is the set of rows that hold it, so the
size of a family IS the length of its columns' lists.  The rows are shuffled: a list's entries lie all over the index.

  rare     4 000 rows; a term is frequent from 0.5 % of the rows = 20 entries on, every list here holds 19 at most, so
           every term of a row is a prefix term: np = nnz.  Families of 19 rows over 1, 2, 63 and 64 columns (a lane a
           term at 64: a list of 19 takes five rounds of four entries) and over 3 .. 40 columns to fill up.
  skewed   40 000 rows = two super-tiles of 32 768 columns: a lane's stream crosses a visit's boundary.  Rows with ONE list
           of 199 entries (frequent from 200 on) beside ten lists of 2 -- the floor rule leaves five lanes idle there,
           49 + 10 x 1, the remainders give them to the first five short lists -- and rows whose nine lists are all equal
           (12 entries): every remainder ties, the lane left over goes to the first term.
  wide     4 000 rows, 600 of them with 65 .. 128 entries of which 60 .. 64 are prefix terms (lists of 6) and the rest
           frequent terms (68 columns that 24 and more rows hold) carrying 0.3 of the squared norm -- inside the suffix's
           budget ((0.8 - 0.05)^2 = 0.56 at the least) -- with random column numbers, so that the prefix terms lie in both
           halves of the sorted row: the launch over two terms a lane.
Every builder is seeded and cached; the arrays are shared: do not write to them."""
import functools

import numpy as np
import scipy.sparse as sp

DTYPES = (np.float32, np.float64)
CASES = ("rare", "skewed", "wide")
THRESHOLD = 0.8
TOP_N = 32          # more than any row has matches: nothing is cut, every match is compared
SEED = 20240611


def _family(rng, n_rows, n_cols, weights=None):
    """values of a family: n_rows near-copies of one direction over n_cols columns, each of length 1 (float64)"""
    base = rng.uniform(0.5, 1.0, n_cols) if weights is None else np.asarray(weights, np.float64)
    v = base[None, :] * (1.0 + 0.04 * rng.uniform(-1.0, 1.0, (n_rows, n_cols)))
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True))


def _assemble(rng, rows, n_cols, dtype):
    """rows: [(columns, values)] in family order -> the shuffled CSR matrix, columns renumbered at random and sorted"""
    relabel = rng.permutation(n_cols)
    order = rng.permutation(len(rows))
    indptr = np.zeros(len(rows) + 1, np.int64)
    ind, dat = [], []
    for out_i, i in enumerate(order):
        c = relabel[np.asarray(rows[i][0], np.int64)]
        o = np.argsort(c, kind="stable")
        assert (np.diff(c[o]) > 0).all()
        ind.append(c[o])
        dat.append(np.asarray(rows[i][1], np.float64)[o])
        indptr[out_i + 1] = indptr[out_i] + len(c)
    m = sp.csr_matrix((np.concatenate(dat).astype(dtype), np.concatenate(ind).astype(np.int32), indptr), shape=(len(rows), n_cols))
    m.has_sorted_indices = True
    return m


class _Columns:
    def __init__(self):
        self.n = 0

    def take(self, k):
        out = np.arange(self.n, self.n + k)
        self.n += k
        return out


RARE_ROWS, RARE_LIST = 4000, 19
RARE_WIDTHS = (1, 2, 63, 64)


@functools.lru_cache(maxsize=None)
def rare(dtype) -> sp.csr_matrix:
    rng = np.random.default_rng(SEED)
    cols, rows = _Columns(), []
    widths = [w for w in RARE_WIDTHS for _ in range(6)]
    while (len(widths) + 1) * RARE_LIST <= RARE_ROWS:
        widths.append(int(rng.integers(3, 41)))
    sizes = [RARE_LIST] * len(widths)
    if RARE_ROWS - sum(sizes):
        widths.append(16)
        sizes.append(RARE_ROWS - sum(sizes))        # the last family is shorter: lists of what is left
    for w, n in zip(widths, sizes):
        c = cols.take(w)
        for v in _family(rng, n, w):
            rows.append((c, v))
    assert len(rows) == RARE_ROWS
    return _assemble(rng, rows, cols.n, dtype)


SKEWED_ROWS, SKEWED_LONG, SKEWED_LONG_FAMILIES, SKEWED_EQUAL, SKEWED_EQUAL_WIDTH = 40000, 199, 100, 12, 9


@functools.lru_cache(maxsize=None)
def skewed(dtype) -> sp.csr_matrix:
    rng = np.random.default_rng(SEED + 1)
    cols, rows = _Columns(), []
    for _ in range(SKEWED_LONG_FAMILIES):
        h = cols.take(1)                              # the list of 199: one term of every row of the family
        for p in range(SKEWED_LONG // 2 + 1):         # 99 pairs of near-duplicates and one row alone (its ten lists hold 1)
            n = 2 if p < SKEWED_LONG // 2 else 1
            c = np.concatenate([h, cols.take(10)])
            for v in _family(rng, n, 11, weights=np.concatenate([[0.9], rng.uniform(0.5, 1.0, 10)])):
                rows.append((c, v))
    n_equal = (SKEWED_ROWS - len(rows)) // SKEWED_EQUAL
    assert len(rows) + n_equal * SKEWED_EQUAL == SKEWED_ROWS
    for _ in range(n_equal):
        c = cols.take(SKEWED_EQUAL_WIDTH)
        for v in _family(rng, SKEWED_EQUAL, SKEWED_EQUAL_WIDTH):
            rows.append((c, v))
    return _assemble(rng, rows, cols.n, dtype)


WIDE_ROWS, WIDE_FAMILY, WIDE_FREQUENT_COLUMNS, WIDE_FREQUENT_NORM2 = 4000, 6, 68, 0.3
# (prefix terms, frequent terms) of the wide families: 65 and 128 entries, 60 and 64 prefix terms, and what lies between;
# the first four hold every frequent column, which makes each of them a list of 24 entries at the least
WIDE_SHAPES = ((60, 68), (60, 68), (60, 68), (60, 68), (64, 1), (64, 64), (60, 5), (63, 2), (62, 30), (61, 40), (64, 33), (63, 65))


@functools.lru_cache(maxsize=None)
def wide(dtype) -> sp.csr_matrix:
    rng = np.random.default_rng(SEED + 2)
    cols, rows = _Columns(), []
    frequent = cols.take(WIDE_FREQUENT_COLUMNS)
    n_families = 600 // WIDE_FAMILY
    for f in range(n_families):
        n_p, n_f = WIDE_SHAPES[f % len(WIDE_SHAPES)]
        fc = frequent if n_f == WIDE_FREQUENT_COLUMNS else rng.permutation(frequent)[:n_f]
        c = np.concatenate([fc, cols.take(n_p)])
        wf = rng.uniform(0.5, 1.0, n_f)
        wp = rng.uniform(0.5, 1.0, n_p)
        wf *= np.sqrt(WIDE_FREQUENT_NORM2 / (wf * wf).sum())
        wp *= np.sqrt((1.0 - WIDE_FREQUENT_NORM2) / (wp * wp).sum())
        for v in _family(rng, WIDE_FAMILY, n_f + n_p, weights=np.concatenate([wf, wp])):
            rows.append((c, v))
    while len(rows) < WIDE_ROWS:                      # the rest: pairs over 16 columns of their own
        c = cols.take(16)
        for v in _family(rng, 2, 16):
            rows.append((c, v))
    assert len(rows) == WIDE_ROWS
    return _assemble(rng, rows, cols.n, dtype)


def matrix(case: str, dtype) -> sp.csr_matrix:
    return {"rare": rare, "skewed": skewed, "wide": wide}[case](dtype)


def list_lengths(m: sp.csr_matrix) -> np.ndarray:
    """entries of every column's posting list"""
    return np.bincount(m.indices, minlength=m.shape[1])


def frequent_from(m: sp.csr_matrix) -> int:
    """the list length from which the index build calls a term frequent: 0.5 % of the rows"""
    return max(1, int(0.005 * m.shape[0]))


_PORT = {}


def port(case: str, dtype):
    """The port's answer for the case's self-product, computed once and shared: do not write to it."""
    from oracle import port as P
    key = (case, np.dtype(dtype).name)
    if key not in _PORT:
        A = matrix(case, dtype)
        _PORT[key] = P.sp_matmul_topn_port(A, A.T, TOP_N, THRESHOLD, True, 8)
    return _PORT[key]
