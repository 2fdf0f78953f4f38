"""Inputs for the grouping of identical rows (sg_collapse.hip) and what numpy expects of them.

The matrices are built as CSR, not from names.  Every hub row is ``{c: 0.5, c + 1: 0.5}`` on a column pair of its own: all
scores are exact in f32 and f64, squared row norms stay <= 1 (the index build groups such a matrix), and rows of different
hubs score 0.  Rows are shuffled with a fixed seed, so that arrival order in the hash table is not row order."""
import numpy as np
import scipy.sparse as sp

TOP_N = 10
THRESHOLD = 0.2
LEFT_ROWS = 4000                 # the one-sided product: rows [0, LEFT_ROWS) against the whole list
SORT_LDS = 8192                  # SG_GROUP_SORT_LDS: the largest group a workgroup sorts in LDS
LARGE_MAX = 28                   # SG_GROUP_LARGE_MAX: very large groups the table path lists itself

SIZES = [2, 3, 32, 33, SORT_LDS, SORT_LDS + 1, 9000]
WIDE = (3, 200)                  # three rows of 200 entries of 2^-4: the pruned multiply hands them to the exact kernel
N_EMPTY = 5


def build(sizes, n_single, seed, dtype, extras=True):
    """A hub of every size in ``sizes``, ``n_single`` rows that stand alone and -- with ``extras`` -- a group of 2 that
    equals the first hub but for one value one ulp lower, a group of 2 that is the first hub's first entry alone (a prefix:
    it scores 0.25 against the first hub and its near-copy), WIDE[0] identical rows of WIDE[1] entries and N_EMPTY rows
    without entries."""
    rng = np.random.default_rng(seed)
    types = []
    col = 0
    for s in sizes:
        types.append((np.array([col, col + 1]), np.array([0.5, 0.5]), s))
        col += 2
    for _ in range(n_single):
        types.append((np.array([col]), np.array([1.0]), 1))
        col += 1
    if extras:
        types.append((np.array([0, 1]), np.array([0.5, np.nextafter(dtype(0.5), dtype(0))]), 2))
        types.append((np.array([0]), np.array([0.5]), 2))
        types.append((np.arange(col, col + WIDE[1]), np.full(WIDE[1], 2.0 ** -4), WIDE[0]))
        col += WIDE[1]
        types.append((np.array([], dtype=np.int64), np.array([]), N_EMPTY))
    which = np.concatenate([np.full(t[2], i) for i, t in enumerate(types)])
    which = which[rng.permutation(len(which))]
    lens = np.array([len(t[0]) for t in types])[which]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([types[i][0] for i in which]).astype(np.int32)
    data = np.concatenate([types[i][1] for i in which]).astype(dtype)
    return sp.csr_matrix((data, indices, indptr), shape=(len(which), col))


def sizes(dtype):
    return build(SIZES, 300, 1, dtype)


def hubs(n_hubs, dtype):
    """``n_hubs`` groups of SORT_LDS + 1 rows and 40 single rows.  Built in f32 and widened: both dtypes hold the same
    numbers, so the port's f32 result serves both wherever its scores are exact (all rows but those on the first hub's columns)."""
    return build([SORT_LDS + 1] * n_hubs, 40, 2, np.float32).astype(dtype)


def barely(n_groups, dtype):
    """10 000 rows in ``n_groups`` groups: pairs and single rows only"""
    pairs = 10000 - n_groups
    return build([2] * pairs, n_groups - pairs, 3, dtype, extras=False)


def tiny(which, dtype):
    rows = {"two_same": [0, 0], "three_two_same": [0, 1, 0], "three_distinct": [0, 1, 2]}[which]
    indices = np.array([[2 * t, 2 * t + 1] for t in rows], dtype=np.int32).ravel()
    return sp.csr_matrix((np.full(len(indices), 0.5, dtype), indices, 2 * np.arange(len(rows) + 1, dtype=np.int64)),
                         shape=(len(rows), 6))


def expected_gid(A):
    """numpy's numbering of the distinct rows by first occurrence, over (indices bytes, data bytes)"""
    seen = {}
    gid = np.empty(A.shape[0], np.int64)
    for r, (a, b) in enumerate(zip(A.indptr[:-1], A.indptr[1:])):
        gid[r] = seen.setdefault((A.indices[a:b].tobytes(), A.data[a:b].tobytes()), len(seen))
    return gid, len(seen)


def expected_members(gid):
    """(rows of group 0 ascending, then those of group 1, ..., the groups' sizes)"""
    return np.argsort(gid, kind="stable"), np.bincount(gid)
