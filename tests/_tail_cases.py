"""Constructed inputs, plain references and deliberately wrong references ("mutants") for the kernels that run after the
multiply: K5 (sg_topn_zip), K6 (sg_matchlist_build), K7 (sg_matchlist_best_master), K8 (sg_matchlist_group_reps),
K9 (sg_csr_rowwise_dot) and sg_row_costs.  TEST INFRASTRUCTURE ONLY: host arrays, numpy / scipy / pandas, no GPU and no
library.  tests/test_tail_references_cpu.py proves that the inputs tell every mutant from its reference;
tests/test_tail_gpu.py feeds the same inputs to the kernels and expects the references' bits.

A reference is the operation the reference project performs on the same arrays (string_grouper.py line numbers in the
docstrings), not a restatement of a kernel.  Every builder is seeded and cached: the arrays it returns are shared and
must not be written to.
"""
import functools
from typing import NamedTuple

import numpy as np
import pandas as pd
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

DTYPES = (np.float32, np.float64)

# Lengths of the "rest" of a row (row length minus one: numpy's reduceat adds the first element to the pairwise sum of the
# others) around every branch of numpy's pairwise sum: fewer than 8 sequentially; 8 .. 128 in eight strided partial sums
# with a sequential tail; longer runs split into halves rounded down to a multiple of 8.  257 and 300 split into halves of
# which one (257: 128 + 129) or both (300: 144 + 156) split again.
BOUNDARY_RESTS = (0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 300)
# Two-candidate components per length of the centroid sweep.  A fixed-stride input costs rows x stride cells, and a component
# of row length L needs L + 1 column nodes, so a length costs about N * L^2 cells: 400 keeps the longest at 440 MB of (mostly
# untouched) float64 cells.  A left-to-right sum changes the representative of 33 - 52 % of these components (the sign of
# the difference of the two sums flips; counted in tests/test_tail_references_cpu.py): 130 - 210 per length.
SWEEP_COMPONENTS = 400


class TopN(NamedTuple):
    """A fixed-stride result as sg_topn_from_host takes it: row i holds counts[i] entries at cols[i, :counts[i]]."""
    cols: np.ndarray      # int32 [n_rows, stride]
    vals: np.ndarray      # float32 / float64 [n_rows, stride]
    counts: np.ndarray    # int32 [n_rows]
    n_cols: int


class CsrList(NamedTuple):
    """A match list as sg_matchlist_to_host returns it."""
    row_ptr: np.ndarray   # int64 [n_rows + 1]
    cols: np.ndarray      # int32
    vals: np.ndarray


def topn_from_rows(row_ptr, cols, vals, n_cols, stride=None) -> TopN:
    row_ptr = np.asarray(row_ptr, np.int64)
    cnt = np.diff(row_ptr).astype(np.int32)
    n = len(cnt)
    if stride is None:
        stride = max(1, int(cnt.max()) if n else 1)
    out_c = np.zeros((n, stride), np.int32)
    out_v = np.zeros((n, stride), np.asarray(vals).dtype)
    r = np.repeat(np.arange(n), cnt)
    p = np.arange(len(cols)) - np.repeat(row_ptr[:-1], cnt)
    out_c[r, p] = cols
    out_v[r, p] = vals
    return TopN(out_c, out_v, cnt, int(n_cols))


def topn_to_list(t: TopN) -> CsrList:
    """The stored entries in their within-row order."""
    mask = np.arange(t.cols.shape[1])[None, :] < t.counts[:, None]
    row_ptr = np.zeros(len(t.counts) + 1, np.int64)
    np.cumsum(t.counts, out=row_ptr[1:])
    return CsrList(row_ptr, t.cols[mask].astype(np.int32), t.vals[mask])


def list_to_csr(ml: CsrList, shape) -> sp.csr_matrix:
    return sp.csr_matrix((ml.vals.copy(), ml.cols.copy(), ml.row_ptr.copy()), shape=shape)


def rows_of(ml: CsrList) -> np.ndarray:
    return np.repeat(np.arange(len(ml.row_ptr) - 1, dtype=np.int64), np.diff(ml.row_ptr))


def check_preconditions(t: TopN, sorted_rows=False):
    """What include/sg_hip.h asks of a fixed-stride input: counts within the stride, columns in range and distinct within a
    row (and ascending where a consumer needs sorted rows)."""
    assert t.cols.dtype == np.int32 and t.counts.dtype == np.int32
    assert t.cols.shape == t.vals.shape and t.cols.shape[0] == len(t.counts)
    assert (t.counts >= 0).all() and (t.counts <= t.cols.shape[1]).all()
    assert (t.cols >= 0).all() and (t.cols < max(t.n_cols, 1)).all()
    ml = topn_to_list(t)
    key = rows_of(ml) * max(t.n_cols, 1) + ml.cols
    assert len(np.unique(key)) == len(key), "a row names a column twice"
    if sorted_rows:
        assert (np.diff(key) > 0).all(), "rows are not sorted by column"


# ===================================================================================================== K5: zip
class ZipCase(NamedTuple):
    parts: tuple          # of TopN, one per column block
    offsets: np.ndarray   # int64, column offset of every part
    n_cols: int


ZIP_TOP_N = (1, 6, 63, 64, 65, 127, 128, 129, 200)
# strides of the parts; with nine values of top_n every layout is cut inside the first pass, at 64, inside the second pass,
# at 128, beyond it, and (1000) above the sum of the strides
ZIP_LAYOUTS = {1: (210,), 2: (70, 150), 5: (3, 64, 65, 100, 1), 9: (10, 1, 80, 7, 64, 30, 2, 129, 5)}


def _mixed_scores(rng, m, dtype):
    """Half of the scores from three levels (long runs of equal scores wherever the cut falls), half full-mantissa."""
    s = np.where(rng.random(m) < 0.5, rng.choice(np.array([0.25, 0.5, 0.75]), m), 0.01 + 0.98 * rng.random(m))
    return s.astype(dtype)


def _straddling_scores(rng, m, dtype):
    """Distinct descending scores except for two runs of equal ones: the first begins at entry 58 .. 63 and is 4 .. 10 long
    (it crosses entries 63 / 64 / 65), the second begins at 122 .. 127 (it crosses 127 / 128)."""
    s = np.sort((0.01 + 0.98 * rng.random(m)).astype(dtype))[::-1].copy()
    for start in (int(rng.integers(58, 64)), int(rng.integers(122, 128))):
        run = int(rng.integers(4, 11))
        if start + run <= m:
            s[start:start + run] = s[start]
    return s


def _zip_parts(seed, dtype, strides, scores, n_rows=150, sort_rows=True, empty_part=None, all_full=False, reverse_offsets=False):
    rng = np.random.default_rng(seed)
    widths = [max(2 * s, s + 5) for s in strides]
    offsets = np.concatenate([[0], np.cumsum(widths)])[:-1].astype(np.int64)
    if reverse_offsets:      # the first part holds the highest columns
        offsets = (np.concatenate([[0], np.cumsum(widths[::-1])])[:-1][::-1]).astype(np.int64)
    cols = [np.zeros((n_rows, s), np.int32) for s in strides]
    vals = [np.zeros((n_rows, s), dtype) for s in strides]
    counts = [np.zeros(n_rows, np.int32) for _ in strides]
    for i in range(n_rows):
        if i % 11 == 3 and not all_full:
            continue                                   # a row that is empty in every part
        full = all_full or i % 4 == 0                  # a row filled to the stride in every part
        cnt = [0 if b == empty_part else (s if full else int(rng.integers(0, s + 1))) for b, s in enumerate(strides)]
        local = [rng.choice(w, c, replace=False) for w, c in zip(widths, cnt)]
        m = sum(cnt)
        score = rng.permutation(scores(rng, m, dtype))
        at = 0
        for b, c in enumerate(cnt):
            sc, lc = score[at:at + c], local[b]
            at += c
            order = np.lexsort((lc, -sc)) if sort_rows else rng.permutation(c)
            cols[b][i, :c] = lc[order]
            vals[b][i, :c] = sc[order]
            counts[b][i] = c
    parts = tuple(TopN(c, v, n, w) for c, v, n, w in zip(cols, vals, counts, widths))
    for p in parts:
        check_preconditions(p)
    return ZipCase(parts, offsets, int(sum(widths)))


@functools.lru_cache(maxsize=None)
def zip_case(name, dtype) -> ZipCase:
    """'parts1' / 'parts2' / 'parts5' / 'parts9': the layouts of ZIP_LAYOUTS, in 'parts5' the first part has all
    counts zero; 'straddle': three full parts of 90 whose equal scores cross entries 63 / 64 / 65 and 127 / 128;
    'unsorted': the parts arrive in random order within a row; 'reversed': the first part holds the highest columns."""
    seed = 5000 + sorted(ZIP_CASES).index(name) * 2 + (dtype is np.float64)
    if name.startswith("parts"):
        k = int(name[5:])
        return _zip_parts(seed, dtype, ZIP_LAYOUTS[k], _mixed_scores, empty_part=0 if k == 5 else None)
    if name == "straddle":
        return _zip_parts(seed, dtype, (90, 90, 90), _straddling_scores, all_full=True)
    if name == "unsorted":
        return _zip_parts(seed, dtype, (40, 90, 76), _mixed_scores, sort_rows=False)
    if name == "reversed":
        return _zip_parts(seed, dtype, (70, 50, 90), _mixed_scores, reverse_offsets=True)
    raise KeyError(name)


ZIP_CASES = ("parts1", "parts2", "parts5", "parts9", "straddle", "unsorted", "reversed")


def _zip_select(case: ZipCase, top_n, select):
    """select(columns, scores) -> the positions kept, in output order."""
    n = len(case.parts[0].counts)
    stride = max(1, min(top_n, sum(p.cols.shape[1] for p in case.parts)))
    dtype = case.parts[0].vals.dtype
    out = TopN(np.zeros((n, stride), np.int32), np.zeros((n, stride), dtype), np.zeros(n, np.int32), case.n_cols)
    for i in range(n):
        c = np.concatenate([p.cols[i, :p.counts[i]].astype(np.int64) + off for p, off in zip(case.parts, case.offsets)])
        v = np.concatenate([p.vals[i, :p.counts[i]] for p in case.parts])
        keep = select(c, v)
        out.cols[i, :len(keep)] = c[keep]
        out.vals[i, :len(keep)] = v[keep]
        out.counts[i] = len(keep)
    return out


def ref_zip(case: ZipCase, top_n) -> TopN:
    """zip_sp_matmul_topn (string_grouper.py:746): all parts' entries of a row under their column offsets, by score
    descending, then column ascending, cut at top_n."""
    return _zip_select(case, top_n, lambda c, v: np.lexsort((c, -v))[:top_n])


def mutant_zip_arrival_order(case: ZipCase, top_n) -> TopN:
    """Equal scores in the order they arrive instead of by column."""
    return _zip_select(case, top_n, lambda c, v: np.argsort(-v, kind="stable")[:top_n])


def mutant_zip_forgets_floor_column(case: ZipCase, top_n) -> TopN:
    """Passes of 64; a later pass resumes strictly below the previous pass's last SCORE and so loses that score's other
    columns."""
    def select(c, v):
        order = np.lexsort((c, -v))
        kept = list(order[:64])
        while len(kept) % 64 == 0 and len(kept) > 0:
            nxt = [p for p in order if v[p] < v[kept[-1]]][:64]
            if not nxt:
                break
            kept += nxt
        return np.array(kept[:top_n], dtype=np.int64)
    return _zip_select(case, top_n, select)


# ===================================================================================================== K6: match list
def _pair_value(r, c, dtype):
    """A value in (0, 1) that depends on the unordered pair only: a stored pair and its stored mirror carry the same one,
    as the multiply guarantees and K6 assumes."""
    lo, hi = np.minimum(r, c).astype(np.int64), np.maximum(r, c).astype(np.int64)
    return (((lo * 2654435761 + hi * 40503) % 99991 + 1) / 99993.0).astype(dtype)


def _random_rows(rng, n_rows, n_cols, stride, dtype, fill, diag_prob=0.0, own_order=True):
    """Rows of 0 .. stride distinct random columns (`fill(i)` -> count), optionally with the diagonal, in random within-row
    order (the multiply orders by score, never by column)."""
    ptr, cols = [0], []
    for i in range(n_rows):
        k = min(fill(i), n_cols)
        c = rng.choice(n_cols, k, replace=False)
        if k and i < n_cols and rng.random() < diag_prob and i not in c:
            c[0] = i
        cols.append(rng.permutation(c) if own_order else np.sort(c))
        ptr.append(ptr[-1] + k)
    cols = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    rows = np.repeat(np.arange(n_rows), np.diff(ptr))
    vals = _pair_value(rows, cols, dtype)
    return topn_from_rows(ptr, cols, vals, n_cols, stride)


@functools.lru_cache(maxsize=None)
def matchlist_case(name, dtype) -> TopN:
    """Inputs of sg_matchlist_build.
    'square':  700 x 700 (three blocks of rows), stride 9: empty rows, rows filled to the stride, stored diagonals whose value
               is not 1, one-directional pairs and pairs stored from both sides.
    'wide':    600 x 350, stride 12: non-square (the two-series case; no diagonal or mirror is defined there).
    'hub':     20 002 x 20 002, stride 3: column 20 001 is listed by every row, and lists back one of them: 20 000 rows that it
               does not list back.  With symmetrize its row grows from 2 entries to 20 002, far beyond the input stride.
    'one':     1 x 1 with its diagonal stored as 0.5.   'one_empty': 1 x 1 without entries.
    'empty':   40 x 40 without a single entry."""
    rng = np.random.default_rng(6000 + sorted(MATCHLIST_CASES).index(name) * 2 + (dtype is np.float64))
    if name == "square":
        t = _random_rows(rng, 700, 700, 9, dtype, lambda i: 0 if i % 7 == 2 else (9 if i % 5 == 0 else int(rng.integers(1, 9))),
                         diag_prob=0.6)
    elif name == "wide":
        t = _random_rows(rng, 600, 350, 12, dtype, lambda i: 0 if i % 9 == 4 else (12 if i % 4 == 1 else int(rng.integers(1, 12))))
    elif name == "hub":
        n, hub = 20002, 20001
        ptr, cols = [0], []
        for i in range(n - 1):                          # the hub, sometimes the diagonal, sometimes a neighbour
            c = [hub] + ([i] if i % 3 == 0 else []) + ([(i * 7919 + 1) % hub] if i % 2 == 0 and (i * 7919 + 1) % hub != i else [])
            cols.append(rng.permutation(np.array(c)))
            ptr.append(ptr[-1] + len(c))
        cols.append(np.array([hub, 5]))                 # the hub's own row: its diagonal and one row that lists it already
        ptr.append(ptr[-1] + 2)
        cols = np.concatenate(cols).astype(np.int32)
        rows = np.repeat(np.arange(n), np.diff(ptr))
        t = topn_from_rows(ptr, cols, _pair_value(rows, cols, dtype), n, 3)
    elif name == "one":
        t = TopN(np.zeros((1, 2), np.int32), np.array([[0.5, 0.0]], dtype), np.array([1], np.int32), 1)
    elif name == "one_empty":
        t = TopN(np.zeros((1, 1), np.int32), np.zeros((1, 1), dtype), np.zeros(1, np.int32), 1)
    elif name == "empty":
        t = TopN(np.zeros((40, 4), np.int32), np.zeros((40, 4), dtype), np.zeros(40, np.int32), 40)
    else:
        raise KeyError(name)
    check_preconditions(t)
    return t


MATCHLIST_CASES = ("square", "wide", "hub", "one", "one_empty", "empty")
MATCHLIST_SQUARE = ("square", "hub", "one", "one_empty", "empty")


def ref_matchlist(t: TopN, fix_diagonal, symmetrize, sort_by_column) -> CsrList:
    """What fit() does with the multiply's result (string_grouper.py:419-427, :954-964) before _get_matches_list reads it
    (:755-763): tolil(); m[r, r] = 1; m[c, r] = m[r, c] over nonzero(); tocsr().  With neither flag the result is read as it
    is, re-sorted by column only where scipy's up-cast of a float32 block does so (:750)."""
    n = len(t.counts)
    m = list_to_csr(topn_to_list(t), (n, t.n_cols))
    if fix_diagonal or symmetrize:
        m = m.tolil()
        if fix_diagonal:
            r = np.arange(m.shape[0])
            m[r, r] = 1
        if symmetrize:
            r, c = m.nonzero()
            if len(r):
                m[c, r] = m[r, c]
        m = m.tocsr()
        m.sort_indices()
    elif sort_by_column:
        m = m.sorted_indices()
    assert m.dtype == t.vals.dtype
    return CsrList(m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data)


# ===================================================================================================== K7: best master
@functools.lru_cache(maxsize=None)
def best_master_case(name, dtype) -> TopN:
    """Inputs of sg_matchlist_best_master (through sg_matchlist_build with no flag).  All similarities are > 0.
    'wide':   5 003 x 3 001, stride 7.  Only every third column is ever named.  Similarities come from five values one unit
              in the last place apart, so a column's maximum is shared by many rows and differs from the runner-up in the
              last bit.
    'shared': 2 500 x 6: every row names every column with the same similarity except a few rows that exceed it by one ulp.
    'norows': 0 x 9."""
    rng = np.random.default_rng(7000 + sorted(BEST_MASTER_CASES).index(name) * 2 + (dtype is np.float64))
    if name == "wide":
        n_rows, n_cols = 5003, 3001
        named = np.arange(0, n_cols, 3)
        ptr, cols = [0], []
        for i in range(n_rows):
            k = 0 if i % 13 == 5 else int(rng.integers(1, 8))
            cols.append(rng.choice(named, k, replace=False))
            ptr.append(ptr[-1] + k)
        cols = np.concatenate(cols).astype(np.int32)
        levels = np.array([0.7], dtype)
        for _ in range(4):
            levels = np.append(levels, np.nextafter(levels[-1], dtype(2)))
        vals = levels[rng.integers(0, 5, len(cols))].astype(dtype)
        t = topn_from_rows(ptr, cols, vals, n_cols, 7)
    elif name == "shared":
        n_rows, n_cols = 2500, 6
        cols = np.tile(np.arange(n_cols, dtype=np.int32), n_rows)
        vals = np.full(n_rows * n_cols, 0.5, dtype)
        up = np.nextafter(dtype(0.5), dtype(1))
        for c in range(1, n_cols):                      # column 0: all equal; column c: rows 2000 - c*300 + {0, 7, 300} lead
            for r in (2000 - c * 300, 2007 - c * 300, 2300 - c * 300):
                vals[r * n_cols + c] = up
        t = topn_from_rows(np.arange(n_rows + 1) * n_cols, cols, vals, n_cols, n_cols)
    elif name == "norows":
        t = TopN(np.zeros((0, 3), np.int32), np.zeros((0, 3), dtype), np.zeros(0, np.int32), 9)
    else:
        raise KeyError(name)
    check_preconditions(t)
    assert (topn_to_list(t).vals > 0).all()
    return t


BEST_MASTER_CASES = ("wide", "shared", "norows")


def ref_best_master(ml: CsrList, n_cols, ties="min") -> np.ndarray:
    """match_most_similar's reduction (string_grouper.py:803-807): per duplicate the largest similarity, merged back into
    the list, then the lowest master among those; -1 for a duplicate nobody names."""
    frame = pd.DataFrame({"master_side": rows_of(ml), "dupe_side": ml.cols.astype(np.int64), "similarity": ml.vals})
    top = frame.groupby("dupe_side").agg({"similarity": "max"}).reset_index()
    top = top.merge(frame, on=["dupe_side", "similarity"])
    top = top.groupby(["dupe_side"]).agg({"master_side": ties}).reset_index()
    best = np.full(n_cols, -1, np.int32)
    best[top.dupe_side.to_numpy()] = top.master_side.to_numpy()
    return best


def mutant_best_master_highest_row(ml: CsrList, n_cols) -> np.ndarray:
    return ref_best_master(ml, n_cols, ties="max")


# ===================================================================================================== K8: group representatives
class GraphCase(NamedTuple):
    topn: TopN            # square, rows sorted by column (a match list is)
    sweep_pairs: object   # centroid sweep only: int array [components, 2], the two candidates of every component


def _graph_from_edges(n, r, c, rng, dtype, vals=None) -> TopN:
    """Directed edges (r[i], c[i]) as a square list with rows sorted by column; full-mantissa similarities in (0.5, 1)."""
    order = np.lexsort((c, r))
    r, c = np.asarray(r)[order], np.asarray(c)[order]
    vals = (0.5 + 0.5 * rng.random(len(r))).astype(dtype) if vals is None else np.asarray(vals)[order]
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
    return topn_from_rows(ptr, c.astype(np.int32), vals, n)


@functools.lru_cache(maxsize=None)
def centroid_sweep_case(rest, dtype) -> GraphCase:
    """SWEEP_COMPONENTS components, each with exactly two candidates for the centroid: two nodes that list the same
    rest + 1 other nodes (which list nobody: their row sum is 0) with the SAME similarities in a different column order.
    The component's nodes are numbered at random inside its block, so its lowest index is a column node more often than not,
    and every seventh component is followed by an isolated node.
    float64: full-mantissa values; which candidate wins depends on the order of summation alone.
    float32: sums of a few hundred widened float32 are exact in float64, so equal values give an exact tie (the lower index
             wins); in every other component one value of one candidate is raised by one float32 ulp, and that candidate
             wins -- unless the sum is rounded to float32 on the way."""
    rng = np.random.default_rng(8000 + 10 * rest + (dtype is np.float64))
    length = rest + 1
    r, c, v, pairs, base = [], [], [], [], 0
    for k in range(SWEEP_COMPONENTS):
        nodes = base + rng.permutation(length + 2)
        a, b, columns = nodes[0], nodes[1], np.sort(nodes[2:])
        va = (0.5 + 0.5 * rng.random(length)).astype(dtype)
        vb = rng.permutation(va)
        if dtype is np.float32 and k % 2 == 1:
            j = int(rng.integers(length))
            vb[j] = np.nextafter(vb[j], np.float32(2))
        for node, vv in ((a, va), (b, vb)):
            r.append(np.full(length, node))
            c.append(columns)
            v.append(vv)
        pairs.append((a, b))
        base += length + 2 + (k % 7 == 0)
    r, c, v = np.concatenate(r), np.concatenate(c), np.concatenate(v)
    t = _graph_from_edges(base, r, c, rng, dtype, v)
    check_preconditions(t, sorted_rows=True)
    return GraphCase(t, np.array(pairs, np.int64))


@functools.lru_cache(maxsize=None)
def graph_case(name, dtype) -> GraphCase:
    """Square lists for the connected components.  Every edge is stored from ONE side only (scipy's directed=True with
    connection='weak' must still join its ends) unless said otherwise.
    'path_random':  a path of 100 000 nodes under a random renumbering, every edge stored from a random end.
    'path_ordered': the same path numbered along its length, so the lowest index sits at one end and its label has to
                    travel all the way.
    'stars':        400 stars of 30 leaves whose centre has the highest index of the star; the leaves list the centre.
    'stars_out':    the same with the centre listing its leaves (one row of 30 entries).
    'small':        3 000 two-node components stored from BOTH sides with one similarity (equal row sums: the centroid is a
                    tie and the lower index wins), 3 000 three-node components a -> b <- c, and 500 isolated nodes, all under
                    one random renumbering."""
    rng = np.random.default_rng(8500 + sorted(GRAPH_CASES).index(name) * 2 + (dtype is np.float64))
    vals = None
    if name in ("path_random", "path_ordered"):
        n = 100000
        number = rng.permutation(n) if name == "path_random" else np.arange(n)
        flip = rng.random(n - 1) < 0.5
        u, w = number[:-1], number[1:]
        r, c = np.where(flip, w, u), np.where(flip, u, w)
    elif name in ("stars", "stars_out"):
        stars, leaves = 400, 30
        n = stars * (leaves + 1)
        centre = np.repeat(np.arange(stars) * (leaves + 1) + leaves, leaves)
        leaf = (np.arange(stars)[:, None] * (leaves + 1) + np.arange(leaves)[None, :]).ravel()
        r, c = (leaf, centre) if name == "stars" else (centre, leaf)
    elif name == "small":
        pairs, triples, lonely = 3000, 3000, 500
        n = 2 * pairs + 3 * triples + lonely
        number = rng.permutation(n)
        p = number[:2 * pairs].reshape(pairs, 2)
        t = number[2 * pairs:2 * pairs + 3 * triples].reshape(triples, 3)
        r = np.concatenate([p[:, 0], p[:, 1], t[:, 0], t[:, 2]])
        c = np.concatenate([p[:, 1], p[:, 0], t[:, 1], t[:, 1]])
        pv = (0.5 + 0.5 * rng.random(pairs)).astype(dtype)
        vals = np.concatenate([pv, pv, (0.5 + 0.5 * rng.random(2 * triples)).astype(dtype)])
    else:
        raise KeyError(name)
    t = _graph_from_edges(n, r, c, rng, dtype, vals)
    check_preconditions(t, sorted_rows=True)
    return GraphCase(t, None)


GRAPH_CASES = ("path_random", "path_ordered", "stars", "stars_out", "small")


def _row_sums(graph, ml: CsrList, order, accumulate):
    """graph.data = the similarities (cast to `accumulate`); graph.sum(axis=1); widened to float64.  order 'numpy' is scipy's
    own (np.add.reduceat over the row), 'sequential' adds left to right."""
    graph = graph.copy()
    assert graph.has_canonical_format and np.array_equal(graph.indices, ml.cols)    # rows sorted: the list's order is the graph's
    graph.data = ml.vals.astype(accumulate)
    if order == "numpy":
        return np.asarray(graph.sum(axis=1)).squeeze(axis=1).astype(np.float64)
    weight = np.zeros(graph.shape[0], np.float64)
    for i in np.flatnonzero(np.diff(ml.row_ptr)):
        weight[i] = np.cumsum(graph.data[ml.row_ptr[i]:ml.row_ptr[i + 1]])[-1]
    return weight


def ref_group_reps(ml: CsrList, n, centroid, connection="weak", order="numpy", accumulate=np.float64, ties="first") -> np.ndarray:
    """group_similar_strings' reduction (string_grouper.py:851-904): connected_components(directed=True) over the list's
    pairs; 'first': a component's lowest index; 'centroid': graph.sum(axis=1) of the float64 similarities, then per
    component the first index of the maximum (pandas' idxmax)."""
    graph = sp.csr_matrix((np.full(len(ml.cols), 1), (rows_of(ml), ml.cols)), shape=(n, n))
    _, groups = connected_components(csgraph=graph, directed=True, connection=connection)
    if not centroid:
        weight, how = pd.Series(np.arange(n)), "first"
    else:
        weight, how = pd.Series(_row_sums(graph, ml, order, accumulate)), "idxmax"
        if ties == "last":      # the last index of the maximum: reverse, take the first, map back
            rev = pd.Series(weight.to_numpy()[::-1]).groupby(groups[::-1], sort=False).transform("idxmax").to_numpy()
            return (n - 1 - rev[::-1]).astype(np.int32)
    return weight.groupby(groups, sort=False).transform(how).to_numpy().astype(np.int32)


def mutant_reps_left_to_right(ml, n):
    return ref_group_reps(ml, n, True, order="sequential")


def mutant_reps_float32_sum(ml, n):
    return ref_group_reps(ml, n, True, accumulate=np.float32)


def mutant_reps_highest_index(ml, n):
    return ref_group_reps(ml, n, True, ties="last")


def mutant_reps_strong(ml, n, centroid):
    return ref_group_reps(ml, n, centroid, connection="strong")


# ===================================================================================================== K9: row-wise dot
class DotCase(NamedTuple):
    a: sp.csr_matrix
    b: sp.csr_matrix
    zero_rows: np.ndarray   # rows holding a common column whose product underflows to exactly 0


@functools.lru_cache(maxsize=None)
def dot_case(dtype) -> DotCase:
    """Row pairs for sg_csr_rowwise_dot, sorted rows of distinct columns.  For every number of common columns with a
    non-zero product m = 0 and BOUNDARY_RESTS + 1, six pairs:
      0, 1  values of mixed magnitude (mantissa x 2^-12 .. 2^12): the rounded sum depends on the order;
      2, 3  the same with 1 + m // 16 further common columns whose product underflows to exactly 0 -- scipy drops those, so
            they must not take a place in the summation order -- at random places, the first column among them in pair 3;
      4     the same as 0 with common columns whose product is subnormal but not 0, which scipy keeps;
      5     only subnormal products (the sum itself is subnormal).
    Every pair also has columns that only one side holds.  Then: rows without a common column, rows empty in A, in B, in both."""
    rng = np.random.default_rng(9000 + (dtype is np.float64))
    tiny, sub = (2.0 ** -80, 2.0 ** -72) if dtype is np.float32 else (2.0 ** -600, 2.0 ** -530)
    n_cols = 2000
    rows_a, rows_b, zero_rows = [], [], []

    def mixed(k):
        return (1 + rng.random(k)) * 2.0 ** rng.integers(-12, 13, k)

    def emit(common, va, vb, only_a=5, only_b=4):
        free = np.setdiff1d(np.arange(n_cols), common)
        extra = rng.choice(free, only_a + only_b, replace=False)
        ca = np.concatenate([common, extra[:only_a]])
        cb = np.concatenate([common, extra[only_a:]])
        ra = (ca, np.concatenate([va, mixed(only_a)]).astype(dtype))
        rb = (cb, np.concatenate([vb, mixed(only_b)]).astype(dtype))
        for rows, (cc, vv) in ((rows_a, ra), (rows_b, rb)):
            o = np.argsort(cc)
            rows.append((cc[o], vv[o]))

    for m in (0,) + tuple(r + 1 for r in BOUNDARY_RESTS):
        for flavour in range(6):
            z = 0 if flavour in (0, 1, 5) else 1 + m // 16
            common = np.sort(rng.choice(n_cols, m + z, replace=False))
            va, vb = mixed(m + z), mixed(m + z)
            if flavour == 5:
                va, vb = (1 + rng.random(m)) * sub, (1 + rng.random(m)) * sub
            if z:
                special = rng.choice(m + z, z, replace=False)
                if flavour == 3:
                    special[0] = 0
                    special = np.unique(special)
                scale = sub if flavour == 4 else tiny
                va[special], vb[special] = (1 + rng.random(len(special))) * scale, (1 + rng.random(len(special))) * scale
                if flavour != 4:
                    zero_rows.append(len(rows_a))
            emit(common, va, vb)
    for only_a, only_b in ((6, 9), (0, 5), (7, 0), (0, 0)):     # no common column; empty in A; in B; in both
        emit(np.zeros(0, np.int64), np.zeros(0), np.zeros(0), only_a, only_b)

    def csr(rows):
        ptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
        m = sp.csr_matrix((np.concatenate([v for _, v in rows]).astype(dtype),
                           np.concatenate([c for c, _ in rows]).astype(np.int32), ptr), shape=(len(rows), n_cols))
        assert m.has_canonical_format and (m.data != 0).all()
        return m
    return DotCase(csr(rows_a), csr(rows_b), np.array(zero_rows))


def ref_rowwise_dot(a, b) -> np.ndarray:
    """StringGrouper.dot (string_grouper.py:433-440)."""
    return np.asarray(a.multiply(b).sum(axis=1)).squeeze(axis=1)


def _common_products(a, b):
    """Per row the products over the common columns in ascending column order, zero products included."""
    out = []
    for i in range(a.shape[0]):
        ca, cb = a.indices[a.indptr[i]:a.indptr[i + 1]], b.indices[b.indptr[i]:b.indptr[i + 1]]
        _, ia, ib = np.intersect1d(ca, cb, assume_unique=True, return_indices=True)
        out.append(a.data[a.indptr[i] + ia] * b.data[b.indptr[i] + ib])
    return out


def mutant_dot_keeps_zero_products(a, b) -> np.ndarray:
    prods = _common_products(a, b)
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in prods])])
    cols = np.concatenate([np.arange(len(p), dtype=np.int32) for p in prods])
    m = sp.csr_matrix((np.concatenate(prods), cols, ptr), shape=(a.shape[0], max(1, int(np.diff(ptr).max()))))
    return np.asarray(m.sum(axis=1)).squeeze(axis=1)


def mutant_dot_left_to_right(a, b) -> np.ndarray:
    out = np.zeros(a.shape[0], a.dtype)
    for i, p in enumerate(_common_products(a, b)):
        p = p[p != 0]
        if len(p):
            out[i] = np.cumsum(p)[-1]
    return out


# ===================================================================================================== row costs
class CostCase(NamedTuple):
    a: sp.csr_matrix
    b: sp.csr_matrix


@functools.lru_cache(maxsize=None)
def cost_case(name) -> CostCase:
    """A: 700 x 300 with every fifth row empty.  B, 9 000 x 300 (above the 8 192 rows from which an index groups identical
    rows by default), rows of 2 .. 12 positive values:
      'repeats'  -- 3 000 different rows of unit length, each three times, shuffled.  Cosine-like (values >= 0, sorted rows,
                    norms <= 1), which is what the library asks of a matrix before it groups its identical rows;
      'repeats_long' -- the same rows times 3: norms above 1, so the index keeps every row although they repeat;
      'distinct' -- rows of unit length, no two alike."""
    rng = np.random.default_rng(9500 + sorted(COST_CASES).index(name))
    n_terms = 300

    def rows(n, empty_every=0):
        ptr, cols = [0], []
        for i in range(n):
            k = 0 if empty_every and i % empty_every == 0 else int(rng.integers(2, 13))
            cols.append(np.sort(rng.choice(n_terms, k, replace=False)))
            ptr.append(ptr[-1] + k)
        cols = np.concatenate(cols).astype(np.int32)
        m = sp.csr_matrix((0.1 + rng.random(len(cols)), cols, np.array(ptr, np.int32)), shape=(n, n_terms))
        norm = np.sqrt(np.asarray(m.multiply(m).sum(axis=1)).ravel())
        m.data = (m.data / np.repeat(np.where(norm > 0, norm, 1.0), np.diff(m.indptr))).astype(np.float32)
        return m
    a = rows(700, empty_every=5)
    if name.startswith("repeats"):
        b = rows(3000)[rng.permutation(np.repeat(np.arange(3000), 3))]
        if name == "repeats_long":
            b.data *= np.float32(3)
    else:
        b = rows(9000)
    b = sp.csr_matrix(b)
    b.sort_indices()
    assert b.has_canonical_format and (b.data > 0).all() and b.dtype == np.float32
    return CostCase(a, b)


COST_CASES = ("repeats", "repeats_long", "distinct")


def distinct_rows(b: sp.csr_matrix) -> sp.csr_matrix:
    """One row per group of identical rows (same columns, same values), the group's first."""
    keys = [(b.indices[b.indptr[i]:b.indptr[i + 1]].tobytes(), b.data[b.indptr[i]:b.indptr[i + 1]].tobytes())
            for i in range(b.shape[0])]
    first = sorted({k: i for i, k in reversed(list(enumerate(keys)))}.values())
    return b[first]


def ref_row_costs(a: sp.csr_matrix, index_rows: sp.csr_matrix) -> np.ndarray:
    """Intermediate products per left row: (A != 0) @ df, df[k] = index rows that hold term k."""
    df = np.asarray((index_rows != 0).sum(axis=0)).ravel().astype(np.int64)
    return np.asarray((a != 0).astype(np.int64) @ df).ravel().astype(np.int64)
