"""Constructed right-hand matrices for the index build's fill (sg_postings.hip: postings_count_lds, postings_fill_staged,
plan_build's split).  TEST INFRASTRUCTURE ONLY: host arrays, numpy / scipy, the oracle's port; no GPU and no library.

The index cannot be read back: a lost or misplaced posting shows only through a multiply.  So every matrix here is built so
that a posting DECIDES a match.  A row carries ONE group term of weight w in [0.95, 0.995], and the rest of its norm (<= 1)
on filler terms of small weight.  Two rows of one group score w_i w_j (+ at most 0.1 of filler) >= 0.9, two rows of different
groups at most 0.1 + 0.04: at 0.8 rows match if and only if each is found through the other's posting of the group term --
which can never fall into a row's suffix, the rest of the row being far too light to reach 0.8 on its own -- and a row
finds ITSELF only through its own.  The weights are distinct over all rows, so the scores inside a group are, and the top-n
cut is decided: groups of up to 80 rows are not cut at all, of a larger group (the tiny vocabularies) the heaviest rows stay.  A group's rows inside one part of a tile are one (term, part) CELL of the build.

tests/test_fill_edge_cases_cpu.py shows without a GPU that removing one posting of a checked cell changes the port's result;
tests/test_postings_fill_edges_gpu.py builds the index over these matrices under every split and staging mode and expects the
port's bits.  Every builder is cached: the arrays are shared and must not be written to."""
import functools
from typing import NamedTuple, Tuple

import numpy as np
import scipy.sparse as sp

TOP_N, THRESHOLD = 80, 0.8          # top 80: no cut inside the sized cells (<= 70 rows), so EVERY posting of theirs decides
TILE = 4096
SPLITS = (1, 2, 3, 4, 5, 6, 7, 8)            # every number of parts plan_build may choose for a 4096-row tile (parts >= 512 rows)
FREQUENT_WEIGHT = 0.2


def part_begin(part: int, split: int, tile: int = TILE) -> int:
    """where part `part` of `split` begins inside a tile (sg_postings.hip, part_begin)"""
    return tile if part >= split else (part * tile // split) & ~63


class Case(NamedTuple):
    name: str
    B: sp.csr_matrix                 # the right-hand matrix (and the left one of the self-join)
    checked: Tuple[Tuple[int, Tuple[int, ...]], ...]    # (group term, its rows): the cells whose every posting decides a match
    left_rows: slice                 # the left rows of the one-sided product
    collapse_off: bool               # rows repeat: SG_COLLAPSE=0 keeps every row a row of the index


def _build(name, n_rows, n_terms, groups, lengths=None, frequent=False, seed=1, dtype=np.float32, collapse_off=False) -> Case:
    """`groups`: lists of rows; every group gets a term of its own, spread over [0, n_terms) with the first and the last term
    taken; rows in no group are groups of one.  `lengths`: row -> entries (default 2: the group term and one filler term; 0: an
    empty row; 1: the group term alone, at weight w < 1).  `frequent`: one more term, of weight 0.2, in EVERY row."""
    rng = np.random.default_rng(seed)
    lengths = dict(lengths or {})
    in_group = set(r for g in groups for r in g)
    groups = [list(g) for g in groups] + [[r] for r in range(n_rows) if r not in in_group]
    n_groups = len(groups)
    room = n_terms - (1 if frequent else 0)
    if n_groups > room:              # fewer terms than groups: the groups share them round robin (vocabularies of 1, 2, 63 ...)
        merged = [[] for _ in range(room)]
        for i, g in enumerate(groups):
            merged[i % room].extend(g)
        groups, n_groups = merged, room
    group_terms = np.unique(np.round(np.linspace(0, room - 1, n_groups)).astype(np.int64))
    assert len(group_terms) == n_groups and group_terms[0] == 0 and group_terms[-1] == room - 1
    filler = np.setdiff1d(np.arange(room), group_terms)
    freq_term = n_terms - 1 if frequent else -1
    weights = 0.95 + (0.025 if frequent else 0.045) * (rng.permutation(n_rows) + 0.5) / n_rows     # distinct over all rows
    # (with the frequent term's 0.04 of squared norm beside it the group term stays below 0.975)
    term_of = np.empty(n_rows, np.int64)
    for t, g in zip(group_terms, groups):
        term_of[g] = t
    cols, vals, indptr = [], [], [0]
    for r in range(n_rows):
        m = lengths.get(r, 2 if len(filler) else 1)
        if m > 0:
            c, v = [term_of[r]], [weights[r]]
            rest = 1.0 - weights[r] ** 2
            if frequent:
                c.append(freq_term)
                v.append(FREQUENT_WEIGHT)
                rest -= FREQUENT_WEIGHT ** 2
            n_fill = m - len(c)
            if n_fill > 0:
                at = (r * 7 + np.arange(n_fill)) % len(filler)
                assert len(np.unique(at)) == n_fill, "not enough filler terms for a row of this length"
                c.extend(filler[at])
                v.extend([np.sqrt(rest * 0.98 / n_fill)] * n_fill)             # (0.98: the norm stays below 1 in either type)
            order = np.argsort(c)
            cols.extend(np.asarray(c)[order])
            vals.extend(np.asarray(v)[order])
        indptr.append(len(cols))
    B = sp.csr_matrix((np.asarray(vals, dtype), np.asarray(cols, np.int32), np.asarray(indptr, np.int64)), shape=(n_rows, n_terms))
    B.has_sorted_indices = True
    checked = tuple((int(t), tuple(int(r) for r in g if lengths.get(r, 1) > 0)) for t, g in zip(group_terms, groups)
                    if len(g) > 1 or n_groups <= 70)
    return Case(name, B, checked, slice(0, min(n_rows, 1500)), collapse_off)


def _cells_in_part_0():
    """groups of 63, 64 and 65 consecutive rows below row 512 -- inside part 0 of the first tile under every split -- and one
    whose rows lie 300 apart: a cell of one or two entries in every part it reaches"""
    return [range(0, 63), range(63, 127), range(127, 192), range(200, 3000, 300)]


ROW_LENGTHS = {300: 0, 301: 1, 302: 16, 303: 17, 304: 64, 2999: 64, 2998: 0}


@functools.lru_cache(maxsize=None)
def case(name: str, dtype=np.float32) -> Case:
    s5 = [part_begin(p, 5) for p in range(6)]          # 0, 768, 1600, 2432, 3264, 4096
    if name == "one_tile":          # 3 000 rows, ~18 000 terms; cells of 1, 63, 64, 65; rows of 0, 1, 16, 17 and 64 entries
        return _build(name, 3000, 18001, _cells_in_part_0(), ROW_LENGTHS, dtype=dtype)
    if name == "two_tiles_and_a_row":   # 8 193 rows: the last tile holds one row, every other part of it is empty
        return _build(name, 8193, 18000, _cells_in_part_0() + [range(4000, 4070), [8192, 250, 4300]], ROW_LENGTHS, dtype=dtype)
    if name == "ends_on_a_part":    # the second tile ends exactly where part 1 of 5 begins: parts 1 .. 4 are empty
        return _build(name, TILE + s5[1], 9001, _cells_in_part_0() + [range(TILE, TILE + 65)], dtype=dtype)
    if name == "part_of_one_row":   # ... one row further: part 1 of 5 holds one row
        return _build(name, TILE + s5[1] + 1, 9001, _cells_in_part_0() + [[TILE + s5[1], TILE + 3, 250]], dtype=dtype)
    if name == "frequent_everywhere":   # a term in every row: the rows' frequent-part norms are not trivial
        return _build(name, 3000, 5000, _cells_in_part_0(), ROW_LENGTHS, frequent=True, dtype=dtype)
    if name == "rows_of_60":        # a part is several chunks: 60 entries a row
        return _build(name, 3000, 3001, _cells_in_part_0(), {r: 60 for r in range(3000)}, dtype=dtype)
    if name.startswith("terms_"):   # tiny vocabularies: 1, 2, 63, 64, 65 terms -- a cell holds every row of a part (or a 63rd)
        return _build(name, 3000, int(name[6:]), [], dtype=dtype, collapse_off=True)
    raise KeyError(name)


CASES = ("one_tile", "two_tiles_and_a_row", "ends_on_a_part", "part_of_one_row", "frequent_everywhere", "rows_of_60",
         "terms_1", "terms_2", "terms_63", "terms_64", "terms_65")


def postings_of_chunk(c: Case, row0: int, row1: int) -> int:
    return int(c.B.indptr[row1] - c.B.indptr[row0])


_PORT = {}


def port(name: str, dtype, one_sided: bool):
    """the port's answer, computed once and shared: do not write to it"""
    from oracle import port as P
    key = (name, np.dtype(dtype).name, one_sided)
    if key not in _PORT:
        c = case(name, dtype)
        left = c.B[c.left_rows] if one_sided else c.B
        _PORT[key] = P.sp_matmul_topn_port(left, c.B.T, TOP_N, THRESHOLD, True, 8)
    return _PORT[key]


def without_posting(B: sp.csr_matrix, row: int, term: int) -> sp.csr_matrix:
    """B with the entry (row, term) taken out: what an index that lost this posting stands for"""
    lo, hi = B.indptr[row], B.indptr[row + 1]
    at = lo + int(np.flatnonzero(B.indices[lo:hi] == term)[0])
    indptr = B.indptr.copy()
    indptr[row + 1:] -= 1
    out = sp.csr_matrix((np.delete(B.data, at), np.delete(B.indices, at), indptr), shape=B.shape)
    out.has_sorted_indices = True
    return out
