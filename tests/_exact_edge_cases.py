"""Constructed inputs for the EXACT multiply (K4: string_grouper_amd/csrc/sg_spgemm_topn.hip, sg_k4_device.h) that sit on the
edges of its loops, a census that counts what the kernel will meet on them, and the multiply restated in plain numpy -- right,
and with one thing wrong at a time.  TEST INFRASTRUCTURE ONLY: host arrays, numpy / scipy; no GPU and no library.
tests/test_exact_edge_cases_cpu.py proves without a GPU that the inputs reach every edge and that every wrong reference
changes the answer on them; tests/test_exact_edges_gpu.py runs the kernel on them and expects the port's bits.

The design is written in POSITION order -- position p is column p % tile_cols of tile p // tile_cols of the index -- with
n = 2 * tile_cols + 104 right-hand rows: three tiles, the last one partial, and more rows than the 2 * tile_cols below which
the library does not permute.  The caller's matrix is the design permuted by the library's rule (sg_postings.hip,
build_permuted; restated in ``permutation``): row j of the caller lies at position pos_of[j] = j * M % n.  Results name ROWS.

Families (``build(family, dtype, tile_cols, permute)``), the first five one-sided products of the exact kernel:

  lists    posting segments of every length at which segment_batch / stream_rest change their path: 1 2 63 64 65 127 128 129,
           319 320 321, 575 576 577, 831 832 833, 1087 1088 1089, 1343 1344 1345, tile_cols - 1 and tile_cols (a term held by
           every column of a tile), in tiles 0 and 1; 1 2 63 64 65 103 104 in the partial tile.  One left row per term, one row
           over all the long terms.  top_n = n_right observes every accumulator.
           LEFT OUT BY CONSTRUCTION: a length that does not fit the tile -- 1087 .. 1345 at tile_cols = 1024, so the wrong
           reference "entries past 1088 lost" has nothing to bite on there (``expected`` / ``flaws_of`` leave both out at 1024).
  batches  left rows whose chunks of 64 entries hold 0 1 7 8 9 15 16 17 63 64 non-empty segments in tile 0, 1 or the partial
           tile; rows of 65 71 72 73 127 128 129 192 193 entries whose second and third chunks hold 1 7 8 9; chunks where only
           lane 0, only lane 63, or lanes 0 and 63 hold a segment; a row with nothing in the middle tile; rows with segments
           only in the partial tile; the empty row; a row whose terms nobody holds; term 0 and term V - 1; and rows of inexact
           values over three hub columns whose sum depends on the order of the additions, one of them stored in descending
           column order.
  sweep    hits at tile positions 0, 1, VEC - 1, VEC, 64 VEC - 1, 64 VEC, 256 VEC - 1, 256 VEC, tile_cols - 1, the first column
           of the next tile and the last column of the partial tile; all VEC elements of a vector; all 64 lanes of a stripe in
           one ballot; more than 64 hits a tile with scores rising and falling with the column; a score exactly at the
           threshold and its upper neighbour at every corner position.
           LEFT OUT BY CONSTRUCTION: position 256 VEC inside a tile where 256 VEC == tile_cols (float32 at 1024: it IS the
           first column of the next tile, which is built).
  state    the list between launches and passes: rows whose count after the first tile is 0 1 63 64 and whose later tiles
           bring better, worse and equal scores; rows of exactly 63 64 65 127 128 129 matches; one row of 140 matches with
           blocks of equal scores over ranks 60-70 and 124-132 whose members lie in all three tiles.
  waves    4 x CUs left rows (SG_WAVES_PER_CU=1: one wave a CU, many rows in turn): a row that touches every column of every
           tile alternates with probes that touch one tile, two tiles with the middle one left out, or nothing.

  selfjoin one cosine-like matrix on both sides (values >= 0, columns ascending, squared norms <= 1 from dyadic values), for the
           exact kernel's self-join launch (SELF: a row scores the columns <= itself over the tiles up to its own, keeps those and
           hands the mirrored pairs to the pair list in chunks of 256): a club of 300 rows that share one term -- values 1, 1/2,
           1/4 -- at positions 0, tile_cols - 1, tile_cols, n - 1 and spread over the three tiles, whose m-th member has exactly m
           mirrored pairs (127 128 129 and 255 256 257 among them, the latter with all partners but a few in earlier tiles), and hubs
           of identical rows of 4 x 0.5, 64 x 0.125 and 256 x 0.0625; every other row holds a term of its own.
           LEFT OUT BY CONSTRUCTION: tile_cols = 1024 -- the self-join form needs an index the pruned multiply's gate accepts,
           tiles of 2048 columns and up (sg_pruned_supports_tile); SELF_TILES leaves it out.

Every builder is cached: the arrays it returns are shared and must not be written to."""
import functools
import math
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp

DTYPES = (np.float32, np.float64)
TILES = (1024, 2048, 4096)
FAMILIES = ("lists", "batches", "sweep", "state", "waves")      # one-sided; and "selfjoin", at SELF_TILES
SELF_TILES = (2048, 4096)
MIRRORED_PAIRS = (127, 128, 129, 255, 256, 257)
PAIR_CHUNK = 256           # SG_PAIR_CHUNK
LANES = 64                 # SG_TOPN_LANES: entries of the register list, lanes of a wave, entries of a chunk of a left row
NB = 8                     # segments a batch (launch_spgemm: spgemm_topn_kernel<T, TILE_LOG2, 8>)
TILE_GROUPS = (1, 2, 0)    # SG_TILE_GROUP: a launch a tile, two tiles then one, one launch (0: the library's choice -- all three)

SEGMENT_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 319, 320, 321, 575, 576, 577, 831, 832, 833, 1087, 1088, 1089, 1343, 1344, 1345)
PARTIAL = 104              # columns of the last tile
PARTIAL_LENGTHS = (1, 2, 63, 64, 65, PARTIAL - 1, PARTIAL)
SEGMENT_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64)
# (entries, non-empty segments per chunk of 64) of the long left rows: the second and third chunks hold 1, 7, 8 and 9
LONG_ROWS = ((65, (0, 1)), (71, (9, 7)), (72, (0, 8)), (73, (8, 9)), (127, (0, 7)), (128, (17, 8)), (129, (0, 9, 1)),
             (192, (1, 1, 7)), (193, (0, 8, 9, 1)), (192, (0, 9, 8)), (193, (7, 7, 1, 1)))
FIRST_GROUP_COUNTS = (0, 1, 63, 64)
MATCH_COUNTS = (63, 64, 65, 127, 128, 129)
TIE_BLOCKS = ((60, 70), (124, 132))


def vec(dtype) -> int:
    """accumulators per 16-byte LDS access of the sweep"""
    return 16 // np.dtype(dtype).itemsize


def permutation(n: int):
    """(pos_of, orig_of) of the library's row permutation of n rows (sg_postings.hip: build_permuted)."""
    m = int(0.6180339887498949 * n) | 1
    while math.gcd(m, n) != 1:
        m += 2
    m %= n
    j = np.arange(n, dtype=np.int64)
    pos_of = j * m % n
    orig_of = np.empty(n, np.int64)
    orig_of[pos_of] = j
    return pos_of, orig_of


class Lists(NamedTuple):
    """The posting lists of a right-hand matrix in position order: term k = entries ptr[k] .. ptr[k + 1], positions ascending."""
    n: int
    tile: int
    ptr: np.ndarray
    pos: np.ndarray
    val: np.ndarray
    orig_of: np.ndarray       # position -> row of the caller's matrix


def lists_of(B: sp.csr_matrix, tile_cols: int, pos_of=None) -> Lists:
    n = B.shape[0]
    orig_of = np.arange(n, dtype=np.int64)
    if pos_of is not None:
        orig_of = np.empty(n, np.int64)
        orig_of[np.asarray(pos_of, np.int64)] = np.arange(n, dtype=np.int64)
    c = sp.csc_matrix(sp.csr_matrix(B)[orig_of])
    c.sort_indices()
    return Lists(n, int(tile_cols), c.indptr.astype(np.int64), c.indices.astype(np.int64), c.data.copy(), orig_of)


class Case(NamedTuple):
    family: str
    dtype: type
    tile_cols: int
    permute: bool
    n: int
    n_terms: int
    B: sp.csr_matrix          # the caller's right-hand matrix (n x V): the design permuted (or the design itself)
    pos_of: np.ndarray        # None: not permuted
    orig_of: np.ndarray       # position -> caller's row (the identity when not permuted)
    lists: Lists
    A: sp.csr_matrix          # the left matrix
    row_names: tuple          # what each left row is there for
    edges: dict               # edge -> the left rows / terms that carry it (as built; the census counts independently)
    schedule: tuple           # ((top_n, thr, sort), ...)
    probe: np.ndarray = None  # selfjoin (A is B): the rows the numpy reference is run on -- every club and hub member, a few others


# ------------------------------------------------------------------------------------------------------------ the builder
class _Design:
    def __init__(self, dtype, tile):
        self.dtype, self.tile, self.n = dtype, tile, 2 * tile + PARTIAL
        self.p, self.k, self.v = [], [], []
        self.n_terms = 0
        self.rows, self.names, self.edges = [], [], {}

    def term(self, positions=(), values=1.0):
        k = self.n_terms
        self.n_terms += 1
        self.hold(k, positions, values)
        return k

    def hold(self, k, positions, values=1.0):
        positions = np.asarray(positions, np.int64).ravel()
        assert len(set(positions.tolist())) == len(positions) and (len(positions) == 0 or (0 <= positions.min() and positions.max() < self.n))
        self.p += positions.tolist()
        self.k += [k] * len(positions)
        self.v += np.broadcast_to(np.asarray(values, np.float64), positions.shape).tolist()

    def row(self, name, cols, vals=1.0, edge=None):
        cols = np.asarray(cols, np.int64).ravel()
        self.rows.append((cols, np.broadcast_to(np.asarray(vals, np.float64), cols.shape).copy()))
        self.names.append(name)
        if edge:
            self.edges.setdefault(edge, []).append(len(self.rows) - 1)
        return len(self.rows) - 1

    def right(self):
        m = sp.csr_matrix((np.asarray(self.v, self.dtype), (np.asarray(self.p, np.int64), np.asarray(self.k, np.int64))),
                          shape=(self.n, self.n_terms))
        m.sort_indices()
        assert m.nnz == len(self.p), "a position holds a term twice"
        return m

    def left(self):
        indptr = np.zeros(len(self.rows) + 1, np.int64)
        np.cumsum([len(c) for c, _ in self.rows], out=indptr[1:])
        cols = np.concatenate([c for c, _ in self.rows] + [np.zeros(0, np.int64)])
        vals = np.concatenate([v for _, v in self.rows] + [np.zeros(0)])
        m = sp.csr_matrix((vals.astype(self.dtype), cols.astype(np.int32), indptr), shape=(len(self.rows), self.n_terms))
        # the rows are in STORAGE order as built (one is descending on purpose): nobody may sort them
        m.has_sorted_indices = True
        return m


def _spread(c, width=LANES):
    """c of the `width` lanes of a chunk, spread over it, the last lane among them from two up"""
    if c == 0:
        return []
    if c == 1:
        return [0]
    return sorted({(i * (width - 1)) // (c - 1) for i in range(c)})


def _lists_family(d: _Design):
    tile, n = d.tile, d.n
    single, long_terms = [], []
    lengths = [L for L in SEGMENT_LENGTHS + (tile - 1, tile) if L <= tile]
    for i, L in enumerate(lengths):
        for t in (i % 2, 1 - i % 2) if L in (64, 320, 576, tile) else (i % 2,):
            start = t * tile + (37 * i) % (tile - L + 1)
            pos = np.arange(start, start + L)
            k = d.term(pos, (1 + pos * 5 % 16) / 32.0)
            single.append((k, f"segment of {L} in tile {t}"))
            if L >= 64:
                long_terms.append(k)
    for i, L in enumerate(PARTIAL_LENGTHS):
        start = 2 * tile + (11 * i) % (PARTIAL - L + 1)
        pos = np.arange(start, start + L)
        single.append((d.term(pos, (1 + pos * 3 % 16) / 32.0), f"segment of {L} in the partial tile"))
    for k, name in single:
        d.row(name, [k], 1.0, edge="segment lengths")
    d.row("every long term", long_terms, 0.5, edge="segment lengths")
    # (sort=False keeps a row in shared memory: 2048 entries fit at both value types, the whole row of 8296 does not)
    return ((n, 0.0, True), (LANES, 0.0, True), (2048, 0.0, False))


_X, _Y, _Z, _N, _H = range(5)      # banks of terms: held in tile 0, tile 1, the partial tile, by nobody, by three hub columns
_BANKS = 5
_BANK_M = 193                      # members of a bank = entries of the longest left row


def _batches_family(d: _Design):
    tile, dtype = d.tile, d.dtype
    rng = np.random.default_rng(11)
    hubs = np.array([7, tile + 12, 2 * tile + 13])
    for m in range(_BANK_M):                      # term id = 5 m + bank: a left row picks a bank per entry, ids ascending
        assert d.term([3 + 5 * m]) == _BANKS * m + _X
        d.term([tile + 1 + 5 * m])
        d.term([2 * tile + m % PARTIAL])
        d.term([])
        d.term(hubs, rng.random(3) + 0.5)
    a_of = lambda e: (1 + e % LANES) / 64.0       # distinct within a chunk

    def row(name, banks, edge):                   # entry e: term (e, banks[e])
        e = np.arange(len(banks))
        return d.row(name, _BANKS * e + np.asarray(banks, np.int64), a_of(e), edge)

    for c in SEGMENT_COUNTS:
        for bank, where in ((_X, "tile 0"), (_Y, "tile 1"), (_Z, "the partial tile")):
            banks = np.full(LANES, _N)
            banks[_spread(c)] = bank
            row(f"{c} segments in {where}", banks, "segments per chunk" if c else "terms nobody holds")
    for c in (1, 9):                              # tiles 0 and 2 touched, the middle one not
        banks = np.full(LANES, _N)
        lanes = _spread(2 * c)
        banks[lanes[0::2]], banks[lanes[1::2]] = _X, _Z
        row(f"{c} segments in tile 0 and {c} in the partial tile, none in the middle", banks, "middle tile untouched")
    for lanes, what in (([0], "lane 0"), ([63], "lane 63"), ([0, 63], "lanes 0 and 63")):
        for chunk in (0, 1):
            banks = np.full(LANES * (chunk + 1), _N)
            banks[[LANES * chunk + l for l in lanes]] = _Y if chunk else _X
            row(f"only {what} of chunk {chunk}", banks, "ballot masks")
    for i, (length, counts) in enumerate(LONG_ROWS):
        banks = np.full(length, _N)
        for ch, c in enumerate(counts):
            width = min(LANES, length - LANES * ch)
            lanes = _spread(c, width) if ch == 0 else list(range(width - c, width))     # later chunks: the LAST c entries
            banks[[LANES * ch + l for l in lanes]] = (_X, _Y, _Z)[(i + ch) % 3]
        row(f"{length} entries, segments per chunk {counts}", banks, "long rows")
    d.row("the empty row", [], 1.0, "empty row")
    # inexact values over the hub columns: every accumulator receives all the row's products, the order decides the bits
    for length in (9, 72, _BANK_M):
        e = np.arange(length)
        d.row(f"{length} inexact products a hub column", _BANKS * e + _H, rng.random(length) + 0.25, "order of the sum")
    e = np.arange(72)[::-1]
    d.row("72 inexact products a hub column, stored in descending column order", _BANKS * e + _H, rng.random(72) + 0.25, "order of the sum")
    return ((256, 0.0, True), (LANES, 0.0, True), (8, 0.0, False))


def sweep_positions(dtype, tile):
    """the corner positions of the sweep that exist at this tile size, as positions of the index"""
    v = vec(dtype)
    inside = sorted({q for q in (0, 1, v - 1, v, 64 * v - 1, 64 * v, 256 * v - 1, 256 * v, tile - 1) if q < tile})
    out = [t * tile + q for t in (0, 1) for q in inside] + [2 * tile + q for q in inside if q < PARTIAL] + [2 * tile + PARTIAL - 1]
    return sorted(set(out))


def _sweep_family(d: _Design):
    tile, dtype = d.tile, d.dtype
    v = vec(dtype)
    corners = sweep_positions(dtype, tile)
    for p in corners:
        d.row(f"one hit at position {p} (tile {p // tile} column {p % tile})", [d.term([p])], 0.75, "corner positions")
    at = d.term(corners, 0.5)
    d.row("every corner exactly at 0.5", [at], 1.0, "at the threshold")
    d.row("every corner one ulp above 0.5", [at], float(np.nextafter(dtype(1), dtype(2))), "above the threshold")
    for t in (0, 1, 2):
        x = 10 + t
        d.row(f"all {v} elements of vector {x} of tile {t}", [d.term(t * tile + x * v + np.arange(v), (1 + np.arange(v)) / 8.0)], 1.0, "whole vector")
    for t, stripe in ((0, 0), (1, 1), (1, 3)):
        pos = t * tile + (stripe * LANES + np.arange(LANES)) * v + (v - 1)
        d.row(f"all 64 lanes of stripe {stripe} of tile {t}", [d.term(pos, (1 + np.arange(LANES) * 5 % 64) / 64.0)], 1.0, "whole stripe")
    i = np.arange(100)
    pos = np.concatenate([5 + 7 * i, tile + 6 + 9 * i])
    d.row("200 hits, scores rising with the column", [d.term(pos, (1 + np.arange(200)) / 256.0)], 1.0, "rising")
    d.row("200 hits, scores falling with the column", [d.term(pos, (200 - np.arange(200)) / 256.0)], 1.0, "falling")
    return ((256, 0.0, True), (LANES, 0.0, True), (LANES, 0.5, True), (LANES, 0.5, False))


def _state_family(d: _Design):
    tile, n = d.tile, d.n
    for k0 in FIRST_GROUP_COUNTS:
        for later, b in (("better", 0.75), ("worse", 0.25), ("equal", 0.5)):
            k = d.term(2 + 3 * np.arange(k0), 0.5)
            d.hold(k, tile + 4 + 5 * np.arange(10), b)
            d.hold(k, 2 * tile + 1 + 7 * np.arange(5), b)
            d.row(f"{k0} matches in the first tile, {later} ones later", [k], 1.0, "count after the first group")
    for c in MATCH_COUNTS:
        c0 = c1 = c // 3
        c2 = c - c0 - c1
        pos = np.concatenate([9 + 11 * np.arange(c0), tile + 3 + 13 * np.arange(c1), 2 * tile + 2 * np.arange(c2)])
        d.row(f"exactly {c} matches", [d.term(pos, (1 + np.arange(c) * 7 % 8) / 16.0)], 1.0, "match counts")
    r = np.arange(140)
    score = np.where(r < 60, (256 - r) / 256.0, np.where(r <= 70, 0.5, np.where(r < 124, (100 - (r - 71)) / 256.0,
                     np.where(r <= 132, 0.125, (20 - (r - 133)) / 256.0))))
    pos = (r % 3) * tile + (r * 97) % PARTIAL
    d.row("140 matches, equal scores over ranks 60-70 and 124-132", [d.term(pos, score)], 1.0, "tie blocks")
    return tuple((top_n, 0.0, True) for top_n in (64, 65, 127, 128, 129, 192, n)) + ((65, 0.0, False),)


def _waves_family(d: _Design, n_cu: int):
    tile, n = d.tile, d.n
    full = d.term(np.arange(n), 0.25)
    p0, p1, p2, nobody = d.term([5]), d.term([tile + 6]), d.term([2 * tile + 7]), d.term([])
    probes = (("the empty row", []), ("one hit in tile 0", [p0]), ("one hit in the partial tile", [p2]), ("a term nobody holds", [nobody]),
              ("tiles 0 and 2, the middle one untouched", [p0, p2]), ("one hit in tile 1", [p1]))
    for i in range(2 * n_cu):
        d.row("every column of every tile", [full], 1.0, "full rows")
        name, cols = probes[i % len(probes)]
        d.row(name, cols, 1.0, "probes")
    return ((LANES, 0.0, True), (8, 0.0, False))


def _selfjoin_family(d: _Design):
    tile, n = d.tile, d.n
    i = np.arange(120)
    club = np.concatenate([[0, tile - 1, tile, n - 1], 1 + 13 * i, tile + 3 + 11 * i, 2 * tile + 1 + np.arange(56)])
    club.sort()
    d.term(club, np.array([1.0, 0.5, 0.25, 0.5])[np.arange(len(club)) % 4])
    names = {int(p): f"club member {m}: {m} mirrored pairs" for m, p in enumerate(club)}
    hubs = ((4, 0.5, 5 + 13 * np.arange(15), tile + 7 + 11 * np.arange(15), 2 * tile + 60 + np.arange(10)),
            (64, 0.125, 9 + 13 * np.arange(8), tile + 9 + 11 * np.arange(8), 2 * tile + 75 + np.arange(4)),
            (256, 0.0625, 11 + 13 * np.arange(4), tile + 10 + 11 * np.arange(4), 2 * tile + 90 + np.arange(2)))
    for width, value, *where in hubs:
        pos = np.concatenate(where)
        for _ in range(width):
            d.term(pos, value)
        names.update({int(p): f"hub of {len(pos)} identical rows of {width} x {value}" for p in pos})
    assert len(names) == 300 + 40 + 20 + 10
    for p in range(n):
        if p not in names:
            d.term([p], 1.0)
    d.names = [names.get(p, "a row with a term of its own") for p in range(n)]
    return ((1, 0.0, True), (LANES, 0.0, True), (LANES + 1, 0.0, True), (2 * LANES, 0.0, True), (LANES, 0.25, True), (2 * LANES, 0.0, False))


@functools.lru_cache(maxsize=None)
def build(family: str, dtype, tile_cols: int, permute: bool, n_cu: int = 4) -> Case:
    """The right-hand matrix as the caller holds it, the left matrix and the table of which left rows carry which edge.
    n_cu: the waves family has 4 * n_cu left rows."""
    d = _Design(dtype, tile_cols)
    if family == "waves":
        schedule = _waves_family(d, n_cu)
    elif family == "selfjoin":
        assert tile_cols in SELF_TILES
        schedule = _selfjoin_family(d)
    else:
        schedule = {"lists": _lists_family, "batches": _batches_family, "sweep": _sweep_family, "state": _state_family}[family](d)
    design = d.right()
    n = d.n
    pos_of, orig_of = (permutation(n) if permute else (None, np.arange(n, dtype=np.int64)))
    B = design if not permute else sp.csr_matrix(design[pos_of])      # caller's row j lies at position pos_of[j]
    B.sort_indices()
    lists = lists_of(B, tile_cols, pos_of)
    assert np.array_equal(lists.orig_of, orig_of)
    if family == "selfjoin":      # one matrix on both sides; the rows are named by position in the design
        names = [d.names[p] for p in (pos_of if permute else range(n))]
        member = np.flatnonzero([nm != "a row with a term of its own" for nm in names])
        other = np.flatnonzero([nm == "a row with a term of its own" for nm in names])
        probe = np.sort(np.concatenate([member, other[:5], other[-5:], other[len(other) // 2:len(other) // 2 + 5]]))
        assert B.has_sorted_indices and (B.data > 0).all() and np.asarray(B.multiply(B).sum(axis=1)).max() <= 1.0
        return Case(family, dtype, tile_cols, permute, n, d.n_terms, B, pos_of, orig_of, lists, B, tuple(names), {}, schedule, probe)
    return Case(family, dtype, tile_cols, permute, n, d.n_terms, B, pos_of, orig_of, lists, d.left(), tuple(d.names), dict(d.edges), schedule)


# ------------------------------------------------------------------------------------------------------------ the reference
# flaw -> (the family whose cases it must change, what is wrong)
FLAWS = {
    "segment-multiple-of-64-loses-an-entry": ("lists", "the last entry of every segment whose length is a multiple of 64 is lost"),
    "second-register-set-lost": ("lists", "entries 320.. of a segment are lost unless it is longer than 576"),
    "stream-leaves-after-two-trips": ("lists", "entries past 1088 of a segment are lost"),
    "partial-batch-lost": ("batches", "the segments behind the last full batch of 8 of a chunk are lost (the partial batch does not run)"),
    "first-chunk-only": ("batches", "entries 64.. of a left row are lost"),
    "touched-from-first-chunk": ("batches", "a tile is swept only if the row's FIRST chunk has a segment in it"),
    "descending-sum": ("batches", "the products of a row are added in descending storage order"),
    "fused-multiply-add": ("batches", "product and sum rounded once (float32 only; emulated in float64)"),
    "last-vector-unswept": ("sweep", "the last 16 bytes of a tile are not swept"),
    "last-element-ignored": ("sweep", "element VEC - 1 of every vector is ignored"),
    "first-column-ignored": ("sweep", "the first column of every tile is ignored"),
    "greater-or-equal": ("sweep", ">= for > at the threshold"),
    "restart-empty": ("state", "the list restarts empty at every tile group"),
    "last-restored-lost": ("state", "the last entry restored at a tile group is lost"),
    "floor-by-score": ("state", "a pass takes only scores BELOW its floor: the ties of rank 64 are lost"),
    "floor-inclusive": ("state", "a pass takes its floor entry again: entry 64 comes back as 65"),
    "ties-by-higher-column": ("state", "equal scores in descending column order"),
    "ties-by-position": ("state", "equal scores in POSITION order, not row order"),
    "diagonal-dropped": ("selfjoin", "a row does not keep the pair with itself"),
    "earlier-tile-pair-lost": ("selfjoin", "a pair whose partner lies in an earlier tile is lost, for both rows"),
    "mirror-257-lost": ("selfjoin", "the 257th mirrored pair a row hands over is lost: its partner never receives the row"),
    "stale-accumulators": ("waves", "the sweep does not re-zero: a row starts from what the rows before it left"),
}


def flaws_of(family: str, dtype, tile_cols: int):
    """The wrong references a family's cases must catch at this dtype and tile size."""
    out = [f for f, (fam, _) in FLAWS.items() if fam == family]
    if tile_cols < 2048:
        out = [f for f in out if f != "stream-leaves-after-two-trips"]       # no segment beyond 1024 entries fits the tile
    if dtype != np.float32:
        out = [f for f in out if f != "fused-multiply-add"]
    return out


def _segment_keep(L: int, flaw):
    """which of the L entries of a segment are applied"""
    keep = np.ones(L, bool)
    if flaw == "segment-multiple-of-64-loses-an-entry" and L % 64 == 0:
        keep[-1] = False
    elif flaw == "second-register-set-lost" and L <= 576:
        keep[320:] = False
    elif flaw == "stream-leaves-after-two-trips":
        keep[1088:] = False
    return keep


_SEGMENT_FLAWS = ("segment-multiple-of-64-loses-an-entry", "second-register-set-lost", "stream-leaves-after-two-trips", "partial-batch-lost",
                  "touched-from-first-chunk")


_ACCUMULATOR_FLAWS = _SEGMENT_FLAWS + ("first-chunk-only", "descending-sum", "fused-multiply-add", "stale-accumulators")


def accumulate(cols, vals, L: Lists, dtype, flaw=None, acc=None):
    """One left row: (accumulators by POSITION, which tiles are swept).  Term by term in storage order,
    acc[p] = acc[p] + a * b with the product and the sum rounded on their own."""
    n, tile = L.n, L.tile
    n_tiles = -(-n // tile)
    if acc is None:
        acc = np.zeros(n, dtype)
    touched = np.zeros(n_tiles, bool)
    entries = list(zip(cols.tolist(), vals))
    if flaw == "first-chunk-only":
        entries = entries[:LANES]
    order = range(len(entries))
    if flaw == "descending-sum":
        order = reversed(order)
    bounds = np.arange(n_tiles + 1) * tile
    cuts = [np.searchsorted(L.pos[L.ptr[k]:L.ptr[k + 1]], bounds) for k, _ in entries]
    nonempty_all = np.array([np.diff(c) > 0 for c in cuts], bool).reshape(len(entries), n_tiles)
    for e in order:
        k, a = entries[e]
        lo, hi = L.ptr[k], L.ptr[k + 1]
        if hi == lo:
            continue
        ps, bs = L.pos[lo:hi], L.val[lo:hi].astype(dtype)
        cut, nonempty = cuts[e], nonempty_all[e]
        if flaw in _SEGMENT_FLAWS:
            keep = np.ones(len(ps), bool)
            c0 = e - e % LANES
            for t in np.flatnonzero(nonempty):
                if flaw == "partial-batch-lost":       # the non-empty segments of the chunk in this tile, in storage order
                    total = int(nonempty_all[c0:c0 + LANES, t].sum())
                    rank = int(nonempty_all[c0:e, t].sum())
                    if rank >= total - total % NB:
                        keep[cut[t]:cut[t + 1]] = False
                elif flaw == "touched-from-first-chunk":
                    touched[t] |= e < LANES
                else:
                    keep[cut[t]:cut[t + 1]] = _segment_keep(cut[t + 1] - cut[t], flaw)
            ps, bs = ps[keep], bs[keep]
        if flaw != "touched-from-first-chunk":
            touched |= nonempty
        if flaw == "fused-multiply-add":
            acc[ps] = (acc[ps].astype(np.float64) + np.float64(a) * bs.astype(np.float64)).astype(dtype)
        else:
            acc[ps] = acc[ps] + dtype(a) * bs
    return acc, touched


def _ranked(s, j, p, flaw):
    """order of the hits: score descending, then ROW ascending"""
    key = -j if flaw == "ties-by-higher-column" else (p if flaw == "ties-by-position" else j)
    return np.lexsort((key, -s.astype(np.float64)))


def select(acc, touched, L: Lists, top_n: int, thr, flaw=None, group: int = 0, trace=None, veto=None):
    """The row's result (rows named, scores) from its accumulators: > thr, score descending then row ascending, cut at top_n.
    With a flaw of the state between launches -- or with ``trace`` (a list that receives (pass, group, count) after every
    launch) -- the list is carried through the tile groups and passes as the kernel carries it."""
    tile, dtype = L.tile, acc.dtype.type
    n_tiles = len(touched)
    in_tile = np.arange(L.n) % tile
    thr = dtype(thr)
    hit = (acc >= thr if flaw == "greater-or-equal" else acc > thr) & np.repeat(touched, tile)[:L.n]
    if veto is not None:
        hit &= ~veto
    if flaw == "last-vector-unswept":
        hit &= in_tile < tile - vec(dtype)
    elif flaw == "last-element-ignored":
        hit &= in_tile % vec(dtype) != vec(dtype) - 1
    elif flaw == "first-column-ignored":
        hit &= in_tile != 0
    p = np.flatnonzero(hit)
    s, j = acc[p], L.orig_of[p]
    stride = max(1, min(int(top_n), L.n))
    launches = flaw in ("restart-empty", "last-restored-lost", "floor-by-score", "floor-inclusive") or trace is not None
    if not launches:
        o = _ranked(s, j, p, flaw)[:stride]
        return j[o], s[o]
    group = n_tiles if group <= 0 else min(group, n_tiles)
    out_j, out_s = np.zeros(0, np.int64), np.zeros(0, dtype)
    for pss in range(-(-stride // LANES)):
        pass_off = LANES * pss
        keep_n = min(LANES, stride - pass_off)
        ok = np.ones(len(p), bool)
        if pss > 0:
            if len(out_j) < pass_off:
                break
            fs, fj = out_s[pass_off - 1], out_j[pass_off - 1]
            tie = (j >= fj) if flaw == "floor-inclusive" else (j > fj)
            ok = (s < fs) | ((s == fs) & tie & (flaw != "floor-by-score"))
        lj, ls, lp = np.zeros(0, np.int64), np.zeros(0, dtype), np.zeros(0, np.int64)
        for g, tb in enumerate(range(0, n_tiles, group)):
            if g > 0 and flaw == "restart-empty":
                lj, ls, lp = lj[:0], ls[:0], lp[:0]
            if g > 0 and flaw == "last-restored-lost":
                lj, ls, lp = lj[:-1], ls[:-1], lp[:-1]
            mine = ok & (p // tile >= tb) & (p // tile < tb + group)
            lj, ls, lp = np.concatenate([lj, j[mine]]), np.concatenate([ls, s[mine]]), np.concatenate([lp, p[mine]])
            o = _ranked(ls, lj, lp, flaw)[:min(LANES, keep_n)]
            lj, ls, lp = lj[o], ls[o], lp[o]
            if trace is not None:
                trace.append((pss, g, pass_off + len(lj)))
        out_j, out_s = np.concatenate([out_j[:pass_off], lj]), np.concatenate([out_s[:pass_off], ls])
    return out_j, out_s


def reference(A, B, top_n, thr, sort, dtype, flaw=None, *, tile_cols=1024, pos_of=None, group=0, lists=None, left_pos=None, cache=None):
    """The multiply in plain numpy, in ``dtype``: row by row, term by term in storage order.  A: left matrix, B: the caller's
    right-hand matrix (rows x terms).  tile_cols / pos_of / group: the index's tiles, the row permutation and SG_TILE_GROUP --
    the right answer does not depend on them, most wrong ones do.  ``lists``: lists_of(B, tile_cols, pos_of), if at hand.
    left_pos: the positions in the index of the left rows, where they are rows of B (the self-join's wrong references).
    cache: a dict of the caller's that keeps the rows' accumulators from one call to the next on the same matrices (they do
    not depend on top_n, thr and sort; a wrong reference that changes them does not use it)."""
    L = lists if lists is not None else lists_of(B, tile_cols, pos_of)
    A = sp.csr_matrix(A) if not sp.isspmatrix_csr(A) else A
    indptr, indices, data = [], [], []
    acc = None
    lost = {}
    if flaw == "mirror-257-lost":      # row r hands its matches p < r over in position order, in chunks of 256
        for i in range(A.shape[0]):
            lo, hi = A.indptr[i], A.indptr[i + 1]
            if cache is not None and i not in cache:
                cache[i] = accumulate(A.indices[lo:hi], A.data[lo:hi], L, dtype)
            acc, touched = cache[i] if cache is not None else accumulate(A.indices[lo:hi], A.data[lo:hi], L, dtype)
            lower = np.flatnonzero((acc[:left_pos[i]] > dtype(thr)))
            if len(lower) > PAIR_CHUNK:
                lost.setdefault(int(lower[PAIR_CHUNK]), []).append(int(left_pos[i]))
    for i in range(A.shape[0]):
        lo, hi = A.indptr[i], A.indptr[i + 1]
        carry = acc if flaw == "stale-accumulators" else None
        if cache is not None and flaw not in _ACCUMULATOR_FLAWS:
            if i not in cache:
                cache[i] = accumulate(A.indices[lo:hi], A.data[lo:hi], L, dtype)
            acc, touched = cache[i]
        else:
            acc, touched = accumulate(A.indices[lo:hi], A.data[lo:hi], L, dtype, flaw, carry)
        veto = None
        if flaw in ("diagonal-dropped", "earlier-tile-pair-lost", "mirror-257-lost"):
            veto = np.zeros(L.n, bool)
            if flaw == "diagonal-dropped":
                veto[left_pos[i]] = True
            elif flaw == "earlier-tile-pair-lost":
                veto = np.arange(L.n) // L.tile != left_pos[i] // L.tile
            else:
                veto[lost.get(int(left_pos[i]), [])] = True
        j, s = select(acc, touched, L, top_n, thr, flaw, group, None, veto)
        if not sort:
            o = np.argsort(j, kind="stable")
            j, s = j[o], s[o]
        indptr.append(len(j))
        indices.append(j)
        data.append(s)
    ip = np.zeros(A.shape[0] + 1, np.int64)
    np.cumsum(indptr, out=ip[1:])
    return sp.csr_matrix((np.concatenate(data + [np.zeros(0, dtype)]).astype(dtype), np.concatenate(indices + [np.zeros(0, np.int64)]).astype(np.int32), ip),
                         shape=(A.shape[0], L.n))


def port(case: Case, top_n, thr, sort):
    """The oracle's port on a case, its left matrix AS STORED: oracle.port.sp_matmul_topn_port without the sort of A's rows
    it starts with (one left row is in descending column order on purpose) -- the same C function on the same arrays."""
    import ctypes
    from oracle import port as P
    A, dtype = case.A, case.dtype
    Bt = P._as_bt_csr(case.B.T)
    n_left, n_right = A.shape[0], Bt.shape[1]
    top_n = int(max(1, min(top_n, n_right)))
    a_ip, a_ix, a_d = A.indptr.astype(np.int64), A.indices.astype(np.int32), np.ascontiguousarray(A.data)
    b_ip, b_ix, b_d = Bt.indptr.astype(np.int64), Bt.indices.astype(np.int32), np.ascontiguousarray(Bt.data)
    oc, ov, cnt = np.empty(n_left * top_n, np.int32), np.empty(n_left * top_n, dtype), np.zeros(n_left, np.int32)
    lib = P._lib()
    fn = lib.sdtn_sp_matmul_topn_f32 if dtype == np.float32 else lib.sdtn_sp_matmul_topn_f64
    c_thr = ctypes.c_float(float(np.float32(thr))) if dtype == np.float32 else ctypes.c_double(float(thr))
    rc = fn(ctypes.c_int64(n_left), ctypes.c_int64(n_right), P._p(a_ip), P._p(a_ix), P._p(a_d), P._p(b_ip), P._p(b_ix), P._p(b_d),
            ctypes.c_int32(top_n), c_thr, ctypes.c_int32(1 if sort else 0), ctypes.c_int32(4), P._p(oc), P._p(ov), P._p(cnt), ctypes.c_int32(0))
    assert rc == 0
    return P.fixed_stride_to_csr(oc, ov, cnt, top_n, (n_left, n_right))


def same(a: sp.csr_matrix, b: sp.csr_matrix) -> bool:
    return (a.shape == b.shape and a.data.dtype == b.data.dtype and np.array_equal(a.indptr, b.indptr)
            and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data))


# ------------------------------------------------------------------------------------------------------------ the census
def census(case: Case) -> dict:
    """What the kernel will meet on a case, counted from the matrices alone (no arithmetic claim: scores are only compared
    with the schedule's thresholds and with one another)."""
    if case.family == "selfjoin":
        return _census_selfjoin(case)
    L, A, tile, n = case.lists, case.A, case.tile_cols, case.n
    n_tiles = -(-n // tile)
    bounds = np.arange(n_tiles + 1) * tile
    seg_len = np.zeros((case.n_terms, n_tiles), np.int64)
    for k in range(case.n_terms):
        seg_len[k] = np.diff(np.searchsorted(L.pos[L.ptr[k]:L.ptr[k + 1]], bounds))
    out = dict(segment_lengths={}, segments_per_chunk=set(), later_chunk_segments=set(), masks=set(), row_lengths=set(),
               untouched_middle=0, only_partial_tile=0, empty_rows=0, rows_nobody_holds=0, terms_used=set(), hits_in_tile=set(),
               hit_positions=set(), whole_vectors=0, whole_stripes=0, hits_in_a_tile_max=0, at_threshold=set(), above_threshold=set(),
               rising=0, falling=0, first_group_counts=set(), first_group_later=set(), match_counts=set(), counts_by_launch={},
               tie_blocks=[], rows_per_kind={}, macs=0)
    used = np.unique(A.indices)
    out["terms_used"] = set(used.tolist())
    out["macs"] = int(seg_len.sum(axis=1)[A.indices].sum())
    for k in used:
        for t in range(n_tiles):
            if seg_len[k, t]:
                key = (int(seg_len[k, t]), "partial" if t == n_tiles - 1 else "full")
                out["segment_lengths"][key] = out["segment_lengths"].get(key, 0) + 1
    v = vec(case.dtype)
    thresholds = sorted({thr for _, thr, _ in case.schedule})
    for i in range(A.shape[0]):
        cols, vals = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
        out["row_lengths"].add(len(cols))
        out["rows_per_kind"][case.row_names[i]] = out["rows_per_kind"].get(case.row_names[i], 0) + 1
        if len(cols) == 0:
            out["empty_rows"] += 1
        elif not seg_len[cols].any():
            out["rows_nobody_holds"] += 1
        tiles_touched = seg_len[cols].any(axis=0) if len(cols) else np.zeros(n_tiles, bool)
        out["untouched_middle"] += bool(tiles_touched[0] and tiles_touched[-1] and not tiles_touched[1:-1].any())
        out["only_partial_tile"] += bool(tiles_touched[-1] and not tiles_touched[:-1].any())
        for c0 in range(0, len(cols), LANES):
            for t in range(n_tiles):
                lanes = np.flatnonzero(seg_len[cols[c0:c0 + LANES], t] > 0)
                out["segments_per_chunk"].add(len(lanes))
                if c0:
                    out["later_chunk_segments"].add((min(c0 // LANES, 2), len(lanes)))
                if len(lanes):
                    out["masks"].add((min(c0 // LANES, 1), tuple(lanes.tolist())) if len(lanes) <= 2 else "many")
        acc, touched = accumulate(cols, vals, L, case.dtype)
        for thr in thresholds:
            hit = np.flatnonzero((acc > case.dtype(thr)) & np.repeat(touched, tile)[:n])
            out["hits_in_tile"].update((hit % tile).tolist())
            out["hit_positions"].update(hit.tolist())
            if thr > 0:
                out["at_threshold"].update(np.flatnonzero(acc == case.dtype(thr)).tolist())
                out["above_threshold"].update(np.flatnonzero(acc == np.nextafter(case.dtype(thr), case.dtype(2))).tolist())
                continue
            if len(hit):
                per_tile = np.bincount(hit // tile, minlength=n_tiles)
                out["hits_in_a_tile_max"] = max(out["hits_in_a_tile_max"], int(per_tile.max()))
                vecs, cnt = np.unique(hit // v, return_counts=True)
                out["whole_vectors"] += int((cnt == v).sum())
                for e in range(v):
                    he = hit[hit % v == e]
                    stripes, cnt = np.unique((he % tile) // (v * LANES) + (he // tile) * tile, return_counts=True)
                    out["whole_stripes"] += int((cnt == LANES).sum())
                if len(hit) > LANES:
                    d = np.diff(acc[hit].astype(np.float64))
                    out["rising"] += bool((d > 0).all())
                    out["falling"] += bool((d < 0).all())
            out["match_counts"].add(len(hit))
            first = int((hit < tile).sum())
            out["first_group_counts"].add(first)
            if len(hit) > first:
                later, mine = acc[hit[hit >= tile]], acc[hit[hit < tile]]
                if first:
                    out["first_group_later"].add((first, "better" if later.min() > mine.max() else "worse" if later.max() < mine.min() else
                                                  "equal" if (later.min() == mine.min() == later.max() == mine.max()) else "mixed"))
                else:
                    out["first_group_later"].add((0, "any"))
            if case.family != "state":         # (the family that owns the state between launches and the ties)
                continue
            # the list after every launch of every (SG_TILE_GROUP, top_n) of the schedule
            for top_n, thr2, _ in case.schedule:
                if thr2 != thr:
                    continue
                for group in TILE_GROUPS:
                    trace = []
                    select(acc, touched, L, top_n, thr, None, group, trace)
                    out["counts_by_launch"].setdefault((group, top_n), set()).update(trace)
            # blocks of equal scores among the ranked hits
            j = L.orig_of[hit]
            o = _ranked(acc[hit], j, hit, None)
            s, jj, pp = acc[hit][o], j[o], hit[o]
            start = 0
            for r in range(1, len(s) + 1):
                if r == len(s) or s[r] != s[start]:
                    if r - start > 1:
                        disagree = bool((np.diff(pp[start:r]) < 0).any())       # rows ascending: are the positions?
                        out["tie_blocks"].append((start, r - 1, len(set((pp[start:r] // tile).tolist())), disagree))
                    start = r
    return out


def _census_selfjoin(case: Case) -> dict:
    """the self-join at threshold 0: every pair of rows with a term in common is a match (all values are positive)"""
    n, tile = case.n, case.tile_cols
    design = sp.csr_matrix(case.B[case.orig_of])                 # rows in position order
    pattern = sp.csr_matrix((np.ones(design.nnz, np.int32), design.indices, design.indptr), shape=design.shape)
    g = (pattern @ pattern.T).tocoo()
    lower = g.col < g.row
    mirrored = np.bincount(g.row[lower], minlength=n)            # per position: the matches the row hands over
    earlier = np.bincount(g.row[lower & (g.col // tile < g.row // tile)], minlength=n)
    rows = {}
    for p in range(n):
        key = (design.indices[design.indptr[p]:design.indptr[p + 1]].tobytes(), design.data[design.indptr[p]:design.indptr[p + 1]].tobytes())
        rows.setdefault(key, []).append(p)
    hubs = [ps for ps in rows.values() if len(ps) >= 10]
    lengths = np.diff(case.lists.ptr)
    return dict(mirrored_pairs=set(mirrored.tolist()), mirrored_from_earlier_tiles=set(mirrored[earlier > 0].tolist()),
                rows_with_pairs=set(np.flatnonzero(np.bincount(g.row[g.col != g.row], minlength=n)).tolist()),
                hubs=len(hubs), hubs_over_all_tiles=sum(len({p // tile for p in ps}) == 3 for ps in hubs),
                row_lengths=set(np.diff(design.indptr).tolist()), pairs=int(lower.sum()), macs=int((lengths * lengths).sum()))


def expected(family: str, dtype, tile_cols: int, permute: bool) -> dict:
    """The edges a family owns at this dtype and tile size: census key -> what must be found there.  An edge the tile size
    cannot hold is absent HERE, with the reason (see also the module's docstring); nothing is waived at run time."""
    v = vec(dtype)
    if family == "lists":
        lengths = {(L, "full") for L in SEGMENT_LENGTHS + (tile_cols - 1, tile_cols) if L <= tile_cols}      # (longer ones do not fit)
        return dict(segment_lengths=lengths | {(L, "partial") for L in PARTIAL_LENGTHS})
    if family == "batches":
        return dict(segments_per_chunk=set(SEGMENT_COUNTS),
                    later_chunk_segments={(ch, c) for ch in (1, 2) for c in (1, 7, 8, 9)},
                    masks={(ch, m) for ch in (0, 1) for m in ((0,), (63,), (0, 63))},
                    row_lengths={0, 64, 65, 71, 72, 73, 127, 128, 129, 192, 193},
                    untouched_middle=1, only_partial_tile=1, empty_rows=1, rows_nobody_holds=1,
                    terms_used={0, _BANKS * _BANK_M - 1})
    if family == "sweep":
        inside = {q for q in (0, 1, v - 1, v, 64 * v - 1, 64 * v, 256 * v - 1, 256 * v, tile_cols - 1) if q < tile_cols}   # (256 VEC == tile_cols: the next tile's first column)
        corners = set(sweep_positions(dtype, tile_cols))
        return dict(hits_in_tile=inside, hit_positions=corners | {tile_cols, 2 * tile_cols, 2 * tile_cols + PARTIAL - 1},
                    whole_vectors=3, whole_stripes=3, hits_in_a_tile_max=LANES + 1, rising=1, falling=1,
                    at_threshold=corners, above_threshold=corners)
    if family == "state":
        return dict(first_group_counts=set(FIRST_GROUP_COUNTS), match_counts=set(MATCH_COUNTS),
                    first_group_later={(k0, how) for k0 in FIRST_GROUP_COUNTS[1:] for how in ("better", "worse", "equal")} | {(0, "any")},
                    tie_blocks=TIE_BLOCKS)
    if family == "waves":
        return dict(untouched_middle=1, only_partial_tile=1, empty_rows=1, rows_nobody_holds=1, hits_in_a_tile_max=tile_cols)
    if family == "selfjoin":
        n = 2 * tile_cols + PARTIAL
        return dict(mirrored_pairs=set(MIRRORED_PAIRS), mirrored_from_earlier_tiles=set(MIRRORED_PAIRS),
                    rows_with_pairs={0, tile_cols - 1, tile_cols, n - 1}, hubs=3, hubs_over_all_tiles=3, row_lengths={1, 4, 64, 256},
                    pairs=2 * PAIR_CHUNK * 8 + 1)                # (more than the 8 chunks of the small pair list of the GPU test)
    raise KeyError(family)


def missing(found: dict, want: dict, permute: bool) -> list:
    """The expected edges the census did not find, named."""
    out = []
    for key, w in want.items():
        f = found[key]
        if key == "tie_blocks":
            for lo, hi in w:
                blocks = [b for b in f if b[0] <= lo and b[1] >= hi and b[2] >= 2 and (b[3] or not permute)]
                if not blocks:
                    out.append(f"a block of equal scores over ranks {lo}-{hi} with members in several tiles"
                               + (" whose row order and position order disagree" if permute else ""))
        elif isinstance(w, set):
            have = set(f.keys()) if isinstance(f, dict) else f
            out += [f"{key}: {m}" for m in sorted(w - have, key=repr)]
        elif f < w:
            out.append(f"{key}: {f} found, at least {w} wanted")
    return out
