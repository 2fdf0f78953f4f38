"""Constructed inputs, the plain reference and deliberately wrong references ("flaws") for the second pass of the multi-GPU
self-join: sg_selfjoin_merge -- pairs_flat_count_kernel, pairs_flat_fill_kernel and pairs_select_kernel of
sg_spgemm_pruned.hip.  TEST INFRASTRUCTURE ONLY: host arrays and numpy, no GPU and no library.
tests/test_merge_cases_cpu.py shows without a GPU that the inputs reach every path, batch boundary and cut of the row select
and tell the reference from the same reference with one thing wrong; tests/test_selfjoin_merge_gpu.py feeds the same inputs
to the library and expects the reference's bits.

THE CONTRACT (``ref_merge``; include/sg_hip.h says the same of sg_selfjoin_merge).  A result of n rows and `stride` columns,
a list of records {i, j, score bits}, a share (lo, hi, step) and, for an index built over the row permutation, pos_of:
  - row j is the rank's when lo <= pos_of[j] < hi and (hi - 1 - pos_of[j]) % step == 0 (pos_of = identity without a table);
  - a rank's row receives the column i, with the record's score bits, of every record whose j names it;
  - identical records, and a record that repeats the column of an entry the row holds already, count once;
  - candidates are ordered by score descending BY VALUE (-0.0 equals +0.0), then column ascending; the first `stride` stay,
    counts[j] is their number, the bits written are the candidate's own;
  - a row that is not the rank's, and a rank's row that no record names, keeps every cell and its count.

THE THREE PATHS of pairs_select_kernel, by m = the row's count + its records (repeats included) -- ``path_of``:
  rank    m <= 64: one lane a candidate, ranked against all others; repeats found by column and taken out of the ranks;
  narrow  m > 64, stride <= 64: one register list of 64, fed in batches of 64 records; the list's stride-th entry, read before
          a batch, is the bar a record must beat to be inserted at all;
  wide    m > 64, stride 65 .. 128: two register lists; the bar is entry stride - 65 of the second, and the row's own entries
          are inserted like records.
One result has one stride, so it holds rows of the rank path next to rows of ONE register path; every case here does.

Scores are k / 1024 (exact in both value types) unless a case is about the last place.  Every builder is seeded and
cached: the arrays it returns are shared and must not be written to."""
import functools
from typing import NamedTuple, Optional

import numpy as np

DTYPES = (np.float32, np.float64)
LANES = 64
COLUMN_POOL = 4096                      # the constructed columns are drawn from [0, 4096); a record's i is only ever stored

NARROW_STRIDES = (1, 2, 10, 63, 64)
WIDE_STRIDES = (65, 100, 127, 128)
BOUNDARY_M = (1, 63, 64, 65, 66)        # own + mirrored around the end of the rank path
BATCH_LENGTHS = (64, 65, 127, 128, 129, 200)     # mirrored lists around the ends of one, two and three batches
ARRIVALS = ("ascending", "descending", "shuffled")
WIDE_OWN = (0, 64, 65, 128)             # own entries of a wide row: none, the first list full, one pushed on, both full
WIDE_CUTS = (65, 100, 128)              # the bar in lane 0, in the middle and in the last lane of the second list
TIE_STRIDES = (10, 64, 100, 128)
REPEAT_STRIDES = (10, 64, 100)
ARRIVAL_STRIDES = (10, 100)
ORDERS = ("as-built", "reversed", "shuffled")
STEPS = (1, 2, 3, 7)
SIZES = (1, 63, 64, 65, 129)
PERMUTED_ROWS = 9000                    # more than two tiles of 4096 rows: the library builds such an index over its permutation
PERMUTED_SHARE = (1000, 8000, 3)
PERMUTED_STRIDES = (10, 100)


class RowInfo(NamedTuple):
    """What a case says of one of its rows that records name."""
    row: int
    own: int              # entries the row holds before the merge
    mirrored: int         # records that name it, repeats included
    path: str             # "rank", "narrow", "wide"; "outside": not a row of the share -- it must stay as it is
    arrival: str          # the order of the row's records in the list: one of ARRIVALS, or "" where nothing is said
    what: str


class MergeCase(NamedTuple):
    name: str
    cols: np.ndarray      # int32 [n, stride]      the result before the merge
    vals: np.ndarray      # float32 / float64 [n, stride]
    counts: np.ndarray    # int32 [n]
    n_cols: int
    pairs: np.ndarray     # int32 [records, 3 or 4]: {i, j, score bits}, f64 as (lo, hi) words
    lo: int
    hi: int
    step: int
    pos_of: Optional[np.ndarray]
    rows: tuple           # of RowInfo, one per row that a record names

    @property
    def stride(self):
        return self.cols.shape[1]

    @property
    def words(self):
        return self.pairs.shape[1]


def words_of(dtype) -> int:
    return 4 if np.dtype(dtype) == np.float64 else 3


def record_scores(pairs: np.ndarray, dtype) -> np.ndarray:
    """the scores of a record list, from their bits"""
    if len(pairs) == 0:
        return np.zeros(0, dtype)
    return np.ascontiguousarray(pairs[:, 2:]).view(dtype).ravel()


def make_records(i, j, scores, dtype) -> np.ndarray:
    scores = np.ascontiguousarray(scores, dtype)
    out = np.zeros((len(scores), words_of(dtype)), np.int32)
    out[:, 0], out[:, 1] = i, j
    out[:, 2:] = scores.view(np.int32).reshape(len(scores), -1)
    return out


def path_of(m: int, stride: int) -> str:
    return "rank" if m <= LANES else ("wide" if stride > LANES else "narrow")


def is_member(pos, lo, hi, step) -> bool:
    return lo <= pos < hi and (hi - 1 - pos) % max(int(step), 1) == 0


# ---------------------------------------------------------------------------------------------------- the reference
FLAWS = {
    "bits-order": "the order taken by the scores' bits instead of their value: -0.0 goes behind every +0.0",
    "arrival-ties": "a tie broken by arrival instead of by column",
    "repeats-counted": "a repeated record entered and counted again",
    "cut-at-stride-1": "the row cut one entry short of the stride",
    "wide-cut-at-64": "a row of the wide path cut at one register list",
    "bar-drops-equal": "a bar that also turns away records that tie with it on the score",
    "no-residue": "membership without the residue: every position of [lo, hi) is the rank's",
    "membership-on-j": "membership tested on the row number instead of on its position",
    "outside-rewritten": "rows outside the share merged like the rank's own",
}


def _by_value(c, v):
    """score descending by value, then column ascending (lexsort is stable and compares -0.0 == +0.0)"""
    return np.lexsort((c, -v))


def _batched(oc, ov, mc, mv, keep, drop_equal):
    """The register paths restated: the own entries, then the records in batches of 64, each record held against the bar --
    the list's keep-th entry as it was BEFORE the batch -- and entered unless its column is in the list.  The list holds 64
    or 128.  drop_equal: the bar compares scores only."""
    if keep <= 0:
        return np.zeros(0, np.int64)
    cap = LANES if keep <= LANES else 2 * LANES
    key = lambda e: (-e[0], e[1])
    lst = sorted(zip(ov.tolist(), oc.tolist(), range(len(oc))), key=key)        # (score, column, where the bits are)
    for base in range(0, len(mc), LANES):
        bar = lst[keep - 1] if len(lst) >= keep else None
        for k in range(base, min(base + LANES, len(mc))):
            s, c = float(mv[k]), int(mc[k])
            if bar is not None and not (s > bar[0] or (not drop_equal and s == bar[0] and c < bar[1])):
                continue
            if any(c == e[1] for e in lst):
                continue
            lst = sorted(lst + [(s, c, len(oc) + k)], key=key)[:cap]
    return np.array([e[2] for e in lst[:keep]], np.int64)


def _select(oc, ov, mc, mv, stride, flaw=None, batched=False):
    """the entries a row keeps, as indices into own + records"""
    c, v = np.concatenate([oc, mc]), np.concatenate([ov, mv])
    m, keep = len(c), stride
    if flaw == "cut-at-stride-1":
        keep = stride - 1
    if flaw == "wide-cut-at-64" and m > LANES and stride > LANES:
        keep = LANES
    if (batched or flaw == "bar-drops-equal") and m > LANES:
        return _batched(oc, ov, mc, mv, keep, flaw == "bar-drops-equal")
    idx = np.arange(m)
    if flaw != "repeats-counted":
        idx = np.sort(np.unique(c, return_index=True)[1])       # the first of every column, in arrival order
    cc, vv = c[idx], v[idx]
    if flaw == "bits-order":
        bits = vv.view(np.int32 if vv.dtype == np.float32 else np.int64)
        order = np.lexsort((cc, ~bits))         # (as signed integers, descending: right for scores >= +0.0)
    elif flaw == "arrival-ties":
        order = np.argsort(-vv, kind="stable")
    else:
        order = _by_value(cc, vv)
    return idx[order[:max(keep, 0)]]


def ref_merge(res, pairs, lo, hi, step, pos_of=None, flaw=None, batched=False):
    """The contract on host arrays.  res: (cols, vals, counts); returns new ones.  flaw: one of FLAWS -- the same with one
    thing wrong.  batched: the rows beyond 64 candidates through the restated register paths (the same answer)."""
    cols, vals, counts = (np.array(a) for a in res)
    n, stride = cols.shape
    scores = record_scores(pairs, vals.dtype)
    pos = np.arange(n) if pos_of is None or flaw == "membership-on-j" else np.asarray(pos_of)
    step_used = 1 if flaw == "no-residue" else step
    for j in (np.unique(pairs[:, 1]) if len(pairs) else ()):
        if flaw != "outside-rewritten" and not is_member(int(pos[j]), lo, hi, step_used):
            continue
        mine = np.flatnonzero(pairs[:, 1] == j)
        k = int(counts[j])
        oc, ov = cols[j, :k].copy(), vals[j, :k].copy()
        mc, mv = pairs[mine, 0], scores[mine]
        sel = _select(oc, ov, mc, mv, stride, flaw, batched)
        c, v = np.concatenate([oc, mc]), np.concatenate([ov, mv])
        counts[j] = len(sel)
        cols[j, :len(sel)], vals[j, :len(sel)] = c[sel], v[sel]
    return cols, vals, counts


def ref_case(case: MergeCase, flaw=None, batched=False):
    return ref_merge((case.cols, case.vals, case.counts), case.pairs, case.lo, case.hi, case.step, case.pos_of, flaw, batched)


def same(a, b) -> bool:
    """two results (cols, vals, counts), every cell, the values by their bits"""
    return np.array_equal(a[0], b[0]) and a[1].dtype == b[1].dtype and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------- what a case must hold
def check_case(case: MergeCase):
    """The conditions under which the contract has ONE answer, and the case's own statement of its rows' paths."""
    n, stride = case.cols.shape
    assert case.cols.dtype == np.int32 and case.counts.dtype == np.int32 and case.pairs.dtype == np.int32
    assert case.vals.shape == case.cols.shape and len(case.counts) == n and case.pairs.shape[1] == words_of(case.vals.dtype)
    assert (case.counts >= 0).all() and (case.counts <= stride).all(), f"{case.name}: a count outside the stride"
    assert 1 <= stride <= 2 * LANES, f"{case.name}: the row select holds 128 entries"
    assert 0 <= case.lo <= case.hi <= n and case.step >= 1
    if len(case.pairs):
        assert (case.pairs[:, 1] >= 0).all() and (case.pairs[:, 1] < n).all(), f"{case.name}: a record names a row outside the result"
    assert case.pos_of is None or np.array_equal(np.sort(case.pos_of), np.arange(n))
    scores = record_scores(case.pairs, case.vals.dtype)
    bits = np.int32 if case.vals.dtype == np.float32 else np.int64
    named = set(np.unique(case.pairs[:, 1]).tolist()) if len(case.pairs) else set()
    assert named == {r.row for r in case.rows} and len(case.rows) == len(named), f"{case.name}: the rows said and the rows named differ"
    for r in case.rows:
        mine = np.flatnonzero(case.pairs[:, 1] == r.row)
        k = int(case.counts[r.row])
        c = np.concatenate([case.cols[r.row, :k], case.pairs[mine, 0]])
        b = np.concatenate([case.vals[r.row, :k], scores[mine]]).view(bits)
        assert len(np.unique(case.cols[r.row, :k])) == k, f"{case.name} row {r.row}: the row holds a column twice"
        first = {}
        for cc, bb in zip(c.tolist(), b.tolist()):
            assert first.setdefault(cc, bb) == bb, f"{case.name} row {r.row}: column {cc} with two different scores"
        pos = r.row if case.pos_of is None else int(case.pos_of[r.row])
        path = path_of(k + len(mine), stride) if is_member(pos, case.lo, case.hi, case.step) else "outside"
        assert (r.own, r.mirrored, r.path) == (k, len(mine), path), f"{case.name} row {r.row}: said {r}, is {(k, len(mine), path)}"


class _Builder:
    """A result whose every cell is set -- beyond a row's count to a value no candidate has, so that a stray write shows --
    and the records of its rows."""

    def __init__(self, name, dtype, n, stride, seed, n_cols=None):
        self.name, self.dtype, self.n, self.stride = name, np.dtype(dtype).type, n, stride
        self.rng = np.random.default_rng(seed)
        self.n_cols = max(n, COLUMN_POOL) if n_cols is None else n_cols
        self.cols = np.tile((self.n_cols - 1 - np.arange(stride)).astype(np.int32), (n, 1))
        self.vals = np.full((n, stride), 0.123, self.dtype)
        self.counts = np.zeros(n, np.int32)
        self.records, self.said, self.taken = [], [], set()

    def draw(self, m, ties=True):
        """m candidates: distinct columns; scores k / 1024, some of them equal (ties) or all distinct"""
        cols = self.rng.permutation(COLUMN_POOL)[:m]
        if ties:
            k = self.rng.integers(1, max(3 * m // 2, 2) + 1, m)
        else:
            k = 1 + self.rng.permutation(1000)[:m]
        return cols.astype(np.int32), (k / 1024).astype(self.dtype)

    def row(self, j, own, mirrored, arrival="", what=""):
        """own, mirrored: (columns, scores).  The own entries are stored as the multiply leaves a row: by score descending,
        then column ascending.  The records keep their order."""
        assert 0 <= j < self.n and j not in self.taken, (self.name, j)
        self.taken.add(j)
        oc, ov = np.asarray(own[0], np.int32), np.asarray(own[1], self.dtype)
        order = _by_value(oc, ov)
        k = len(oc)
        assert k <= self.stride
        self.cols[j, :k], self.vals[j, :k], self.counts[j] = oc[order], ov[order], k
        mc, mv = np.asarray(mirrored[0], np.int32), np.asarray(mirrored[1], self.dtype)
        if len(mc):
            self.records.append(make_records(mc, j, mv, self.dtype))
            self.said.append((j, k, len(mc), arrival, what))

    def split(self, j, c, v, own, arrival="shuffled", what=""):
        """candidates (c, v) of which a random `own` are the row's own and the others arrive as said"""
        pick = self.rng.permutation(len(c))
        o, m = pick[:own], pick[own:]
        if arrival == "ascending":
            m = m[np.lexsort((c[m], v[m]))]
        elif arrival == "descending":
            m = m[np.lexsort((c[m], v[m]))[::-1]]
        self.row(j, (c[o], v[o]), (c[m], v[m]), arrival, what)

    def quiet_rows(self):
        """every row not taken yet holds a few entries and gets no record"""
        for j in range(self.n):
            if j not in self.taken:
                c, v = self.draw(int(self.rng.integers(0, min(self.stride, 4) + 1)))
                self.row(j, (c, v), ((), ()))

    def finish(self, lo=0, hi=None, step=1, pos_of=None, order="as-built") -> MergeCase:
        hi = self.n if hi is None else hi
        pairs = np.concatenate(self.records) if self.records else np.zeros((0, words_of(self.dtype)), np.int32)
        if order == "reversed":
            pairs = pairs[::-1].copy()
        elif order == "shuffled":
            pairs = pairs[np.random.default_rng(len(pairs)).permutation(len(pairs))]
        rows = []
        for j, k, m, arrival, what in self.said:
            pos = j if pos_of is None else int(pos_of[j])
            rows.append(RowInfo(j, k, m, path_of(k + m, self.stride) if is_member(pos, lo, hi, step) else "outside",
                                arrival if order == "as-built" else "", what))
        case = MergeCase(self.name, self.cols, self.vals, self.counts, self.n_cols, np.ascontiguousarray(pairs), lo, hi, step,
                         None if pos_of is None else np.asarray(pos_of, np.int64), tuple(rows))
        check_case(case)
        for a in (case.cols, case.vals, case.counts, case.pairs):
            a.setflags(write=False)
        return case


def _seed(*parts):
    """a seed from a case's name: the same in every process"""
    return sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(str(p) for p in parts)))


# ---------------------------------------------------------------------------------------------------- the cases
def _boundaries(dtype, S):
    """own + mirrored = 1, 63, 64, 65, 66 with none, one and a full stride of own entries, an untouched row between any two"""
    combos = [(m, own) for m in BOUNDARY_M for own in sorted({0, 1, S}) if own <= min(S, m - 1)]
    b = _Builder(f"boundaries-{S}", dtype, 2 * len(combos) + 1, S, _seed("boundaries", S))
    for k, (m, own) in enumerate(combos):
        c, v = b.draw(m)
        b.split(2 * k + 1, c, v, own, what=f"m={m} own={own}")
    b.quiet_rows()
    return b.finish()


def _batches(dtype, S):
    """mirrored lists of 64 .. 200 records behind own entries, arriving ascending (the bar never helps: everything is
    inserted), descending (the bar is up after the first batch) and shuffled; all scores distinct"""
    owns = [o for o in WIDE_OWN if o <= S] if S > LANES else [1, S]
    b = _Builder(f"batches-{S}", dtype, 2 * len(BATCH_LENGTHS) * len(ARRIVALS) + 1, S, _seed("batches", S))
    k = 0
    for iL, L in enumerate(BATCH_LENGTHS):
        for ia, arrival in enumerate(ARRIVALS):
            own = owns[(iL + ia) % len(owns)]
            if own + L <= LANES:
                own = 1             # (64 records and nothing of its own is the rank path: tests/_merge_cases.py, boundaries)
            c, v = b.draw(own + L, ties=False)
            b.split(2 * k + 1, c, v, own, arrival, what=f"L={L} own={own} {arrival}")
            k += 1
    b.quiet_rows()
    return b.finish()


def _ties(dtype, S):
    dt = np.dtype(dtype).type
    b = _Builder(f"ties-{S}", dtype, 24, S, _seed("ties", S))
    rng = b.rng
    x = dt(0.5)
    # 100 and 200 candidates of one score, the lowest columns anywhere in the list
    c = rng.permutation(COLUMN_POOL)[:100]
    b.row(1, ((), ()), (c, np.full(100, x)), what="100 of one score")
    c = rng.permutation(COLUMN_POOL)[:200]
    own = min(S, 5)
    b.row(2, (c[:own], np.full(own, x)), (c[own:], np.full(200 - own, x)), what="200 of one score, own entries among them")
    # 62 higher scores, six equal ones at entries 62 .. 67, 82 lower ones
    c = rng.permutation(COLUMN_POOL)[:150]
    v = np.concatenate([(1000 - np.arange(62)) / 1024, np.full(6, 0.75), (700 - np.arange(82)) / 1024]).astype(dt)
    b.split(4, c, v, min(S, 20), what="a tie across entries 62 .. 67")
    # S - 1 higher scores, then one score three times: own column 50 between the records' 40 and 60 -- 40 makes the cut
    for j, extra in ((6, 0), (7, 70)):
        high = rng.permutation(np.arange(100, COLUMN_POOL))[:S - 1 + extra]
        hv = np.concatenate([(1000 - np.arange(S - 1)) / 1024, (300 - np.arange(extra)) / 1024]).astype(dt)
        n_own = min(S - 1, 2)
        order = rng.permutation(S - 1 + extra)
        o, m = order[order < n_own], order[order >= n_own]
        b.row(j, (np.concatenate([[50], high[o]]), np.concatenate([[x], hv[o]])),
              (np.concatenate([high[m], [60, 40]]), np.concatenate([hv[m], [x, x]])), what=f"an own entry ties with two records at the cut (+{extra} below)")
    # five neighbouring numbers around the cut, the larger the score the larger the column; an own entry in the middle
    for j, extra in ((9, 0), (10, 70)):
        n_high = max(S - 2, 0)
        ladder = [x]
        for _ in range(4):
            ladder.append(np.nextafter(ladder[-1], dt(0)))
        high = rng.permutation(np.arange(600, COLUMN_POOL))[:n_high + extra]
        hv = np.concatenate([(1000 - np.arange(n_high)) / 1024, (300 - np.arange(extra)) / 1024]).astype(dt)
        order = rng.permutation(n_high + extra + 4)
        mc = np.concatenate([high, [500, 400, 200, 100]])[order]
        mv = np.concatenate([hv, [ladder[0], ladder[1], ladder[3], ladder[4]]]).astype(dt)[order]
        b.row(j, ([300], [ladder[2]]), (mc, mv), what=f"scores one unit in the last place apart around the cut (+{extra} below)")
    # zeros of both signs at the cut: equal by value, the column decides, the sign stays
    for j, n_zero in ((12, 6), (13, 76)):
        n_pos = max(S - 3, 0)
        pc = rng.permutation(np.arange(600, COLUMN_POOL))[:n_pos]
        pv = ((1000 - np.arange(n_pos)) / 1024).astype(dt)
        zc = 10 + np.arange(n_zero)
        zv = np.where(zc % 2 == 0, dt(0.0), dt(-0.0)).astype(dt)
        order = rng.permutation(n_pos + n_zero - 1)
        mc = np.concatenate([pc, zc[zc != 11]])[order]
        mv = np.concatenate([pv, zv[zc != 11]])[order]
        b.row(j, ([11], [dt(-0.0)]), (mc, mv), what=f"+0.0 and -0.0 at the cut, {n_zero} zeros")
    b.quiet_rows()
    return b.finish()


def _repeats(dtype, S):
    dt = np.dtype(dtype).type
    b = _Builder(f"repeats-{S}", dtype, 20, S, _seed("repeats", S))
    rng = b.rng
    c, v = b.draw(7)
    b.row(1, (c[:2], v[:2]), (c[[2, 3, 3, 4, 5, 6, 2]], v[[2, 3, 3, 4, 5, 6, 2]]), what="two records twice: side by side, and first and last")
    c, v = b.draw(6)
    b.row(2, (c[:1], v[:1]), (c[[1, 2, 1, 3, 4, 1, 5]], v[[1, 2, 1, 3, 4, 1, 5]]), what="a record three times")
    c, v = b.draw(6)
    b.row(3, (c[:2], v[:2]), (c[[2, 0, 3, 4, 1, 5]], v[[2, 0, 3, 4, 1, 5]]), what="records that repeat the own entries' columns")
    c, v = b.draw(5)
    b.row(5, (c[:2], v[:2]), (c[[2, 3, 4, 4, 3, 2]], v[[2, 3, 4, 4, 3, 2]]), what="5 distinct of 8: the count is 5 where the stride allows")
    # beyond 64 candidates.  150 distinct records shuffled; the best of them again at the very end, and the best own entry
    c, v = b.draw(154, ties=False)
    order = np.argsort(-v)
    own, rec = order[[1, 5, 9, 13][:min(S, 4)]], np.setdiff1d(order, order[[1, 5, 9, 13][:min(S, 4)]])
    rec = rec[rng.permutation(len(rec))]
    best = rec[np.argmax(v[rec])]
    rec = np.concatenate([[best], rec[rec != best], [best, own[0]]])
    b.row(7, (c[own], v[own]), (c[rec], v[rec]), what="a repeat of an entry that is still in the list, and of an own entry")
    # the worst record first, 150 better ones after it, then the worst again: its first copy is long off the list's end
    c, v = b.draw(151, ties=False)
    order = np.argsort(v)
    rec = np.concatenate([order, order[:1]])
    b.row(8, ((), ()), (c[rec], v[rec]), arrival="", what="a repeat of an entry that has dropped off the list")
    # 40 distinct records, each twice: beyond 64 by the repeats alone
    c, v = b.draw(40)
    rec = rng.permutation(np.concatenate([np.arange(40), np.arange(40)]))
    b.row(10, ((), ()), (c[rec], v[rec]), what="80 records, 40 distinct")
    b.quiet_rows()
    return b.finish()


def _mixed_rows(b, rows_and_m, max_own=None):
    for j, m in rows_and_m:
        own = int(b.rng.integers(0, min(b.stride, m - 1, b.stride if max_own is None else max_own) + 1))
        c, v = b.draw(m)
        b.split(j, c, v, own, what=f"m={m}")


def _arrival(dtype, S, order):
    """one multiset of records in three orders: the lists are filled through an atomic cursor, only an order-free answer is right"""
    b = _Builder(f"arrival-{S}-{order}", dtype, 16, S, _seed("arrival", S))
    _mixed_rows(b, zip(range(1, 16, 2), (5, 40, 64, 65, 90, 129, 150, 200)))
    b.quiet_rows()
    return b.finish(order=order)


def _membership_layout(name, dtype, n, S, seed):
    """every row is named by records, three rows in twenty by 70 of them (even and odd rows)"""
    b = _Builder(name, dtype, n, S, seed)
    _mixed_rows(b, [(j, 70 + j % 3 if j % 10 == 4 or j % 20 == 9 else 2 + j % 4) for j in range(n)], max_own=3)
    return b


def _membership(dtype, step):
    """a share inside the rows: the records of the rows at lo - 1, at hi and of a wrong residue are there and must be ignored"""
    S = 100 if step == 3 else 10
    return _membership_layout(f"membership-{step}", dtype, 150, S, _seed("membership", step)).finish(7, 140, step, order="shuffled")


def _sizes(dtype, n):
    """a wave's 64 rows are (n + 63) / 64 apart: results of 1, 63, 64, 65 and 129 rows, every row named"""
    return _membership_layout(f"rows-{n}", dtype, n, 10, _seed("rows", n)).finish(order="shuffled")


def _nothing(dtype, which):
    b = _membership_layout(f"nothing-{which}", dtype, 70, 10, _seed("nothing"))
    if which == "empty-share":
        return b.finish(20, 20, 1)
    b.records, b.said = [], []          # no record at all
    return b.finish(0, 70, 2)


def library_permutation(n):
    """the library's fixed row permutation (tests/_numpy_ops.py restates it): (orig_of, pos_of)"""
    from tests._numpy_ops import NumpyOps
    return NumpyOps.permutation(n)


def _permuted(dtype, S):
    """Rows chosen by POSITION in an index of 9 000 rows built over the library's permutation: members of the share
    (1000, 8000, 3) and rows just outside it -- position lo - 1, hi, a wrong residue -- and rows anywhere."""
    n = PERMUTED_ROWS
    lo, hi, step = PERMUTED_SHARE
    orig_of, pos_of = library_permutation(n)
    b = _Builder(f"permuted-{S}", dtype, n, S, _seed("permuted", S), n_cols=n)
    edge = [hi - 1, hi - 1 - step, hi - 1 - 64 * step, lo + (hi - 1 - lo) % step, lo - 1, hi, hi - 2, hi - 3, lo - 1 - step, 0, n - 1]
    anywhere = b.rng.permutation(n)[:37]
    positions = list(dict.fromkeys(edge + [int(p) for p in anywhere]))
    ms = (3, 40, 64, 65, 100, 200)
    _mixed_rows(b, [(int(orig_of[p]), ms[k % len(ms)]) for k, p in enumerate(positions)])
    return b.finish(lo, hi, step, pos_of, order="shuffled")      # (the other 8 952 rows: no entries, no records)


_FAMILIES = {
    "boundaries": (_boundaries, NARROW_STRIDES + WIDE_STRIDES),
    "batches": (_batches, (10, 64) + WIDE_CUTS),
    "ties": (_ties, TIE_STRIDES),
    "repeats": (_repeats, REPEAT_STRIDES),
    "membership": (_membership, STEPS),
    "rows": (_sizes, SIZES),
    "nothing": (_nothing, ("empty-share", "no-records")),
    "permuted": (_permuted, PERMUTED_STRIDES),
}
CASES = tuple(f"{fam}-{arg}" for fam, (_, args) in _FAMILIES.items() for arg in args) + \
    tuple(f"arrival-{S}-{order}" for S in ARRIVAL_STRIDES for order in ORDERS)


@functools.lru_cache(maxsize=None)
def _case(name, dtype) -> MergeCase:
    fam, _, arg = name.partition("-")
    if fam == "arrival":
        S, _, order = arg.partition("-")
        return _arrival(dtype, int(S), order)
    build, args = _FAMILIES[fam]
    return build(dtype, next(a for a in args if str(a) == arg))


def case(name, dtype) -> MergeCase:
    return _case(name, np.dtype(dtype).type)


_REF = {}


def want(name, dtype):
    """the contract's answer for a case: computed once and shared, never to be written to"""
    key = (name, np.dtype(dtype).name)
    if key not in _REF:
        _REF[key] = ref_case(case(name, dtype))
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]
