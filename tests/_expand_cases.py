"""Inputs for the expansion of grouped results (sg_collapse.hip: expand_simple_kernel, expand_merge_kernel; sg_spgemm_topn.hip:
sg_topn_expand_groups, sg_topn_expand_range, expand_left_rows_kernel), the statement they are held to, a census of what the
inputs reach, and references that take one wrong turn each.

The layout is built as CSR, not from names: the rows of group k are ``{k: 1.0}``, so the matrix is cosine-like, the index
build groups it under SG_COLLAPSE=1, and a left row ``{k: w_k}`` scores exactly ``w_k`` against group k (one product, added to
+0.0).  A row over groups -- what the multiply on the representatives leaves: (score descending, group ascending) -- is then
written down directly, run by run, and every score is an exact binary fraction in float32 and float64.

-0.0 is not used anywhere: the multiply's sums start at +0.0 and cannot produce it, so a row over groups never holds it and
the expansion's contract does not cover it (a run at -0.0 next to one at +0.0 would compare equal and be one run).

What "every kind goes to groups of every size class" means here: a stride's kinds are dealt in rotation to the groups of one
member, of two and of three (hundreds each, every kind lands on each class: the census asserts it); the nine groups that exist
once (63, 64, 65, 130, 1 000 members, the one on the lowest rows, the one on the last rows, the two that alternate) receive
one queued kind each, another at every stride."""
import numpy as np
import scipy.sparse as sp

from tests._grouping_cases import expected_gid, expected_members

DTYPES = (np.float32, np.float64)
STRIDES = (1, 2, 10, 64, 65, 128, 200)
TOP_NS = (1, 2, 10, 64, 65, 128)
RUNS = (2, 3, 63, 64, 65, 66, 128)
TILE = 1024                      # the index tile of the tests: more than 2 x TILE groups -> built over the row permutation
LANES = 64                       # expand_merge_kernel: runs of at most LANES groups in one branch, longer ones in the other
MERGE_BLOCKS = 2048              # workgroups of expand_merge_kernel: more queued rows than that make a block take several
HI, STEP = 2.0 ** -4, 2.0 ** -13   # scores are HI - i * STEP, i < 256: in [2^-5, 2^-4], 200 of them squared sum to < 1
THRESHOLD = 2.0 ** -7            # the one-sided products: below every positive score used

SPECIAL = (("first", 10), ("last", 11), ("alt_a", 6), ("alt_b", 6), ("h63", 63), ("h64", 64), ("h65", 65), ("h130", 130),
           ("h1000", 1000))
N_TWOS, N_THREES, N_SINGLES = 210, 150, 1800


class Layout:
    """A matrix of unit rows, its group table as numpy states it (tests/_grouping_cases.py), and the types by name."""

    def __init__(self, A, type_of_row=None):
        self.A, self.n = A, A.shape[0]
        self.gid, self.n_groups = expected_gid(A)
        self.members, self.size = expected_members(self.gid)
        self.group_ptr = np.concatenate([[0], np.cumsum(self.size)])
        self.reps = self.members[self.group_ptr[:-1]]
        self.U = A[self.reps]                                   # the representatives' matrix, groups in order
        if type_of_row is not None:
            self.group_of_type = np.empty(type_of_row.max() + 1, np.int64)
            self.group_of_type[type_of_row] = self.gid

    def rows_of(self, g):
        return self.members[self.group_ptr[g]:self.group_ptr[g + 1]]


_LAYOUTS = {}


def layout(dtype):
    """4 025 rows in 2 169 groups: SPECIAL, 210 groups of two, 150 of three, 1 800 rows that stand alone.  "first" owns rows
    0 .. 9, the two alternating groups rows 10 .. 21 (a, b, a, b, ...), "last" the last 11 rows; everything else is shuffled
    with a fixed seed, so the members of different groups interleave.  2 225 rows sit in groups of several members."""
    dtype = np.dtype(dtype).type
    if dtype in _LAYOUTS:
        return _LAYOUTS[dtype]
    size_of_type = np.array([s for _, s in SPECIAL] + [2] * N_TWOS + [3] * N_THREES + [1] * N_SINGLES)
    n, n_types = int(size_of_type.sum()), len(size_of_type)
    type_of_row = np.full(n, -1, np.int64)
    type_of_row[:10] = 0
    type_of_row[10:22] = [2, 3] * 6
    type_of_row[n - 11:] = 1
    rest = np.repeat(np.arange(4, n_types), size_of_type[4:])
    type_of_row[22:n - 11] = rest[np.random.default_rng(7).permutation(len(rest))]
    A = sp.csr_matrix((np.ones(n, dtype), type_of_row.astype(np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, n_types))
    L = Layout(A, type_of_row)
    L.type_of_row = type_of_row
    L.t = {name: i for i, (name, _) in enumerate(SPECIAL)}
    by_gid = lambda types: sorted(types, key=lambda t: L.group_of_type[t])
    k = len(SPECIAL)
    L.twos = by_gid(range(k, k + N_TWOS))
    L.threes = by_gid(range(k + N_TWOS, k + N_TWOS + N_THREES))
    L.singles = by_gid(range(k + N_TWOS + N_THREES, n_types))
    # a group of two with a row that stands alone BETWEEN its members: the single comes after it in a tie, and belongs between
    L.two_around = L.single_inside = None
    single_rows = {int(L.rows_of(L.group_of_type[t])[0]): t for t in L.singles}
    for t in L.twos:
        a, b = L.rows_of(L.group_of_type[t])
        inside = [r for r in range(a + 1, b) if r in single_rows]
        if inside:
            L.two_around, L.single_inside = t, single_rows[inside[0]]
            break
    assert L.two_around is not None and L.n_groups == n_types > 2 * TILE
    _LAYOUTS[dtype] = L
    return L


def variant(dtype):
    """A layout whose groups DO score against each other: 70 types ``{t: 0.5, 70: 0.5}`` in groups of 1, 2, 3, 1, 1, 4 rows,
    shuffled.  A row scores 0.5 against its own group and 0.25 against every other: the self-product's rows over groups are
    one group, then a run of 69 -- and there are fewer groups (70) than top_n 128 asks columns for."""
    dtype = np.dtype(dtype).type
    if ("variant", dtype) not in _LAYOUTS:
        types = np.repeat(np.arange(70), np.resize([1, 2, 3, 1, 1, 4], 70))
        types = types[np.random.default_rng(11).permutation(len(types))]
        n = len(types)
        indices = np.stack([types, np.full(n, 70)], axis=1).astype(np.int32).ravel()
        A = sp.csr_matrix((np.full(2 * n, 0.5, dtype), indices, 2 * np.arange(n + 1, dtype=np.int64)), shape=(n, 71))
        _LAYOUTS["variant", dtype] = Layout(A, types)
    return _LAYOUTS["variant", dtype]


VARIANT_THRESHOLD = 0.125


# ---------------------------------------------------------------------------------------------- rows over groups, by kind
class _Row:
    """One row over groups under construction: segments of (score, types); a segment of several types is a run of ties."""

    def __init__(self, L, dtype):
        self.L, self.dtype, self.segs, self.level = L, dtype, [], 0
        self.at = {"s": 0, "2": 0, "3": 0}

    def take(self, pool, k=1):
        src = {"s": self.L.singles, "2": self.L.twos, "3": self.L.threes}[pool]
        skip = (self.L.two_around, self.L.single_inside)
        out = []
        while len(out) < k:
            t = src[(self.at[pool] * 11 + 5) % len(src)]  # (11 is coprime to every pool's length: a walk through all of it, not in group order)
            self.at[pool] += 1
            if t not in skip:
                out.append(t)
        return out

    def seg(self, types, score=None):
        if score is None:
            score = HI - self.level * STEP
            self.level += 1
        self.segs.append((self.dtype(score), list(types)))
        return self

    def each(self, types):
        for t in types:
            self.seg([t])
        return self

    def lean(self, R):
        """a run of R groups: a group of two, a group of three (R > 2), the rest single rows -- R + 3 members (R = 2: 5)"""
        return self.take("2") + self.take("3") + self.take("s", R - 2)

    def compose(self, total, multi_only=False):
        """types whose sizes sum to ``total``: threes, then a two or a single (``multi_only``: twos instead); None: impossible"""
        if total == 0:
            return []
        if multi_only and total % 3 == 1:
            return None if total < 4 else self.take("3", (total - 4) // 3) + self.take("2", 2)
        rest = {0: [], 1: ("s", 1), 2: ("2", 1)}[total % 3]
        return self.take("3", total // 3) + (self.take(*rest) if rest else [])

    def n_groups(self):
        return sum(len(t) for _, t in self.segs)


def kinds(L, S, dtype):
    """The kinds of rows a result of stride S can hold: [(name, [(score, [types])])], scores descending."""
    t, out = L.t, []

    def add(name, row):
        if row is not None and row.n_groups() <= S:
            assert len(set(x for _, ts in row.segs for x in ts)) == row.n_groups(), name
            out.append((name, row.segs))

    new = lambda: _Row(L, dtype)
    add("count-0", new())
    add("one-single", new().seg(L.singles[:1]))
    sizes = {1: L.singles[3], 2: L.twos[3], 3: L.threes[3], **{s: t[name] for name, s in SPECIAL}}
    below = [z for z in sizes if z < S]
    for z in sorted(set(([max(below)] if below else []) + [z for z in (S, S + 1) if z in sizes] + [1000])):
        add(f"one-group-of-{z}", new().seg([sizes[z]]))
    for name, total, tail in (("below", S - 1, None), ("equal", S, None), ("edge", S, "2"), ("inside", S - 1, "3")):
        r = new()
        groups = r.compose(total, multi_only=True)
        if groups is None or (not groups and not tail):
            continue
        add(f"distinct-{name}", r.each(groups + (r.take(tail) if tail else [])))
    for R in (3, 70):
        if 2 <= min(R, S) and (R == 3 or S >= R):
            r = new()
            add(f"singles-run-{min(R, S)}", r.seg(r.take("s", min(R, S))))
            r = new()
            add(f"singles-run-{min(R, S)}-then-lower", r.seg(r.take("s", min(R, S))).seg(r.take("2")))
    for R in sorted(set(RUNS + (S,))):
        if not 2 <= R <= S:
            continue
        r = new()
        add(f"run{R}-front-then-lower", r.seg(r.lean(R)).seg(r.take("s")))
        r = new()
        add(f"run{R}-front-alone", r.seg(r.lean(R)))
        r = new()
        add(f"run{R}-behind-one-last", r.seg(r.take("s")).seg(r.lean(R)))
        r = new()
        fat = [t["h1000"], t["h130"]] + [x for i in range(R - 2) for x in r.take("s2"[i % 2])]
        add(f"run{R}-fat-cut-inside", r.seg(fat).seg(r.take("s")))
        if S - (R + 3 if R > 2 else 5) >= 0:
            r = new()
            add(f"run{R}-cut-at-its-end", r.each(r.compose(S - (R + 3 if R > 2 else 5))).seg(r.lean(R)).seg(r.take("s")))
    r = new()
    add("cut-before-the-run", r.each(r.compose(S)).seg(r.take("2") + r.take("3")))
    r = new()
    add("short-then-long", r.seg(r.lean(3)).seg(r.lean(66)))
    r = new()
    add("long-then-short", r.seg(r.lean(66)).seg(r.lean(3)))
    r = new()
    add("hub-run", r.seg(([t["h1000"]] + r.take("2") + r.take("s"))[:min(3, S)]))
    r = new()
    add("alternating-run", r.seg([t["alt_a"], t["alt_b"]] + (r.take("s") if S >= 3 else [])))
    r = new()
    add("runs-out", r.seg(r.take("2") + [t["h130"]]))
    r = new()
    add("runs-out-long", r.seg(r.take("2", 64) + [t["h130"], t["h65"]]))
    r = new()
    add("long-run-with-the-lowest-rows", r.seg([t["first"]] + r.take("s", 40) + r.take("2", 24 + (S >= 66))))
    lowest_single, late_two = L.singles[0], L.twos[-1]
    assert L.group_of_type[lowest_single] < L.group_of_type[late_two]
    add("single-before-only", new().seg([lowest_single, late_two]))
    r = new()
    add("single-before-only-then-lower", r.seg([lowest_single, late_two]).seg(r.take("s")))
    add("single-after-only", new().seg([L.two_around, L.single_inside]))
    r = new()
    add("single-after-only-behind-one", r.seg(r.take("s")).seg([L.two_around, L.single_inside]))
    r = new()
    add("full-count", r.each(r.take("s", S - 2)).seg(r.take("2") + r.take("s")) if S >= 2 else r.seg(r.take("2")))
    r = new()
    add("negative-run", r.seg(r.take("s")).seg(r.take("2") + r.take("3"), -HI))
    r = new()
    add("negative-run-2", r.seg(r.take("2") + r.take("s"), -HI))
    r = new()
    add("zero-run", r.seg(r.take("2") + r.take("s"), 0.0))
    # two groups one ulp apart, the LOWER score on the lower rows: merged, its columns would come first
    add("ulp-neighbours", new().seg([L.twos[-1]], HI).seg([L.twos[0]], np.nextafter(dtype(HI), dtype(0))))
    return out


def to_entries(L, segs, dtype):
    """(groups, scores) of a row as the multiply leaves it: score descending, then group ascending"""
    cols, vals = [], []
    for score, types in segs:
        cols += sorted(int(L.group_of_type[x]) for x in types)
        vals += [score] * len(types)
    assert all(a > b for (a, _), (b, _) in zip(segs, segs[1:])), "segments descend"
    return np.array(cols, np.int32), np.array(vals, dtype)


class Case:
    """A result over the groups of ``layout(dtype)`` at stride S: one kind a group, dealt as the module's header says."""

    def __init__(self, dtype, S):
        dtype = np.dtype(dtype).type
        self.dtype, self.S = dtype, S
        L = self.L = layout(dtype)
        self.kinds = kinds(L, S, dtype)
        self.names = [k for k, _ in self.kinds]
        self.rows = [to_entries(L, segs, dtype) for _, segs in self.kinds]
        self.queued = np.array([is_queued(L, c, v, S) for c, v in self.rows])
        self.kind_of_group = np.empty(L.n_groups, np.int64)
        n_kinds = len(self.kinds)
        for cls in (1, 2, 3):
            g = np.flatnonzero(L.size == cls)
            self.kind_of_group[g] = (np.arange(len(g)) + S) % n_kinds
        special = [int(L.group_of_type[L.t[name]]) for name, _ in SPECIAL]
        pool = np.flatnonzero(self.queued) if self.queued.any() else np.arange(n_kinds)
        self.kind_of_group[special] = pool[(np.arange(len(special)) + STRIDES.index(S)) % len(pool)]
        self.cols = np.zeros((L.n_groups, S), np.int32)
        self.vals = np.zeros((L.n_groups, S), dtype)
        self.counts = np.zeros(L.n_groups, np.int32)
        for k, (c, v) in enumerate(self.rows):
            g = np.flatnonzero(self.kind_of_group == k)
            self.cols[g, :len(c)], self.vals[g, :len(c)], self.counts[g] = c, v, len(c)
        self.row_queued = self.queued[self.kind_of_group[L.gid]]
        rng = np.random.default_rng(100 + S)
        hub = L.rows_of(L.group_of_type[L.t["h1000"]])
        self.row_lists = {
            "all": None,
            "ascending": np.flatnonzero(rng.random(L.n) < 0.4),
            "shuffled": rng.permutation(L.n)[:1500],
            "single": hub[-1:],
            "none-queued": np.flatnonzero(~self.row_queued),
        }

    def n_queued(self, which):
        rows = self.row_lists[which]
        return int(self.row_queued.sum() if rows is None else self.row_queued[rows].sum())


_CASES = {}


def case(dtype, S):
    key = (np.dtype(dtype).type, S)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------- the statement
def ref_expand(L, rows, cols, vals, counts, stride, left=False):
    """The statement (``NumpyOps.expand_rows`` of tests/_numpy_ops.py, vectorised, with the output's stride a parameter):
    output row k is, for the caller's row ``rows[k]`` (None: every row), ALL members of ALL groups of row ``gid[rows[k]]`` of
    the result over groups, each with its group's score, ordered by (score descending, column ascending), cut at ``stride``.
    ``left``: the result's rows are the caller's left rows themselves (a one-sided product: no row -> group table)."""
    rows = np.arange(cols.shape[0] if left else L.n) if rows is None else np.asarray(rows, np.int64)
    src, inverse = np.unique(rows if left else L.gid[rows], return_inverse=True)
    cnt = counts[src].astype(np.int64)
    r_idx = np.repeat(np.arange(len(src)), cnt)
    e_idx = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    g, sc = cols[src[r_idx], e_idx].astype(np.int64), vals[src[r_idx], e_idx]
    sz = L.size[g]
    rr, ss = np.repeat(r_idx, sz), np.repeat(sc, sz)
    mem = L.members[np.repeat(L.group_ptr[g], sz) + np.arange(sz.sum()) - np.repeat(np.cumsum(sz) - sz, sz)]
    order = np.lexsort((mem, -ss, rr))
    rr, ss, mem = rr[order], ss[order], mem[order]
    rank = np.arange(len(rr)) - np.searchsorted(rr, np.arange(len(src)))[rr]
    keep = rank < stride
    out_c = np.zeros((len(src), stride), np.int32)
    out_v = np.zeros((len(src), stride), vals.dtype)
    out_c[rr[keep], rank[keep]], out_v[rr[keep], rank[keep]] = mem[keep], ss[keep]
    out_n = np.bincount(rr[keep], minlength=len(src)).astype(np.int32)
    return out_c[inverse], out_v[inverse], out_n[inverse]


def range_rows(L, pos_of, lo, hi, step=1, from_lo=False):
    """sg_topn_expand_range's rows: those whose group sits at a position p of [lo, hi) with (hi - 1 - p) % step == 0, ascending.
    ``from_lo``: the wrong turn -- every step-th position counted from ``lo``."""
    p = (np.arange(L.n_groups) if pos_of is None else np.asarray(pos_of))[L.gid]
    mine = (p >= lo) & (p < hi) & (((p - lo) if from_lo else (hi - 1 - p)) % max(step, 1) == 0)
    return np.flatnonzero(mine)


def fixed(C, stride):
    """a CSR result (rows in result order) as fixed-stride arrays"""
    cnt = np.diff(C.indptr).astype(np.int32)
    cols, vals = np.zeros((C.shape[0], stride), np.int32), np.zeros((C.shape[0], stride), C.data.dtype)
    mask = np.arange(stride)[None, :] < cnt[:, None]
    cols[mask], vals[mask] = C.indices, C.data
    return cols, vals, cnt


def same(a, b):
    """two fixed-stride results: counts, and columns and BITS of the values up to the counts"""
    if a[0].shape != b[0].shape or not np.array_equal(a[2], b[2]):
        return False
    mask = np.arange(a[0].shape[1])[None, :] < a[2][:, None]
    return np.array_equal(a[0][mask], b[0][mask]) and a[1][mask].tobytes() == b[1][mask].tobytes()


# ---------------------------------------------------------------------------------------------- the kernels' rule, restated
def _ties(a, b, flaw=None):
    if flaw == "ulp-merged":
        return a == b or np.nextafter(a, b) == b
    return a == b


def is_queued(L, c, v, S, flaw=None):
    """expand_simple_kernel's rule: it walks the row's groups while fewer than S columns are out, and hands the row to
    expand_merge_kernel at the first group of SEVERAL members whose score equals the previous or the next group's."""
    if flaw == "no-merge":
        return False
    out, m = 0, len(c)
    for e in range(m):
        if out >= S:
            break
        size = int(L.size[c[e]])
        before = e > 0 and _ties(v[e - 1], v[e], flaw) and not (flaw == "tie-before-single-unseen" and L.size[c[e - 1]] == 1)
        after = e + 1 < (m - 1 if flaw == "tie-at-last-unseen" else m) and _ties(v[e + 1], v[e], flaw)
        if size != 1 and (before or after):
            return True
        out += min(size, S - out)
    return False


def expand_row(L, c, v, S, flaw=None):
    """One row as the two kernels write it (``flaw``: with one wrong turn): kept rows group after group, queued rows run by
    run, a run's members merged by column."""
    if flaw == "stride-cut-at-groups":
        S = min(S, L.n_groups)
    lists = [L.rows_of(g) for g in c]
    if flaw == "last-member-dropped":
        lists = [x[:-1] if len(x) > 1 else x for x in lists]
    oc, ov, m = [], [], len(c)
    if not is_queued(L, c, v, S, flaw):
        for e in range(m):
            oc += list(lists[e])
            ov += [v[e]] * len(lists[e])
        return np.array(oc[:S], np.int64), np.array(ov[:S], v.dtype)
    e0 = 0
    while e0 < m and len(oc) < S:
        e1 = e0 + 1
        while e1 < m and _ties(v[e1], v[e0], flaw):
            e1 += 1
        run = list(range(e0, e1))
        if flaw == "run-stops-at-64":
            run = run[:LANES]
        if flaw == "skips-the-64th" and len(run) >= LANES:
            del run[LANES - 1]
        parts = [lists[e] for e in run]
        if flaw == "cut-per-group":          # the columns still wanted are dealt to the groups in their order, then merged
            left, cut = S - len(oc), []
            for x in parts:
                cut.append(x[:left])
                left -= len(cut[-1])
            parts = cut
        cols = np.concatenate(parts) if parts else np.array([], np.int64)
        if not (flaw == "ties-by-group" or (flaw == "only-short-runs-merged" and e1 - e0 > LANES)):
            cols = np.sort(cols)
        oc += list(cols)
        ov += [v[0] if flaw == "score-from-first-entry" else v[e0]] * len(cols)
        e0 = e1
    return np.array(oc[:S], np.int64), np.array(ov[:S], v.dtype)


# name: what the wrong turn is.  Each is a turn in the model of the two kernels above.
FLAWS = {
    "no-merge": "no row is queued: the groups are written in their order, ties not merged by column",
    "ties-by-group": "a queued row's ties are ordered by group, then column, not by column",
    "run-stops-at-64": "the groups of a run beyond the 64th are ignored",
    "skips-the-64th": "the 64th group of a run is ignored",
    "only-short-runs-merged": "runs of more than 64 groups are written in group order",
    "cut-per-group": "the cut is applied group by group before the merge",
    "last-member-dropped": "every group of several members loses its last member",
    "ulp-merged": "groups one ulp apart are taken for a tie",
    "score-from-first-entry": "a run's score is read from the row's first entry",
    "tie-before-single-unseen": "a tie with a preceding group of one member does not queue the row",
    "tie-at-last-unseen": "a tie with the row's last entry does not queue the row",
    "stride-cut-at-groups": "the output's stride is cut at the number of groups of the index",
    "range-from-lo": "a share's every world-th position is counted from pos_lo, not from pos_hi - 1",
}
# A wrong turn that CANNOT change an answer on rows the multiply leaves, and why -- the CPU test asserts that it changes
# none: groups are numbered by ascending lowest member, and equal scores are ordered by group.  A group of one member that
# PRECEDES a tying group g therefore has a lower number than g, its one row is lower than g's lowest, and -- if g ties with
# nothing behind it -- writing the groups in their order IS the merge by column.  (Rows in which an earlier group of several
# members ties are queued by that group's look at its successor.)  The clause is in the kernel; it decides no output.
HARMLESS = {"tie-before-single-unseen"}
# ``no-merge`` and ``ties-by-group`` are different turns (one in expand_simple_kernel's rule, one in expand_merge_kernel's
# comparison) with the same outcome on rows sorted (score, group): both are listed, both must be caught.


def wrong_expand(L, rows, cols, vals, counts, stride, flaw, left=False, cache=None):
    """``ref_expand``'s arguments, through ``expand_row`` with (or, ``flaw`` None, without) one wrong turn."""
    rows = np.arange(cols.shape[0] if left else L.n) if rows is None else np.asarray(rows, np.int64)
    S = min(stride, L.n_groups) if flaw == "stride-cut-at-groups" else stride
    out_c, out_v = np.zeros((len(rows), S), np.int32), np.zeros((len(rows), S), vals.dtype)
    out_n = np.zeros(len(rows), np.int32)
    cache = {} if cache is None else cache
    for k, r in enumerate(rows if left else L.gid[rows]):
        c, v = cols[r, :counts[r]], vals[r, :counts[r]]
        key = (c.tobytes(), v.tobytes(), stride, flaw)
        if key not in cache:
            cache[key] = expand_row(L, c, v, stride, flaw)
        oc, ov = cache[key]
        out_c[k, :len(oc)], out_v[k, :len(oc)], out_n[k] = oc, ov, len(oc)
    return out_c, out_v, out_n


# ---------------------------------------------------------------------------------------------- census
def edges_of(L, c, v, S):
    """What one row over groups reaches, counted from the row, the group sizes and the member lists alone."""
    t, m = L.t, len(c)
    size = L.size[c] if m else np.array([], np.int64)
    found = {"queued" if is_queued(L, c, v, S) else "kept", f"count-{m}" if m == 0 else "count>0"}
    assert not np.signbit(v[v == 0]).any(), "-0.0 is outside the expansion's contract"
    if m == S:
        found.add("count==S")
    total = int(size.sum())
    if m == 1:
        z = int(size[0])
        found |= {"one-single"} if z == 1 else set()
        found.add("one-group<S" if z < S else "one-group==S" if z == S else "one-group==S+1" if z == S + 1 else
                  "one-group>>S" if z >= 5 * S else "one-group>S")
    bounds = [0] + [e for e in range(1, m) if v[e] != v[e - 1]] + [m] if m else [0]
    runs = list(zip(bounds[:-1], bounds[1:]))
    if m and all(b - a == 1 for a, b in runs) and (size > 1).all():
        found.add("distinct-total<S" if total < S else "distinct-total==S" if total == S else "distinct-cut")
    cum = np.concatenate([[0], np.cumsum(size)])
    hub, alt = int(L.group_of_type[t["h1000"]]), {int(L.group_of_type[t["alt_a"]]), int(L.group_of_type[t["alt_b"]])}
    prev_len = None
    for a, b in runs:
        R, at, mem = b - a, int(cum[a]), int(cum[b] - cum[a])
        merge = R >= 2 and (size[a:b] > 1).any()
        if at >= S:
            if merge:
                found.add("cut-before-run")
            continue
        kind = "run" if merge else "singles-run" if R >= 2 else "group"
        if at + mem > S:
            found.add(f"cut-inside-{kind}")
        elif at + mem == S and b < m:
            found.add(f"cut-at-{kind}-end")
        if kind == "singles-run":
            found |= {"singles-run"} | ({"singles-run>64"} if R > LANES else set())
        if not merge:
            prev_len = None
            continue
        found |= {f"run-{R}", "run<=64" if R <= LANES else "run>64"}
        found |= ({"run-front", "tie-at-entry-0"} if a == 0 else set()) | ({"run-behind-one"} if a == 1 else set())
        found |= {"run-last", "tie-at-last-entry"} if b == m else {"run-then-lower"}
        if prev_len is not None:
            found |= ({"short-then-long"} if prev_len <= LANES < R else set()) | ({"long-then-short"} if R <= LANES < prev_len else set())
        prev_len = R
        groups = [int(g) for g in c[a:b]]
        found |= ({"hub-in-run"} if hub in groups else set()) | ({"alternating-in-run"} if alt <= set(groups) else set())
        if R == 2 and size[a] == 1:
            found.add("ties-with-single-before-only")
        if R == 2 and size[b - 1] == 1:
            found.add("ties-with-single-after-only")
        found |= ({"negative-run"} if v[a] < 0 else set()) | ({"zero-run"} if v[a] == 0 else set())
        written = np.sort(np.concatenate([L.rows_of(g) for g in groups]))[:S - at]
        for g in groups:                 # a group all of whose members are out while the run goes on
            rows = L.rows_of(g)
            if len(written) and rows[-1] < written[-1] and len(rows) > 1:
                found.add("group-runs-out" if R <= LANES else "long-run-group-below-last")
    for e in range(m - 1):
        if size[e] > 1 and size[e + 1] > 1 and v[e + 1] == np.nextafter(v[e], v.dtype.type(-1)):
            found.add("ulp-neighbours")
    return found


def required(L, S):
    """The edges a result of stride S can hold (a row has at most S groups), from S and the layout's group sizes alone."""
    sizes = set(int(z) for z in L.size)
    req = {"count-0", "one-single", "count==S", "one-group>>S", "kept", "cut-inside-group", "distinct-cut"}
    req |= ({"one-group<S"} if S > 1 else set()) | ({"one-group==S"} if S in sizes else set()) | ({"one-group==S+1"} if S + 1 in sizes else set())
    if S >= 2:
        req |= {"queued", "singles-run", "run<=64", "run-front", "tie-at-entry-0", "run-last", "tie-at-last-entry", "cut-inside-run",
                "hub-in-run", "alternating-in-run", "ties-with-single-before-only", "ties-with-single-after-only", "zero-run",
                "negative-run", "ulp-neighbours", "distinct-total==S", "cut-at-group-end"}
        req |= {f"run-{R}" for R in RUNS + (S,) if R <= S}
    if S >= 3:
        req |= {"run-behind-one", "run-then-lower", "distinct-total<S"}
    if S >= 10:
        req |= {"cut-at-run-end", "cut-before-run"}
    if S >= 64:
        req.add("group-runs-out")
    if S >= 65:
        req |= {"run>64", "long-run-group-below-last"}
    if S >= 70:
        req |= {"singles-run>64", "short-then-long", "long-then-short"}
    return req


def census(cs):
    """What a case reaches: per kind its edges, the queued and the kept output rows, the lengths of the tying runs, the queued
    rows of every call -- and the assertion that every edge the stride can hold is there."""
    L, S = cs.L, cs.S
    per_kind = {name: edges_of(L, c, v, S) for name, (c, v) in zip(cs.names, cs.rows)}
    found = set().union(*per_kind.values())
    missing = required(L, S) - found
    assert not missing, f"stride {S}: the rows do not reach {sorted(missing)}"
    for cls in (1, 2, 3):
        dealt = set(cs.kind_of_group[L.size == cls])
        assert dealt == set(range(len(cs.kinds))), f"stride {S}: kinds {sorted(set(range(len(cs.kinds))) - dealt)} reach no group of {cls}"
    queued = {which: cs.n_queued(which) for which in cs.row_lists}
    assert queued["none-queued"] == 0 and len(cs.row_lists["none-queued"]) > 0
    if S >= 2:
        assert queued["all"] > MERGE_BLOCKS, f"stride {S}: {queued['all']} queued rows do not outnumber the merge kernel's workgroups"
        assert queued["single"] == 1
    return {"edges": found, "per_kind": per_kind, "queued_rows": queued, "kept_rows": L.n - queued["all"],
            "run_lengths": sorted(int(e[4:]) for e in found if e.startswith("run-") and e[4:].isdigit())}


# ---------------------------------------------------------------------------------------------- one-sided products
def left_matrix(dtype):
    """(matrix, row names): one left row ``{column of group g: w}`` per kind of every stride whose scores are positive --
    against the layout it scores exactly the kind's row over groups.  Squared row norms stay below 1."""
    dtype = np.dtype(dtype).type
    L = layout(dtype)
    names, indptr, indices, data, seen = [], [0], [], [], set()
    for S in STRIDES:
        for name, segs in kinds(L, S, dtype):
            types = [x for _, ts in segs for x in ts]
            w = [s for s, ts in segs for _ in ts]
            key = (tuple(types), tuple(w))
            if not types or min(w) <= 0 or key in seen:
                continue
            seen.add(key)
            order = np.argsort(types)
            indices += list(np.array(types)[order])
            data += list(np.array(w, dtype)[order])
            indptr.append(len(indices))
            names.append(f"{name}@{S}")
    A = sp.csr_matrix((np.array(data, dtype), np.array(indices, np.int32), np.array(indptr, np.int64)), shape=(len(names), L.A.shape[1]))
    assert (np.add.reduceat(A.data.astype(np.float64) ** 2, A.indptr[:-1]) <= 1.0).all()
    return A, names


def repeated(A, names):
    """every left row 1, 2 or 5 times, shuffled (SG_COLLAPSE_LEFT=1 groups them again)"""
    which = np.repeat(np.arange(A.shape[0]), np.resize([1, 2, 5], A.shape[0]))
    which = which[np.random.default_rng(5).permutation(len(which))]
    return A[which], [names[i] for i in which]
