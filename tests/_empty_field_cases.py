"""What sg_topn_rescore with skip_empty (csrc/sg_rescore.hip) is held to, for the CPU and the GPU tests alike.  TEST INFRASTRUCTURE ONLY.

- ``ref_rescore_skip_empty``: the statement of include/sg_hip.h in numpy, built on ``candidate_scores`` / ``refused`` of
  tests/_floor_cases.py -- which fields are empty for a pair (``indptr[a + 1] == indptr[a]`` of the PHYSICAL rows of either
  side), ``c``, ``wp`` and ``wt`` as ``acc = acc + ...`` on arrays of the value type, ``(c * wt) / wp`` as numpy divides (one
  correctly rounded division), floors held on the fields that are not empty, ``>``, the stable sort, the cut;
- its ``variant``s (``WRONG``): the turns a kernel could take instead, each of which must change an answer on some case;
- ``cases(dtype)``: ``{name: (Case, primary, floors)}`` -- ``primary`` a ``Field`` (field 0's matrices and dead lists; its weight
  is not read) or None, ``floors`` a list or None; ``census`` says which edges they hold."""
import functools

import numpy as np

from tests import _floor_cases as FC
from tests import _rescore_cases as C
from tests._pair_cases import csr_of

ROW_CHUNK = FC.ROW_CHUNK
WRONG = ("as_zero", "divide_always", "divide_then_multiply", "reciprocal", "wp_descending", "left_only", "right_only",
         "live_row_for_physical", "primary_never_empty", "zero_entry_is_empty", "floor_held_on_empty",
         "threshold_before_rescale", "bit63_lost", "mask_carried", "all_empty_as_zero")


# ------------------------------------------------------------------------------------------ the statement
_SCORES = {}


def candidate_scores(case):
    """``_floor_cases.candidate_scores``, once a case (the field scores are the slow part of every reference here)."""
    if id(case) not in _SCORES:
        _SCORES[id(case)] = (case, FC.candidate_scores(case))
    return _SCORES[id(case)][1]


def _row_is_empty(m, phys, variant):
    phys = np.minimum(phys, m.shape[0] - 1)                 # (a wrong turn may step outside: it reads the last row then)
    nnz = np.diff(m.indptr)[phys]
    if variant == "zero_entry_is_empty":
        absum = np.add.reduceat(np.r_[np.abs(m.data), 0], np.minimum(m.indptr[:-1], len(m.data)))
        absum = np.where(np.diff(m.indptr) == 0, 0, absum)
        return (nnz == 0) | (absum[phys] == 0)
    return nnz == 0


def empty_sides(case, primary, variant=None):
    """(left[f][p], right[f][p]) for f = 0 .. F and every counted candidate p: has the physical row of that side no entries?"""
    rows, ent, j, _ = candidate_scores(case)
    left, right = [], []
    for k, fld in enumerate([primary] + list(case.fields)):
        if fld is None or (k == 0 and variant == "primary_never_empty"):
            left.append(np.zeros(len(rows), bool)), right.append(np.zeros(len(rows), bool))
            continue
        if variant == "live_row_for_physical":
            a, b = rows, j
        else:
            a, b = C.physical(fld.dead_a, rows), C.physical(fld.dead_b, j)
        left.append(_row_is_empty(fld.A, a, variant)), right.append(_row_is_empty(fld.B, b, variant))
    return left, right


def empty_for_pair(case, primary, variant=None):
    """E[f][p]: is field f empty for candidate p?  (With the turns a mask of the kernel's could take.)"""
    rows, ent, j, _ = candidate_scores(case)
    left, right = empty_sides(case, primary, variant)
    out = []
    for le, ri in zip(left, right):
        ri = ri & ~le                                       # (what the kernel notes per candidate: the right side alone)
        if variant == "bit63_lost":
            ri = ri & (ent % ROW_CHUNK != ROW_CHUNK - 1)
        if variant == "mask_carried":                       # (rows are contiguous: entry e - 64 of the row lies 64 places back)
            ri = ri.copy()
            for p in np.flatnonzero(ent >= ROW_CHUNK):
                ri[p] |= ri[p - ROW_CHUNK]
        if variant == "left_only":
            out.append(le)
        elif variant == "right_only":
            out.append(ri)
        elif variant == "as_zero":
            out.append(np.zeros(len(rows), bool))
        else:
            out.append(le | ri)
    return out


def similarity(scores, W, E, T, variant=None):
    """(c, similarity) of every candidate: the three sums in ascending field order, then the one division."""
    n = len(scores[0])
    with np.errstate(all="ignore"):
        c, wp, wt = np.zeros(n, T), np.zeros(n, T), np.zeros(n, T)
        for f in range(len(W)):
            c = np.where(E[f], c, c + W[f] * scores[f]).astype(T)
            wt = wt + W[f]
        for f in (reversed(range(len(W))) if variant == "wp_descending" else range(len(W))):
            wp = np.where(E[f], wp, wp + W[f]).astype(T)
        assert c.dtype == T and wp.dtype == T and wt.dtype == T
        some = np.zeros(n, bool)
        for e in E:
            some |= e
        if variant == "divide_then_multiply":
            scaled = (c / wp) * wt
        elif variant == "reciprocal":
            scaled = c * (wt / wp)
        else:
            scaled = (c * wt) / wp
        assert scaled.dtype == T
        dropped = T(0) if variant == "all_empty_as_zero" else T(np.nan)
        scaled = np.where(wp > 0, scaled, dropped).astype(T)
        if variant == "divide_always":
            return c, scaled
        return c, np.where(some, scaled, c).astype(T)


def ref_rescore_skip_empty(case, primary, floors, variant=None):
    """(cols[R, min(k, S)], vals, counts) of the statement -- or of one wrong turn."""
    T = case.vals.dtype.type
    R, S = case.cols.shape
    So = min(case.top_n, S)
    rows, ent, j, scores = candidate_scores(case)
    W = [T(case.w0)] + [T(f.w) for f in case.fields]
    E = empty_for_pair(case, primary, variant)
    floors = [None] * len(W) if floors is None else list(floors)
    failed = np.zeros(len(rows), bool)
    with np.errstate(all="ignore"):
        for f, m in enumerate(floors):
            if m is not None:
                below = ~(scores[f] > T(m))
                failed |= below if variant == "floor_held_on_empty" else below & ~E[f]
        c, sim = similarity(scores, W, E, T, variant)
        above = (c > T(case.threshold)) if variant == "threshold_before_rescale" else (sim > T(case.threshold))
        above &= ~np.isnan(sim)
    keep = above & ~failed
    out_c, out_v, out_n = np.zeros((R, So), np.int32), np.zeros((R, So), T), np.zeros(R, np.int32)
    start = np.r_[0, np.cumsum(case.counts)]
    for r in range(R):
        sel = np.arange(start[r], start[r + 1])
        sel = sel[keep[sel]]
        order = sel[np.lexsort((j[sel], -sim[sel]))][:So]
        out_n[r] = len(order)
        out_c[r, :len(order)], out_v[r, :len(order)] = j[order], sim[order]
    return out_c, out_v, out_n


# ------------------------------------------------------------------------------------------ building blocks
def blank_field(n_left, table, dtype, w, left_blank=(), right_blank=(), right_zero=(), dead_a=None, dead_b=None,
                dead_blank_a=(), dead_blank_b=()):
    """``table_field`` with blanks: live left row i is {column 0: 1 + i / 16} or has no entries (``left_blank``), live right
    row j is {column 0: table[j]}, has no entries (``right_blank``) or holds a STORED 0.0 (``right_zero``: not empty).  A dead
    physical row holds POISON -- a wrong row map shows in the score -- or, named in ``dead_blank_*`` by its physical number, no
    entries: a wrong row map shows in what is empty."""
    def phys(values, blank, zero, dead, dead_blank):
        dead = np.zeros(0, np.int64) if dead is None else np.asarray(dead, np.int64)
        n = len(values) + len(dead)
        live_at = np.delete(np.arange(n), dead)
        rows = [([0], [C.POISON]) for _ in range(n)]
        for q in dead_blank:
            assert q in dead
            rows[q] = ([], [])
        for i, at in enumerate(live_at):
            rows[at] = ([], []) if i in blank else ([0], [0.0 if i in zero else values[i]])
        return csr_of(rows, dtype, 4)
    left = (1 + np.arange(n_left) / 16).astype(dtype)
    return C.Field(phys(left, set(left_blank), (), dead_a, dead_blank_a),
                   phys(np.asarray(table, dtype), set(right_blank), set(right_zero), dead_b, dead_blank_b), w,
                   None if dead_a is None else np.asarray(dead_a, np.int64), None if dead_b is None else np.asarray(dead_b, np.int64))


def _some(rng, n, share):
    return set(int(x) for x in np.flatnonzero(rng.uniform(0, 1, n) < share))


def _frozen(case):
    for arr in (case.cols, case.vals, case.counts):
        arr.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def cases(dtype):
    dtype = np.dtype(dtype).type
    T = dtype
    rng = np.random.default_rng(8200 + np.dtype(dtype).itemsize)
    eps = np.finfo(dtype).eps
    out = {}
    w3 = (0.5, 0.3, 0.2)

    def table(n):
        return rng.uniform(0.3, 1.0, n)

    # ---- short rows (1, 7 and 8 candidates), a long one (129) and one in between (65): both select kernels in one call.  Of the
    # long row the entries 0, 63 and 64 have an empty field -- the first bit, the top bit, the next group's first -- and no other
    n_cols = 300
    rows = [(c + 150, v) for c, v in C._random_rows(rng, [0, 1, 7, 8, 65, 3], 150, dtype)]    # (the long row's columns: its own)
    rows.insert(4, C._random_rows(rng, [129], 150, dtype)[0])
    long_cols = rows[4][0]
    blank1 = {int(long_cols[0]), int(long_cols[64])} | {int(rows[r][0][0]) for r in (1, 2, 3)}
    blank2 = {int(long_cols[63])} | {int(c) for c in rows[5][0][::7]}
    assert not (blank1 | blank2) & {int(long_cols[e]) for e in (1, 62, 65, 127)}
    f1 = blank_field(7, table(n_cols), dtype, w3[1], right_blank=blank1)
    f2 = blank_field(7, table(n_cols), dtype, w3[2], right_blank=blank2, left_blank={6})   # (row 6: empty on the left only)
    prim = blank_field(7, table(n_cols), dtype, 1.0)
    mixed = _frozen(C.Case(*C.make_cand(rows, 129, dtype, n_cols), n_cols, w3[0], [f1, f2], -1.0, 129))
    out["mask_bits"] = (mixed, prim, None)
    out["mask_bits:primary_null"] = (mixed, None, None)
    out["mask_bits:cut"] = (mixed._replace(threshold=0.6, top_n=5), prim, None)
    # ---- the sides: empty on the left only (the whole row skips the field), on the right only, on both; field 0 through the
    # primary, and without one; pairs all of whose fields are empty (threshold -1: only the NaN drops them)
    R, N = 12, 40
    rows = C._random_rows(rng, [6] * R, N, dtype)
    left1, right1 = {2, 5}, _some(rng, N, 0.3)
    left2, right2 = {5, 7}, _some(rng, N, 0.3)
    left0, right0 = {5, 9}, _some(rng, N, 0.3)
    right0 |= {int(rows[2][0][0])}
    right1 |= {int(rows[2][0][0]), int(rows[7][0][1])}
    right2 |= {int(rows[2][0][0]), int(rows[2][0][1])}                    # (2, its first column): every field empty; so is row 5
    f1 = blank_field(R, table(N), dtype, w3[1], left_blank=left1, right_blank=right1)
    f2 = blank_field(R, table(N), dtype, w3[2], left_blank=left2, right_blank=right2)
    prim = blank_field(R, table(N), dtype, 1.0, left_blank=left0, right_blank=right0)
    sides = _frozen(C.Case(*C.make_cand(rows, 6, dtype, N), N, w3[0], [f1, f2], -1.0, 6))
    out["sides"] = (sides, prim, None)
    out["sides:primary_null"] = (sides, None, None)
    out["sides:threshold"] = (sides._replace(threshold=0.55, top_n=3), prim, None)
    # a floor on an empty field is not held, on a field of the same pair that is not empty it is; the primary's floor likewise
    _, _, _, s = candidate_scores(sides)
    out["sides:floor_last"] = (sides, prim, [None, None, FC._present(s[2][s[2] > 0], 0.4)])
    out["sides:floor_first_and_last"] = (sides, prim, [None, FC._present(s[1][s[1] > 0], 0.3), FC._present(s[2][s[2] > 0], 0.3)])
    out["sides:floor_primary"] = (sides, prim, [FC._present(s[0], 0.5), None, None])
    out["sides:floor_all"] = (sides._replace(top_n=2), prim, [FC._present(s[0], 0.2), 0.35, 0.35])
    # ---- one further field, and seven with every set of them empty (bit f of the column says whether field f + 1 is), at
    # weights that are no binary fractions: wt != 1 in T, and the order of wp's adds shows
    f1 = blank_field(4, table(30), dtype, 0.5, right_blank=_some(rng, 30, 0.4), left_blank={3})
    one = _frozen(C.Case(*C.make_cand(C._random_rows(rng, [9, 9, 4, 9], 30, dtype), 9, dtype, 30), 30, 0.5, [f1], 0.4, 9))
    out["one_field"] = (one, blank_field(4, table(30), dtype, 1.0, right_blank=_some(rng, 30, 0.3)), None)
    for name, w in (("tenth", 0.1), ("third", 1 / 3)):
        weights = ((1.0 - 7 * w) if name == "tenth" else w,) + (w,) * 7
        N7 = 256
        rows = C._random_rows(rng, [40, 40, 40, 64, 8], N7, dtype)
        fields = [blank_field(5, table(N7), dtype, weights[f + 1], right_blank={j for j in range(N7) if (j >> f) & 1},
                              left_blank={4} if f == 6 else ()) for f in range(7)]
        seven = _frozen(C.Case(*C.make_cand(rows, 64, dtype, N7), N7, weights[0], fields, 0.2, 64))
        prim = blank_field(5, table(N7), dtype, 1.0, right_blank={j for j in range(N7) if j >= 128})
        out[f"weights_{name}_7"] = (seven, prim, None)
        _, _, _, s = candidate_scores(seven)
        out[f"weights_{name}_7:floors"] = (seven, prim, [None if f % 2 else FC._present(x[x > 0], 0.3) for f, x in enumerate(s)])
    # ---- dead lists that differ between the sides and the fields: the physical row next to an empty one holds entries, a dead
    # physical row is empty where its live neighbours are not
    R, N = 12, 40
    rows = C._random_rows(rng, [6] * R, N, dtype)
    f1 = blank_field(R, table(N), dtype, w3[1], left_blank={1, 4, 8}, right_blank=_some(rng, N, 0.35), dead_a=[2, 3, 9],
                     dead_b=[0, 17, 18, 41], dead_blank_a=[3], dead_blank_b=[17, 41])
    f2 = blank_field(R, table(N), dtype, w3[2], right_blank=_some(rng, N, 0.35), dead_b=[5, 6, 7], dead_blank_b=[6])
    prim = blank_field(R, table(N), dtype, 1.0, left_blank={0, 10}, right_blank=_some(rng, N, 0.25), dead_a=[0, 1],
                       dead_b=[39, 40], dead_blank_b=[39])
    dead = _frozen(C.Case(*C.make_cand(rows, 6, dtype, N), N, w3[0], [f1, f2], 0.3, 4))
    out["dead_sides_and_fields_differ"] = (dead, prim, None)
    out["dead_sides_and_fields_differ:floor"] = (dead, prim, [None, 0.4, None])
    # the same handle on both sides with its dead list on both: a self-join of a corpus with removed rows pending
    n_live, dl = 20, np.array([0, 4, 5, 11, 22])
    blank = {3, 4, 10, 19}
    f = blank_field(n_live, table(n_live), dtype, 0.5, right_blank=blank, dead_b=dl, dead_blank_b=[4, 22])
    g = blank_field(n_live, table(n_live), dtype, 1.0, right_blank={1, 3}, dead_b=dl)
    rows = C._random_rows(rng, [5] * n_live, n_live, dtype)
    out["dead_same_handle"] = (_frozen(C.Case(*C.make_cand(rows, 5, dtype, n_live), n_live, 0.5, [C.Field(f.B, f.B, 0.5, dl, dl)],
                                              0.3, 3)), C.Field(g.B, g.B, 1.0, dl, dl), None)
    # ---- a row that holds only a stored 0.0 is NOT empty: its 0 enters with the full weight
    zero = {1, 3, 5}
    f1 = blank_field(2, table(8), dtype, w3[1], right_zero=zero)
    f2 = blank_field(2, table(8), dtype, w3[2], right_blank={3, 4})
    rows = [(np.arange(8), np.linspace(1, 0.6, 8).astype(dtype))] * 2
    out["stored_zero"] = (_frozen(C.Case(*C.make_cand(rows, 8, dtype, 8), 8, w3[0], [f1, f2], 0.45, 8)), None, None)
    # ---- exact binary fractions: field 2 is empty, wp = 0.75, wt = 1, and (c * wt) / wp lies AT the threshold 0.5, one ulp
    # above and one ulp below it (c = 0.375, 0.375 + eps / 4, 0.375 - eps / 4: all under the threshold before the rescale);
    # column 3 has no empty field and the same c
    s0 = np.full(5, 0.5, dtype)
    t1 = np.array([0.5, 0.5 + eps, 0.5 - eps, 0.5, 1.0], dtype)
    f1 = C.table_field(1, t1, dtype, 0.25)
    f2 = blank_field(1, np.full(5, 0.75), dtype, 0.25, right_blank={0, 1, 2, 4})
    out["threshold_exact"] = (_frozen(C.Case(*C.make_cand([(np.arange(5), s0)], 5, dtype, 5), 5, 0.5, [f1, f2], 0.5, 5)), None, None)
    # ---- blocks of equal rescaled scores over the ranks k - 2 .. k + 2 whose candidate order and column order disagree
    for k in (1, 10, 65):
        lead, block, tail = max(k - 2, 0), 5, 3
        m = lead + block + tail
        s0 = (1.0 - np.arange(m) / 256).astype(dtype)
        cols = np.arange(m)
        cols[lead:lead + block] = cols[lead:lead + block][::-1]
        lift = np.zeros(m)
        lift[lead:lead + block] = np.arange(block) / 128             # 0.5 * (-q / 256) + 0.25 * (q / 128) = 0
        tab = np.zeros(m)
        tab[cols] = lift
        f1 = C.table_field(1, tab, dtype, 0.25)
        f2 = blank_field(1, np.ones(m), dtype, 0.25, right_blank=set(range(m)))
        out[f"ties_k{k}"] = (_frozen(C.Case(*C.make_cand([(cols, s0)], m, dtype, m), m, 0.5, [f1, f2], 0.0, k)), None, None)
    # ---- no empty row anywhere: the bits of the call without the option (2 048 entries a row and many long rows: one each)
    base = C.cases(dtype)
    for name in ("counts_short", "counts_long", "weights_third_7", "dead_sides_and_fields_differ", "full_2048_top20",
                 "many_long_rows", "nan_inf", "zeros"):
        out[f"no_blank:{name}"] = (base[name], None, None)
    fl = FC.floor_cases(dtype)
    for name in ("counts_long:all", "weights_tenth_7:mixed", "mask_bits:primary"):
        out[f"no_blank:{name}"] = (fl[name][0], None, fl[name][1])
    return out


@functools.lru_cache(maxsize=None)
def expected(dtype, name):
    """The statement on a case, computed once."""
    want = ref_rescore_skip_empty(*cases(dtype)[name])
    for a in want:
        a.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def expected_without(dtype, name):
    """What the call WITHOUT the option gives on the case (``ref_rescore`` / ``ref_rescore_floors``), computed once."""
    case, _, floors = cases(dtype)[name]
    if name.startswith("no_blank:"):                        # (shared with the tests without the option)
        return C.expected(dtype, name.split(":", 1)[1]) if floors is None else FC.expected(dtype, name.split(":", 1)[1])
    want = C.ref_rescore(case) if floors is None else FC.ref_rescore_floors(case, floors)
    for a in want:
        a.setflags(write=False)
    return want


# ------------------------------------------------------------------------------------------ what the cases hold
EDGES = {"short_rows_1_7_8", "long_row_bits_0_63_64", "long_row_clear_1_62_65_127", "both_select_kernels", "left_only",
         "right_only", "both_sides", "primary_empty", "primary_null", "every_field_empty", "one_further_field",
         "two_further_fields", "seven_further_fields", "one_of_seven_empty", "all_seven_empty", "weights_5_3_2",
         "wt_not_one", "dead_moves_an_empty_row", "stored_zero_row", "at_the_threshold", "ulp_above_the_threshold",
         "ulp_below_the_threshold", "ties_across_the_cut", "floor_on_an_empty_field_not_held", "floor_held_on_the_same_pair",
         "primary_floor_on_an_empty_primary", "rescale_lifts_over_the_threshold", "the_cut_moves", "no_empty_row"}


def census(dtype):
    """The edges the cases are built for, as flags, found in the cases themselves."""
    dtype = np.dtype(dtype).type
    T = dtype
    flags = set()
    for name, (case, primary, floors) in cases(dtype).items():
        rows, ent, j, scores = candidate_scores(case)
        F = len(case.fields)
        W = [T(case.w0)] + [T(f.w) for f in case.fields]
        left, right = empty_sides(case, primary)
        E = empty_for_pair(case, primary)
        some = np.logical_or.reduce(E)
        every = np.logical_and.reduce(E)
        n_empty = np.sum(E, axis=0)
        c, sim = similarity(scores, W, E, T)
        t = T(case.threshold)
        cnt = case.counts[rows]
        want, plain = expected(dtype, name), expected_without(dtype, name)
        if not some.any() and not any(np.any(le | ri) for le, ri in zip(left, right)):
            flags.add("no_empty_row")
            assert C.same_result(want, plain), name
            continue
        if {1, 7, 8} <= set(int(x) for x in case.counts) and some[np.isin(cnt, (1, 7, 8))].any():
            flags.add("short_rows_1_7_8")
        long = cnt == 129
        if long.any():
            if set(int(e) for e in ent[long & some]) == {0, 63, 64}:
                flags |= {"long_row_bits_0_63_64", "long_row_clear_1_62_65_127"}
            if (some & (cnt <= ROW_CHUNK)).any():
                flags.add("both_select_kernels")
        for f in range(F + 1):
            if (left[f] & ~right[f]).any():
                flags.add("left_only")
            if (~left[f] & right[f]).any():
                flags.add("right_only")
            if (left[f] & right[f]).any():
                flags.add("both_sides")
        if primary is None:
            flags.add("primary_null")
        elif E[0].any():
            flags.add("primary_empty")
        if every.any():
            flags.add("every_field_empty")
        flags.add({1: "one_further_field", 2: "two_further_fields", 7: "seven_further_fields"}.get(F, "other"))
        if F == 7 and ((n_empty == 1) & ~E[0]).any():
            flags.add("one_of_seven_empty")
        if F == 7 and np.logical_and.reduce(E[1:]).any():
            flags.add("all_seven_empty")
        if [float(w) for w in W] == [float(T(x)) for x in (0.5, 0.3, 0.2)]:
            flags.add("weights_5_3_2")
        wt = T(0)
        for w in W:
            wt = T(wt + w)
        if wt != 1:
            flags.add("wt_not_one")
        for fld in [primary] + list(case.fields):
            if fld is None:
                continue
            for m, dead in ((fld.A, fld.dead_a), (fld.B, fld.dead_b)):
                nnz = np.diff(m.indptr)
                for d in ([] if dead is None else dead):
                    for q in (d - 1, d + 1):
                        if 0 <= q < len(nnz) and (nnz[q] == 0) != (nnz[d] == 0):
                            flags.add("dead_moves_an_empty_row")
            if (np.diff(fld.B.indptr) == 1).any() and (fld.B.data == 0).any():
                flags.add("stored_zero_row")
        with np.errstate(all="ignore"):
            if (some & (sim == t)).any():
                flags.add("at_the_threshold")
            if (some & (sim == np.nextafter(t, T(np.inf)))).any():
                flags.add("ulp_above_the_threshold")
            if (some & (sim == np.nextafter(t, T(-np.inf)))).any():
                flags.add("ulp_below_the_threshold")
            if (some & (sim > t) & ~(c > t)).any():
                flags.add("rescale_lifts_over_the_threshold")
        for r in range(case.cols.shape[0]):
            k = want[2][r]
            vals = sim[(rows == r) & some]
            if k == case.top_n and k and (vals == want[1][r, k - 1]).sum() > 1 and k < (rows == r).sum():
                flags.add("ties_across_the_cut")
            before, after = set(plain[0][r, :plain[2][r]]), set(want[0][r, :want[2][r]])
            if after - before and before - after:
                flags.add("the_cut_moves")
        if floors is not None:
            with np.errstate(all="ignore"):
                for f, m in enumerate(floors):
                    if m is None:
                        continue
                    below = ~(scores[f] > T(m))
                    if (E[f] & below & (sim > t)).any():
                        flags.add("floor_on_an_empty_field_not_held")
                        if f == 0:
                            flags.add("primary_floor_on_an_empty_primary")
                    if (some & ~E[f] & below & (sim > t)).any():
                        flags.add("floor_held_on_the_same_pair")
    return flags
