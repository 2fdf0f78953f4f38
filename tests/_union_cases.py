"""What sg_topn_union (csrc/sg_union.hip) is held to, for the CPU and the GPU tests alike.  TEST INFRASTRUCTURE ONLY.

- ``ref_union``: the statement of include/sg_hip.h in numpy -- the distinct columns a row's parts name, ascending; part 0's bits
  for the columns part 0 holds, the primary field's score for the others, by ``ref_rescore``'s own restatement of the pair score
  (``physical`` and ``ref_pairs_dot`` of tests/_rescore_cases.py);
- its ``variant``s: the turns a kernel could take instead (``WRONG``), each of which must change an answer on some case;
- ``cases(dtype)``: parts and primary fields built where the kernels can go wrong; ``census`` says which edges a case holds."""
import functools
from collections import namedtuple

import numpy as np

from tests._rescore_cases import (CHUNK, DTYPES, Case, Field, _random_rows, _structured_rows, _values, bits, csr_of,  # noqa: F401
                                  make_cand, physical, ref_pairs_dot, same_result, table_field)

Part = namedtuple("Part", "cols vals counts")
UnionCase = namedtuple("UnionCase", "parts n_cols primary")          # primary: a Field (its weight is ignored)
MAX_ENTRIES = 2048                                                   # the sum of the parts' strides sg_topn_union takes
SHORT = 64                                                           # entries of a row above which a block unites it
MANY_LONG_ROWS = 2100                                                # above 256 CUs x 8 blocks of union_block_kernel's grid
WRONG = ("last_part_value", "duplicates_kept", "arrival_order", "dead_ignored_left", "dead_ignored_right", "fill_everything",
         "stride_sum", "last_entry_lost", "entry_65_lost", "twice_last_place")


# ------------------------------------------------------------------------------------------ the statement
def counted(part: Part):
    """clamp(counts, 0, S): the entries of every row that count."""
    return np.clip(part.counts.astype(np.int64), 0, part.cols.shape[1])


def ref_union(case: UnionCase, variant=None):
    """(cols[R, stride], vals, counts) of the statement -- or of one wrong turn.  Cells behind a row's count are 0."""
    parts, fld = case.parts, case.primary
    T = parts[0].vals.dtype.type
    R = parts[0].cols.shape[0]
    cnt = [counted(p) for p in parts]
    rows = []                                                        # per row: (columns, values, filled?) in output order
    for i in range(R):
        cols, vals, from0, seen, g = [], [], [], {}, 0
        for p, part in enumerate(parts):
            c = int(cnt[p][i])
            for e in range(c):
                lost = (variant == "last_entry_lost" and e == c - 1) or (variant == "entry_65_lost" and g == 64)
                g += 1
                if lost:
                    continue
                j = int(part.cols[i, e])
                if j in seen and variant != "duplicates_kept":
                    if from0[seen[j]] and (variant == "last_part_value" or (variant == "twice_last_place" and p == 0)):
                        vals[seen[j]] = part.vals[i, e]
                    continue
                seen[j] = len(cols)
                cols.append(j)
                vals.append(part.vals[i, e])
                from0.append(p == 0)
        cols, vals, from0 = np.array(cols, np.int64), np.array(vals, T), np.array(from0, bool)
        if variant != "arrival_order":
            order = np.argsort(cols, kind="stable")
            cols, vals, from0 = cols[order], vals[order], from0[order]
        if variant == "fill_everything":
            from0[:] = False
        rows.append((cols, vals, from0))
    # the primary field's score of every column part 0 does not hold
    fi = np.concatenate([np.full(int((~f).sum()), i, np.int64) for i, (_, _, f) in enumerate(rows)] + [np.zeros(0, np.int64)])
    fj = np.concatenate([c[~f] for c, _, f in rows] + [np.zeros(0, np.int64)])
    a = physical(None if variant == "dead_ignored_left" else fld.dead_a, fi)
    b = physical(None if variant == "dead_ignored_right" else fld.dead_b, fj)
    filled = ref_pairs_dot(fld.A, fld.B, a, b)
    counts = np.array([len(c) for c, _, _ in rows], np.int32)
    stride = sum(p.cols.shape[1] for p in parts) if variant == "stride_sum" else max(1, int(counts.max(initial=0)))
    out_c, out_v = np.zeros((R, stride), np.int32), np.zeros((R, stride), T)
    at = 0
    for i, (c, v, f) in enumerate(rows):
        v = v.copy()
        n = int((~f).sum())
        v[~f] = filled[at:at + n]
        at += n
        out_c[i, :len(c)], out_v[i, :len(c)] = c, v
    return out_c, out_v, counts


# ------------------------------------------------------------------------------------------ building blocks
def part_of(rows, stride, dtype, n_cols):
    return Part(*make_cand(rows, stride, dtype, n_cols))


def _two_rows(rng, n0, n1, overlap, n_cols, dtype):
    """Row of part 0 with n0 columns, of part 1 with n1, `overlap` of them shared; every part in an order of its own."""
    cols = rng.choice(n_cols, n0 + n1 - overlap, replace=False)
    c0, c1 = rng.permutation(cols[:n0]), rng.permutation(cols[n0 - overlap:])
    return (c0, np.round(rng.uniform(0.5, 1.0, n0), 3).astype(dtype)), (c1, np.round(rng.uniform(0.5, 1.0, n1), 3).astype(dtype))


def _table(rng, n_left, n_cols, dtype, dead_a=None, dead_b=None):
    """A primary field whose score of (i, j) is table[j] * (1 + i / 16): every left and every right row is its own."""
    f = table_field(n_left, rng.uniform(0.1, 1, n_cols), dtype, 1.0, dead_a, dead_b)
    live = np.delete(np.arange(f.A.shape[0]), np.zeros(0, np.int64) if f.dead_a is None else f.dead_a)
    f.A.data[live] = (1 + np.arange(n_left) / 16).astype(dtype)
    return f


def _random_case(rng, counts_by_part, strides, n_cols, dtype, **dead):
    R = len(counts_by_part[0])
    parts = [part_of(_random_rows(rng, c, n_cols, dtype), s, dtype, n_cols) for c, s in zip(counts_by_part, strides)]
    return UnionCase(parts, n_cols, _table(rng, R, n_cols, dtype, **dead))


def _pairs_case(rng, shapes, strides, n_cols, dtype):
    """shapes: (n0, n1, overlap) a row."""
    both = [_two_rows(rng, n0, n1, ov, n_cols, dtype) for n0, n1, ov in shapes]
    parts = [part_of([r[p] for r in both], strides[p], dtype, n_cols) for p in (0, 1)]
    return UnionCase(parts, n_cols, _table(rng, len(shapes), n_cols, dtype))


@functools.lru_cache(maxsize=None)
def cases(dtype):
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(8200 + np.dtype(dtype).itemsize)
    out = {}
    # ---- two parts of short rows; 37 rows: a last wave (8 rows) and a last block (32 rows) partly filled; rows empty in part 0,
    # rows empty in every part
    R = 37
    c0, c1 = rng.integers(0, 11, R), rng.integers(0, 11, R)
    c0[:6], c1[:6] = [0, 0, 5, 10, 10, 0], [0, 4, 0, 10, 0, 10]
    out["two_parts_short"] = _random_case(rng, [c0, c1], [10, 10], 60, dtype)
    out["three_parts_1_10_64"] = _random_case(rng, [rng.integers(0, 2, 20), rng.integers(0, 11, 20), rng.integers(0, 54, 20)],
                                              [1, 10, 64], 300, dtype)
    out["eight_parts"] = _random_case(rng, [rng.integers(0, s + 1, 20) for s in range(1, 9)], list(range(1, 9)), 30, dtype)
    # ---- union sizes around the two kernels' border, rows of either kernel in one call (strides 64 and 65)
    shapes = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (32, 31, 0), (40, 40, 17), (32, 32, 0), (64, 0, 0), (64, 64, 64), (40, 40, 16),
              (32, 33, 0), (64, 65, 64), (64, 65, 0), (33, 32, 1), (3, 2, 1)]
    out["union_sizes"] = _pairs_case(rng, shapes, [64, 65], 400, dtype)
    # ---- the longest rows: 1 024 + 1 024 entries, 2 047 and 2 048 distinct columns
    out["wide_1024"] = _pairs_case(rng, [(1024, 1024, 1), (1024, 1024, 0), (1024, 1024, 1024), (3, 1024, 2), (0, 0, 0)],
                                   [1024, 1024], 2500, dtype)
    # ---- more rows above the short kernel's 64 entries than the block kernel's grid has blocks: a block takes several
    out["many_long_rows"] = _pairs_case(rng, [(33, 32, 31)] * MANY_LONG_ROWS, [33, 32], 80, dtype)
    # ---- content
    ident = _pairs_case(rng, [(6, 6, 6)] * 9 + [(0, 0, 0)], [6, 6], 40, dtype)
    p0 = ident.parts[0]
    out["identical_parts"] = ident._replace(parts=[p0, Part(p0.cols, p0.vals, p0.counts)])      # nothing to fill
    out["disjoint_parts"] = _pairs_case(rng, [(5, 7, 0)] * 9, [5, 7], 200, dtype)
    out["shared_value_differs"] = _pairs_case(rng, [(5, 5, 3)] * 6, [5, 5], 30, dtype)           # (the parts' values are drawn apart)
    tiny = np.finfo(dtype).tiny
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, tiny / 4], dtype)
    sp0 = (np.array([9, 2, 7, 0, 39, 20]), special)
    sp1 = (np.array([0, 39, 2, 7, 9, 20, 11]), np.full(7, 0.5, dtype))                           # columns 0 and N - 1 in both
    out["special_values"] = UnionCase([part_of([sp0, sp0], 6, dtype, 40), part_of([sp1, (np.array([39, 0]), np.full(2, 0.5, dtype))], 7, dtype, 40)],
                                      40, _table(rng, 2, 40, dtype))
    # a caller-made part that names a column twice: in part 0 the entry at the lowest place gives the value
    tw0 = (np.array([7, 3, 7, 12]), np.array([0.7, 0.3, 0.9, 0.1], dtype))
    tw1 = (np.array([3, 3, 9, 9, 7]), np.array([0.4, 0.5, 0.6, 0.7, 0.8], dtype))
    out["named_twice"] = UnionCase([_raw_part([tw0, tw1], 5, dtype), _raw_part([tw1, tw1], 5, dtype)], 20, _table(rng, 2, 20, dtype))
    # counts above the stride and below zero
    base = _random_case(rng, [[4, 4, 4, 4, 4, 4]] * 3, [4, 4, 4], 50, dtype)
    bent = []
    for p, part in enumerate(base.parts):
        counts = part.counts.copy()
        counts[p], counts[p + 3] = 4 + 5 + p, -1 - p
        bent.append(Part(part.cols, part.vals, counts))
    out["counts_outside"] = base._replace(parts=bent)
    # ---- filled pairs whose rows sit at the merge's chunk edges
    a_rows, b_rows, _ = _structured_rows(rng, dtype)
    SA, SB = csr_of(a_rows, dtype), csr_of(b_rows, dtype)
    n = len(b_rows)
    q0 = [(np.array([(p + 1) % n]), np.array([0.9], dtype)) for p in range(len(a_rows))]
    q1 = [(np.array([(p + 2) % n, p, (p + 1) % n]), np.array([0.8, 0.7, 0.6], dtype)) for p in range(len(a_rows))]
    out["fill_structured"] = UnionCase([part_of(q0, 1, dtype, n), part_of(q1, 3, dtype, n)], n, Field(SA, SB, 1.0, None, None))
    lengths = (0, 1, 7, 8, 9, 16, 17, 64, 65)
    M = csr_of([(np.sort(rng.choice(256, k, replace=False)), _values(rng, k, dtype)) for k in lengths], dtype)
    L = len(lengths)
    diag = [(np.array([r]), np.array([1.0], dtype)) for r in range(L)]
    full = [(np.arange(L)[::-1], np.linspace(1, 0.5, L).astype(dtype))] * L
    out["fill_lengths_self"] = UnionCase([part_of(diag, 1, dtype, L), part_of(full, L, dtype, L)], L, Field(M, M, 1.0, None, None))
    # ---- dead lists (tables: a dead row holds POISON); the named pair is found by part 1 alone, so it is filled
    R, N = 12, 40
    named_row, named_col = 5, 17

    def dead_case(dead_a, dead_b):
        r0 = _random_rows(rng, [4] * R, N, dtype)
        r1 = _random_rows(rng, [6] * R, N, dtype)
        r0[named_row] = (np.array([3, 30]), np.array([0.9, 0.8], dtype))
        r1[named_row] = (np.array([named_col, 3, 31]), np.array([0.9, 0.8, 0.7], dtype))
        return UnionCase([part_of(r0, 4, dtype, N), part_of(r1, 6, dtype, N)], N, _table(rng, R, N, dtype, dead_a, dead_b))

    out["dead_before"] = dead_case([named_row - 1], [named_col - 1])
    out["dead_at"] = dead_case([named_row], [named_col])
    out["dead_after"] = dead_case([named_row + 1], [named_col + 1])
    out["dead_first_and_last"] = dead_case([0, R + 1], [0, N + 1])
    out["dead_32"] = dead_case(np.sort(rng.choice(R + 32, 32, replace=False)), np.sort(rng.choice(N + 32, 32, replace=False)))
    out["dead_left_only"] = dead_case([2, 3, 9], None)
    out["dead_right_only"] = dead_case(None, [0, 17, 18, 41])
    # the same handle on both sides, with its dead list on both: a self-join of a corpus with removed rows pending
    n_live, dead = 20, np.array([0, 4, 5, 11, 22])
    f = table_field(n_live, rng.uniform(0.25, 1, n_live), dtype, 1.0, dead, dead)
    same = csr_of([([0, 1 + r % 3], [v, 0.5]) for r, v in enumerate(f.B.data)], dtype, 4)
    out["dead_same_handle"] = UnionCase([part_of(_random_rows(rng, [3] * n_live, n_live, dtype), 3, dtype, n_live),
                                         part_of(_random_rows(rng, [5] * n_live, n_live, dtype), 5, dtype, n_live)], n_live,
                                        Field(same, same, 1.0, dead, dead))
    for case in out.values():
        for part in case.parts:
            for arr in part:
                arr.setflags(write=False)
    return out


def _raw_part(rows, stride, dtype):
    """As ``make_cand``, for rows that may name a column twice."""
    cols, vals = np.zeros((len(rows), stride), np.int32), np.zeros((len(rows), stride), dtype)
    counts = np.array([len(c) for c, _ in rows], np.int32)
    for r, (c, v) in enumerate(rows):
        cols[r, :len(c)], vals[r, :len(c)] = c, v
    return Part(cols, vals, counts)


@functools.lru_cache(maxsize=None)
def expected(dtype, name):
    """The reference of a case, computed once."""
    want = ref_union(cases(dtype)[name])
    for a in want:
        a.setflags(write=False)
    return want


def rescore_case(case: UnionCase, union, weights=(0.5, 0.5), threshold=0.3, top_n=5) -> Case:
    """The union as the candidates of a rescoring on one further field (a table of its own): what the engine does next."""
    cols, vals, counts = union
    rng = np.random.default_rng(11)
    fld = table_field(cols.shape[0], rng.uniform(0, 1, case.n_cols), vals.dtype.type, weights[1])
    return Case(cols, vals, counts, case.n_cols, weights[0], [fld], threshold, top_n)


# ------------------------------------------------------------------------------------------ what the cases hold
def census(dtype):
    """The edges the cases are built for, as sets and flags, from the cases themselves."""
    dtype = np.dtype(dtype).type
    seen = dict(n_parts=set(), strides=set(), stride_lists=set(), union_sizes=set(), totals=set(), fill_row_lengths=set(),
                dead_lengths=set(), flags=set())
    for name, case in cases(dtype).items():
        parts, fld = case.parts, case.primary
        R = parts[0].cols.shape[0]
        cnt = np.stack([counted(p) for p in parts])
        total = cnt.sum(axis=0)
        w_cols, w_vals, w_counts = expected(dtype, name)
        seen["n_parts"].add(len(parts))
        seen["strides"] |= {p.cols.shape[1] for p in parts}
        seen["stride_lists"].add(tuple(p.cols.shape[1] for p in parts))
        seen["union_sizes"] |= set(int(c) for c in w_counts)
        seen["totals"] |= set(int(t) for t in total)
        if ((cnt[0] == 0) & (total > 0)).any():
            seen["flags"].add("a_row_empty_in_part_0_alone")
        if (total == 0).any():
            seen["flags"].add("a_row_empty_in_every_part")
        for p in parts:
            if (p.counts > p.cols.shape[1]).any():
                seen["flags"].add("a_count_above_the_stride")
            if (p.counts < 0).any():
                seen["flags"].add("a_negative_count")
        if (total <= SHORT).any() and (total > SHORT).any():
            seen["flags"].add("rows_for_both_kernels")
        if np.count_nonzero(total > SHORT) > 256 * 8:
            seen["flags"].add("more_long_rows_than_blocks")
        if R % 8 and R > 8:
            seen["flags"].add("last_wave_partly_filled")
        if R % 32 and R > 32:
            seen["flags"].add("last_block_partly_filled")
        filled_i, filled_j = [], []
        for i in range(R):
            sets = [set(int(j) for j in p.cols[i, :cnt[k][i]]) for k, p in enumerate(parts)]
            for k, p in enumerate(parts):
                if len(sets[k]) < cnt[k][i]:
                    seen["flags"].add("a_part_names_a_column_twice" + ("_part_0" if k == 0 else ""))
            others = set().union(*sets[1:])
            if total[i] and all(s == sets[0] for s in sets):
                seen["flags"].add("identical_rows_nothing_to_fill")
            if total[i] and sets[0] and others and not (sets[0] & others):
                seen["flags"].add("disjoint_rows")
            for j in sets[0] & others:
                v0 = parts[0].vals[i, list(parts[0].cols[i, :cnt[0][i]]).index(j)]
                for k in range(1, len(parts)):
                    at = np.flatnonzero(parts[k].cols[i, :cnt[k][i]] == j)
                    if len(at) and bits(parts[k].vals[i, at[:1]])[0] != bits(np.array([v0]))[0]:
                        seen["flags"].add("a_shared_column_whose_bits_differ")
            if 0 in sets[0] | others and case.n_cols - 1 in sets[0] | others:
                seen["flags"].add("columns_0_and_last")
            for j in sorted(others - sets[0]):
                filled_i.append(i)
                filled_j.append(j)
        v0 = np.concatenate([parts[0].vals[i, :cnt[0][i]] for i in range(R)] + [np.zeros(0, dtype)])
        for what, hit in (("nan", np.isnan(v0)), ("plus_inf", np.isposinf(v0)), ("minus_inf", np.isneginf(v0)),
                          ("plus_zero", (v0 == 0) & ~np.signbit(v0)), ("minus_zero", (v0 == 0) & np.signbit(v0)),
                          ("denormal", (v0 != 0) & (np.abs(v0) < np.finfo(dtype).tiny))):
            if hit.any():
                seen["flags"].add("part_0_holds_" + what)
        a, b = physical(fld.dead_a, filled_i), physical(fld.dead_b, filled_j)
        la, lb = np.diff(fld.A.indptr)[a], np.diff(fld.B.indptr)[b]
        seen["fill_row_lengths"] |= set(int(x) for x in la) | set(int(x) for x in lb)
        if fld.A is fld.B:
            seen["flags"].add("same_handle")
        for p in range(len(a)):
            ka = fld.A.indices[fld.A.indptr[a[p]]:fld.A.indptr[a[p] + 1]]
            kb = fld.B.indices[fld.B.indptr[b[p]]:fld.B.indptr[b[p] + 1]]
            common = np.intersect1d(ka, kb)
            if len(ka) > CHUNK and len(kb):
                if len(common) == 0:
                    seen["flags"].add("no_common_column")
                elif np.all(np.searchsorted(ka, common) < CHUNK):
                    seen["flags"].add("match_in_first_chunk_only")
                elif np.all(np.searchsorted(ka, common) >= CHUNK * ((len(ka) - 1) // CHUNK)):
                    seen["flags"].add("match_in_last_chunk_only")
        for side, dead, n_phys, named, live in (("left", fld.dead_a, fld.A.shape[0], a, filled_i), ("right", fld.dead_b, fld.B.shape[0], b, filled_j)):
            seen["dead_lengths"].add(0 if dead is None else len(dead))
            if dead is None:
                continue
            if 0 in dead and n_phys - 1 in dead:
                seen["flags"].add("dead_first_and_last")
            for d in dead:
                if d + 1 in named:
                    seen["flags"].add(f"dead_just_before_a_filled_row_{side}")
                if d - 1 in named:
                    seen["flags"].add(f"dead_just_after_a_filled_row_{side}")
            if np.intersect1d(live, dead).size:
                seen["flags"].add(f"dead_at_the_number_of_a_filled_row_{side}")
        if (fld.dead_a is None) != (fld.dead_b is None):
            seen["flags"].add("dead_on_one_side_only")
    return seen
