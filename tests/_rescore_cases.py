"""What sg_topn_rescore (csrc/sg_rescore.hip) is held to, for the CPU and the GPU tests alike.  TEST INFRASTRUCTURE ONLY.

- ``ref_rescore``: the statement of include/sg_hip.h in numpy, built on ``ref_pairs_dot`` of tests/_pair_cases.py -- live ->
  physical rows, the field scores, ``acc = acc + W[f] * s[f]`` on arrays of the value type, ``>``, a stable sort by (c
  descending by value, column ascending), the cut;
- its ``variant``s: the turns a kernel could take instead (``WRONG``), each of which must change an answer on some case;
- ``cases(dtype)``: candidates and fields built where the kernels can go wrong; ``census`` says which edges a case holds."""
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

from tests._pair_cases import DTYPES, _round_to, _structured_rows, _values, bits, csr_of, ref_pairs_dot, same_bits  # noqa: F401

Field = namedtuple("Field", "A B w dead_a dead_b")          # scipy matrices (A is B: one handle), weight, dead physical rows or None
Case = namedtuple("Case", "cols vals counts n_cols w0 fields threshold top_n")
MAX_STRIDE = 2048
CHUNK = 8                                                   # SG_PAIR_LANES: entries a chunk of the merge
MANY_LONG_ROWS = 2100                                       # above 256 CUs x 8 blocks of rescore_select_block_kernel's grid
WRONG = ("ge", "no_resort", "ties_by_position", "cut_before_filter", "cut_by_primary", "fma", "wide_accumulator",
         "descending_fields", "weight_after_sum", "side_left", "dead_ignored", "a_list_for_b", "last_chunk_lost", "nan_kept",
         "zero_sign_order")


# ------------------------------------------------------------------------------------------ the statement
def physical(dead, live, side="right"):
    """CorpusState.physical_rows: dead row q has dead[q] - q live rows before it."""
    live = np.asarray(live, np.int64)
    if dead is None or len(dead) == 0:
        return live
    dead = np.asarray(dead, np.int64)
    return live + np.searchsorted(dead - np.arange(len(dead)), live, side=side)


def _without_last_chunk(m):
    """Every row cut before its last chunk of eight entries: what a merge that drops a row's tail would read."""
    rows = []
    for r in range(m.shape[0]):
        lo, hi = m.indptr[r], m.indptr[r + 1]
        kept = CHUNK * max((hi - lo - 1) // CHUNK, 0)
        rows.append((m.indices[lo:lo + kept], m.data[lo:lo + kept]))
    return csr_of(rows, m.dtype.type, m.shape[1])


def _fma(acc, w, s, T):
    out = np.empty_like(acc)
    for p in range(len(acc)):
        if np.isfinite(acc[p]) and np.isfinite(s[p]):
            out[p] = _round_to(Fraction(float(w)) * Fraction(float(s[p])) + Fraction(float(acc[p])), T)
        else:
            out[p] = T(acc[p] + w * s[p])
    return out


def _combined(scores, W, T, variant):
    """scores[f][p], W[f] of type T -> c[p]."""
    n = len(scores[0])
    order = range(len(W))
    with np.errstate(all="ignore"):
        if variant == "descending_fields":
            order = reversed(order)
        if variant == "wide_accumulator":                   # products and sums exact (or as wide as there is), rounded once
            if all(np.all(np.isfinite(s)) for s in scores):
                return np.array([_round_to(sum(Fraction(float(W[f])) * Fraction(float(scores[f][p])) for f in range(len(W))), T)
                                 for p in range(n)], T).reshape(n)
            return sum(np.float64(W[f]) * scores[f].astype(np.float64) for f in range(len(W))).astype(T)
        if variant == "weight_after_sum" and len(set(float(w) for w in W)) == 1:
            acc = np.zeros(n, T)
            for f in order:
                acc = acc + scores[f]
            return (W[0] * acc).astype(T)
        acc = np.zeros(n, T)
        for k, f in enumerate(order):
            if variant == "fma":
                acc = _fma(acc, W[f], scores[f], T)
            elif variant == "zero_sign_order" and k == 0:   # the chain started from the first product: a -0.0 survives
                acc = (W[f] * scores[f]).astype(T)
            else:
                acc = acc + W[f] * scores[f]
        assert acc.dtype == T
        return acc


def ref_rescore(case: Case, variant=None):
    """(cols[R, min(k, S)], vals, counts) of the statement -- or of one wrong turn.  Cells behind a row's count are 0."""
    cols, vals, counts = case.cols, case.vals, case.counts
    T = vals.dtype.type
    R, S = cols.shape
    So = min(case.top_n, S)
    rows = np.repeat(np.arange(R), counts)
    ent = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int64)
    j, s0 = cols[rows, ent].astype(np.int64), vals[rows, ent]
    scores = [s0]
    for fld in case.fields:
        A, B = fld.A, fld.B
        if variant == "last_chunk_lost":
            A = _without_last_chunk(A)
        side = "left" if variant == "side_left" else "right"
        dead_a, dead_b = (None, None) if variant == "dead_ignored" else (fld.dead_a, fld.dead_b)
        if variant == "a_list_for_b":
            dead_b = dead_a
        a, b = physical(dead_a, rows, side), physical(dead_b, j, side)
        b = np.minimum(b, B.shape[0] - 1)                   # (a wrong turn may step outside: it reads the last row then)
        scores.append(ref_pairs_dot(A, B, a, b))
    W = [T(case.w0)] + [T(f.w) for f in case.fields]
    c = _combined(scores, W, T, variant)
    with np.errstate(all="ignore"):
        t = T(case.threshold)
        keep = (c >= t) if variant == "ge" else ~(c <= t) if variant == "nan_kept" else (c > t)
    out_c, out_v, out_n = np.zeros((R, So), np.int32), np.zeros((R, So), T), np.zeros(R, np.int32)
    start = np.r_[0, np.cumsum(counts)]
    for r in range(R):
        sel = np.arange(start[r], start[r + 1])
        if variant == "cut_before_filter":
            sel = sel[:case.top_n]
        sel = sel[keep[sel]]
        if variant == "cut_by_primary":
            sel = sel[:case.top_n]
        cr, jr = c[sel], j[sel]
        if variant == "no_resort":
            order = np.arange(len(sel))
        elif variant == "ties_by_position":
            order = np.argsort(-cr, kind="stable")
        elif variant == "zero_sign_order":
            order = np.lexsort((jr, np.signbit(cr), -cr))
        else:
            order = np.lexsort((jr, -cr))                   # by value: -(+0.0) and -(-0.0) are equal; stable
        if variant == "nan_kept":
            order = np.r_[order[np.isnan(cr[order])], order[~np.isnan(cr[order])]]
        order = order[:So]
        out_n[r] = len(order)
        out_c[r, :len(order)], out_v[r, :len(order)] = jr[order], cr[order]
    return out_c, out_v, out_n


def same_result(got, want) -> bool:
    """Columns, value bits and counts of the first ``count`` entries of every row."""
    (gc, gv, gn), (wc, wv, wn) = got, want
    if gc.shape != wc.shape or gv.dtype != wv.dtype or not np.array_equal(gn, wn):
        return False
    mask = np.arange(wc.shape[1])[None, :] < wn[:, None]
    return np.array_equal(gc[mask], wc[mask]) and np.array_equal(bits(gv[mask]), bits(wv[mask]))


# ------------------------------------------------------------------------------------------ building blocks
def make_cand(rows, stride, dtype, n_cols):
    """rows: a list of (columns, scores) in candidate order."""
    cols, vals = np.zeros((len(rows), stride), np.int32), np.zeros((len(rows), stride), dtype)
    counts = np.array([len(c) for c, _ in rows], np.int32)
    for r, (c, v) in enumerate(rows):
        cols[r, :len(c)], vals[r, :len(c)] = c, v
    assert counts.max(initial=0) <= stride and (cols >= 0).all() and (cols < n_cols).all()
    return cols, vals, counts


POISON = 1000.0


def table_field(n_left, table, dtype, w, dead_a=None, dead_b=None):
    """A field whose score of (i, j) is exactly table[j]: every left row is {column 0: 1.0}, right row j {column 0: table[j]}.
    Dead physical rows hold POISON: a wrong row map shows."""
    def phys(values, dead):
        dead = np.zeros(0, np.int64) if dead is None else np.asarray(dead, np.int64)
        out = np.full(len(values) + len(dead), POISON, dtype)
        out[np.delete(np.arange(len(out)), dead)] = values
        return csr_of([([0], [v]) for v in out], dtype, 4)
    return Field(phys(np.ones(n_left, dtype), dead_a), phys(np.asarray(table, dtype), dead_b), w,
                 None if dead_a is None else np.asarray(dead_a, np.int64), None if dead_b is None else np.asarray(dead_b, np.int64))


def _random_rows(rng, counts, n_cols, dtype):
    """Candidate rows as a multiply leaves them: distinct columns, scores descending then column ascending."""
    rows = []
    for c in counts:
        cols = rng.choice(n_cols, c, replace=False)
        vals = np.round(rng.uniform(0.5, 1.0, c), 2).astype(dtype)
        order = np.lexsort((cols, -vals))
        rows.append((cols[order], vals[order]))
    return rows


def _table_case(rng, counts, stride, n_cols, dtype, weights, threshold, top_n, **dead):
    rows = _random_rows(rng, counts, n_cols, dtype)
    fields = [table_field(len(rows), rng.uniform(0, 1, n_cols), dtype, w, **(dead if k == 0 else {})) for k, w in enumerate(weights[1:])]
    return Case(*make_cand(rows, stride, dtype, n_cols), n_cols, weights[0], fields, threshold, top_n)


@functools.lru_cache(maxsize=None)
def cases(dtype):
    dtype = np.dtype(dtype).type
    T = dtype
    rng = np.random.default_rng(7100 + np.dtype(dtype).itemsize)
    eps = np.finfo(dtype).eps
    out = {}
    half = (0.5, 0.25, 0.25)
    # ---- candidate counts around a group's stride of eight, a chunk of 64 and the two select kernels; a last wave (8 rows)
    # and a last block (32 rows) that are partly filled
    short_counts = [0, 1, 7, 8, 9, 63, 64] + [int(x) for x in rng.integers(0, 12, 30)]
    out["counts_short"] = _table_case(rng, short_counts, 64, 300, dtype, half, 0.55, 10)
    out["counts_long"] = _table_case(rng, [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 3, 0], 129, 300, dtype, half, 0.55, 10)
    for stride, top_n, thr in ((10, 10, -1.0), (64, 64, 0.5), (65, 65, 0.5), (65, 64, 0.3), (2048, 2048, 0.5), (2048, 20, 0.3)):
        out[f"full_{stride}_top{top_n}"] = _table_case(rng, [stride] * 3, stride, stride + 52, dtype, half, thr, top_n)
    # more rows above the short kernel's 64 candidates than the block kernel's grid has blocks (eight a CU): a block takes several
    out["many_long_rows"] = _table_case(rng, [65] * MANY_LONG_ROWS, 65, 80, dtype, (0.5, 0.5), 0.6, 3)
    out["top_n_above_stride"] = _table_case(rng, [10, 4, 0], 10, 40, dtype, half, -1.0, 500)
    # ---- field rows at the merge's chunk edges: every length against every length, one handle on both sides
    lengths = (0, 1, 7, 8, 9, 16, 17, 64, 65)
    M = csr_of([(np.sort(rng.choice(256, n, replace=False)), _values(rng, n, dtype)) for n in lengths], dtype)
    full = [(np.arange(len(lengths)), np.linspace(1, 0.5, len(lengths)).astype(dtype))] * len(lengths)
    out["field_lengths_self"] = Case(*make_cand(full, len(lengths), dtype, len(lengths)), len(lengths), 0.5,
                                     [Field(M, M, 0.25, None, None), Field(M, M, 0.125, None, None)], -1e30, 4)
    a_rows, b_rows, pairs = _structured_rows(rng, dtype)    # the match in the first / the last chunk only, no common column
    SA, SB = csr_of(a_rows, dtype), csr_of(b_rows, dtype)
    rows = [(np.array([p, (p + 1) % len(b_rows)]), np.array([0.9, 0.8], dtype)) for p in range(len(a_rows))]
    out["field_structured"] = Case(*make_cand(rows, 2, dtype, len(b_rows)), len(b_rows), 1.0, [Field(SA, SB, 1e-3, None, None)], -1e30, 2)
    # ---- exact binary fractions: c at the threshold, one ulp above and one below
    s0 = np.array([1.0, 1.0, 1.0, 0.5, 1.0], dtype)
    t1 = np.array([0.5, 0.5, 0.5, 1.5, 0.25], dtype)
    t2 = np.array([0.5, 0.5 + 2 * eps, 0.5 - 2 * eps, 0.5, 0.5], dtype)   # c = 0.75, 0.75 + eps / 2, 0.75 - eps / 2, 0.75, 0.6875
    out["threshold_exact"] = Case(*make_cand([(np.arange(5), s0)], 5, dtype, 5), 5, 0.5,
                                  [table_field(1, t1, dtype, 0.25), table_field(1, t2, dtype, 0.25)], 0.75, 5)
    # ---- weights that are no binary fractions: the order of the adds and a fused multiply-add change the last bit
    for name, w, n_f in (("tenth", 0.1, 2), ("tenth", 0.1, 7), ("third", 1 / 3, 2), ("third", 1 / 3, 7)):
        weights = ((1.0 - n_f * w) if name == "tenth" else w,) + (w,) * n_f
        out[f"weights_{name}_{n_f}"] = _table_case(rng, [40] * 5, 40, 64, dtype, weights, 0.2, 40)
    # ---- the combined order is the reverse of the candidates'
    n = 12
    out["reverse_order"] = Case(*make_cand([(np.arange(n), (1.0 - np.arange(n) / 64).astype(dtype))], n, dtype, n), n, 0.5,
                                [table_field(1, np.arange(n) / 16, dtype, 0.25), table_field(1, np.arange(n) / 16, dtype, 0.25)], 0.0, 5)
    # ---- blocks of equal c over the ranks k - 2 .. k + 2 whose candidate order and column order disagree
    for k in (1, 10, 64, 65):
        lead, block, tail = max(k - 2, 0), 5, 3
        m = lead + block + tail
        # candidate order: s0 descending; columns DESCEND inside the block; the first field lifts the block's members to one c
        s0 = (1.0 - np.arange(m) / 256).astype(dtype)
        cols = np.arange(m)
        cols[lead:lead + block] = cols[lead:lead + block][::-1]
        lift = np.zeros(m)
        lift[lead:lead + block] = np.arange(block) / 128             # 0.5 * (-q / 256) + 0.25 * (q / 128) = 0
        table = np.zeros(m)
        table[cols] = lift
        out[f"ties_k{k}"] = Case(*make_cand([(cols, s0)], m, dtype, m), m, 0.5,
                                 [table_field(1, table, dtype, 0.25), table_field(1, np.zeros(m), dtype, 0.25)], 0.0, k)
    # ---- special values
    out["zeros"] = Case(*make_cand([(np.array([7, 2, 4]), np.array([0.0, -0.0, 0.25], dtype))], 3, dtype, 8), 8, 0.5,
                        [table_field(1, np.zeros(8), dtype, -0.25), table_field(1, np.zeros(8), dtype, -0.25)], -0.5, 3)
    table = np.array([np.nan, np.inf, -np.inf, 0.5, np.inf, 0.25], dtype)
    zero_times_inf = np.array([0.5, 0.5, 0.5, 0.5, 0.0, 0.5], dtype)
    out["nan_inf"] = Case(*make_cand([(np.arange(6), np.full(6, 0.9, dtype)), (np.array([3, 5]), np.array([0.9, 0.8], dtype))], 6, dtype, 6),
                          6, 0.5, [table_field(2, table, dtype, 0.25), table_field(2, zero_times_inf, dtype, 0.25)], 0.3, 6)
    out["all_fail"] = _table_case(rng, [6, 9, 3], 9, 30, dtype, half, 5.0, 4)
    # ---- dead lists (tables: a dead row holds POISON)
    R, N = 12, 40
    named_row, named_col = 5, 17

    def dead_case(dead_a, dead_b, dead_a2=None, dead_b2=None, top_n=6):
        rows = _random_rows(rng, [6] * R, N, dtype)
        rows[named_row] = (np.array([named_col, 3, 30]), np.array([0.9, 0.8, 0.7], dtype))
        f1 = table_field(R, rng.uniform(0, 1, N), dtype, 0.25, dead_a, dead_b)
        f2 = table_field(R, rng.uniform(0, 1, N), dtype, 0.25, dead_a2, dead_b2)
        # the left rows differ too: row i scores table[j] * (1 + i / 16)
        for f in (f1, f2):
            live = np.delete(np.arange(f.A.shape[0]), np.zeros(0, np.int64) if f.dead_a is None else f.dead_a)
            f.A.data[live] = (1 + np.arange(R) / 16).astype(dtype)
        return Case(*make_cand(rows, 6, dtype, N), N, 0.5, [f1, f2], 0.3, top_n)

    out["dead_before"] = dead_case([named_row - 1], [named_col - 1])     # (nothing dead before them: physical == live there)
    out["dead_at"] = dead_case([named_row], [named_col])
    out["dead_after"] = dead_case([named_row + 1], [named_col + 1])
    out["dead_first_and_last"] = dead_case([0, R + 1], [0, N + 1])
    out["dead_32"] = dead_case(np.sort(rng.choice(R + 32, 32, replace=False)), np.sort(rng.choice(N + 32, 32, replace=False)))
    out["dead_sides_and_fields_differ"] = dead_case([2, 3, 9], [0, 17, 18, 41], None, [5, 6, 7])
    # the same handle on both sides, with its dead list on both: a self-join of a corpus with removed rows pending
    n_live, dead = 20, np.array([0, 4, 5, 11, 22])
    table = rng.uniform(0.25, 1, n_live)
    f = table_field(n_live, table, dtype, 0.5, dead, dead)
    same = csr_of([([0, 1 + r % 3], [v, 0.5]) for r, v in enumerate(f.B.data)], dtype, 4)
    out["dead_same_handle"] = Case(*make_cand(_random_rows(rng, [5] * n_live, n_live, dtype), 5, dtype, n_live), n_live, 0.5,
                                   [Field(same, same, 0.5, dead, dead)], 0.3, 3)
    for case in out.values():
        for arr in (case.cols, case.vals, case.counts):
            arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(dtype, name):
    """The reference of a case, computed once."""
    want = ref_rescore(cases(dtype)[name])
    for a in want:
        a.setflags(write=False)
    return want


# ------------------------------------------------------------------------------------------ what the cases hold
def census(dtype):
    """The edges the cases are built for, as sets and flags, from the cases themselves."""
    dtype = np.dtype(dtype).type
    seen = dict(counts=set(), full_strides=set(), field_row_lengths=set(), n_fields=set(), dead_lengths=set(), top_n=set(),
                flags=set())
    for name, case in cases(dtype).items():
        R, S = case.cols.shape
        seen["counts"] |= set(int(c) for c in case.counts)
        seen["full_strides"] |= {S} if (case.counts == S).any() else set()
        seen["n_fields"].add(len(case.fields))
        seen["top_n"].add(case.top_n)
        if R % 8 and R > 8:
            seen["flags"].add("last_wave_partly_filled")
        if R % 32 and R > 32:
            seen["flags"].add("last_block_partly_filled")
        rows = np.repeat(np.arange(R), case.counts)
        ent = np.concatenate([np.arange(c) for c in case.counts] + [np.zeros(0, np.int64)]).astype(np.int64)
        j = case.cols[rows, ent].astype(np.int64)
        for fld in case.fields:
            a, b = physical(fld.dead_a, rows), physical(fld.dead_b, j)
            la, lb = np.diff(fld.A.indptr)[a], np.diff(fld.B.indptr)[b]
            seen["field_row_lengths"] |= set(int(x) for x in la) | set(int(x) for x in lb)
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
            for side, dead, n_phys, named in (("a", fld.dead_a, fld.A.shape[0], a), ("b", fld.dead_b, fld.B.shape[0], b)):
                seen["dead_lengths"].add(0 if dead is None else len(dead))
                if dead is None:
                    continue
                if 0 in dead and n_phys - 1 in dead:
                    seen["flags"].add("dead_first_and_last")
                for d in dead:
                    for off, what in ((1, "dead_just_before_a_named_row"), (-1, "dead_just_after_a_named_row")):
                        if d + off in named:
                            seen["flags"].add(what)
            if fld.dead_a is not None and fld.dead_b is not None and not np.array_equal(fld.dead_a, fld.dead_b):
                seen["flags"].add("dead_lists_differ_between_sides")
            for live, dead in ((rows, fld.dead_a), (j, fld.dead_b)):
                if dead is not None and np.intersect1d(live, dead).size:
                    seen["flags"].add("dead_at_the_number_of_a_named_row")
        if len({None if f.dead_b is None else tuple(f.dead_b) for f in case.fields}) > 1:
            seen["flags"].add("dead_lists_differ_between_fields")
        c_cols, c_vals, c_counts = expected(dtype, name)
        if (c_counts == 0).any() and (case.counts[c_counts == 0] > 0).any():
            seen["flags"].add("a_row_whose_entries_all_fail")
        if np.array_equal(c_counts, case.counts) and (case.top_n >= case.counts).all() and case.counts.max() > 1:
            seen["flags"].add("nothing_fails_and_k_covers_the_row")
    return seen
