"""What sg_topn_rescore with floors (csrc/sg_rescore.hip) is held to, for the CPU and the GPU tests alike.  TEST INFRASTRUCTURE ONLY.

- ``ref_rescore_floors``: ``ref_rescore`` of tests/_rescore_cases.py with the floor mask -- ``s_f > (T)m_f`` on every field
  that has a floor, the score the candidate carries included -- applied to ``keep`` before the per-row selection;
- its ``variant``s (``WRONG``): the turns the kernel's mask could take instead, each of which must change an answer on some case;
- ``floor_cases(dtype)``: ``{name: (Case, floors)}``, the cases of ``_rescore_cases.cases`` with floors chosen from each case's
  own scores; ``census`` says which edges they hold."""
import functools

import numpy as np

from tests import _rescore_cases as C
from tests._pair_cases import ref_pairs_dot

ROW_CHUNK = 64                                              # SG_PAIR_ROW_CHUNK: entries of a row one group walks, a mask bit each
WRONG = ("ge", "after_cut", "weighted", "primary_ignored", "shifted", "failed_as_zero", "mask_restarted", "bit63_lost",
         "mask_carried")


# ------------------------------------------------------------------------------------------ the statement
def candidate_scores(case):
    """(row, entry, column, [s_0, s_1 .. s_F]) of every counted candidate, rows ascending, entries in candidate order."""
    rows = np.repeat(np.arange(case.cols.shape[0]), case.counts)
    ent = np.concatenate([np.arange(c) for c in case.counts] + [np.zeros(0, np.int64)]).astype(np.int64)
    j = case.cols[rows, ent].astype(np.int64)
    scores = [case.vals[rows, ent]]
    for fld in case.fields:
        scores.append(ref_pairs_dot(fld.A, fld.B, C.physical(fld.dead_a, rows), C.physical(fld.dead_b, j)))
    return rows, ent, j, scores


def refused(scores, floors, W, ent, T, variant=None):
    """For every candidate: has a floor refused it?  ``floors``: one entry a field, the primary's first, None: no floor."""
    floors = list(floors)
    F = len(scores) - 1
    assert len(floors) == F + 1
    if variant == "primary_ignored":
        floors[0] = None
    if variant == "shifted":                                # further field f reads the entry of field f - 1
        floors = [floors[0]] + floors[:F]
    if variant == "mask_restarted":                         # only what the last field's pass refused is still known at the end
        floors = [None] * F + [floors[F]]
    out = np.zeros(len(ent), bool)
    with np.errstate(all="ignore"):
        for f, m in enumerate(floors):
            if m is None:
                continue
            s = (W[f] * scores[f]).astype(T) if variant == "weighted" else scores[f]
            out |= ~((s >= T(m)) if variant == "ge" else (s > T(m)))
    if variant == "bit63_lost":
        out &= ent % ROW_CHUNK != ROW_CHUNK - 1
    if variant == "mask_carried":                           # (rows are contiguous: entry e - 64 of the row lies 64 places back)
        for p in np.flatnonzero(ent >= ROW_CHUNK):
            out[p] |= out[p - ROW_CHUNK]
    return out


def ref_rescore_floors(case, floors, variant=None):
    """(cols[R, min(k, S)], vals, counts) of the statement with floors -- or of one wrong turn."""
    T = case.vals.dtype.type
    R, S = case.cols.shape
    So = min(case.top_n, S)
    rows, ent, j, scores = candidate_scores(case)
    W = [T(case.w0)] + [T(f.w) for f in case.fields]
    failed = refused(scores, floors, W, ent, T, variant)
    if variant == "failed_as_zero":                         # a field below its floor counts 0, the candidate stays
        with np.errstate(all="ignore"):
            scores = [s if m is None else np.where(s > T(m), s, T(0)).astype(T) for s, m in zip(scores, floors)]
        failed[:] = False
    c = C._combined(scores, W, T, None)
    with np.errstate(all="ignore"):
        above = c > T(case.threshold)
    keep = above if variant == "after_cut" else above & ~failed
    out_c, out_v, out_n = np.zeros((R, So), np.int32), np.zeros((R, So), T), np.zeros(R, np.int32)
    start = np.r_[0, np.cumsum(case.counts)]
    for r in range(R):
        sel = np.arange(start[r], start[r + 1])
        sel = sel[keep[sel]]
        order = sel[np.lexsort((j[sel], -c[sel]))][:So]
        if variant == "after_cut":
            order = order[~failed[order]]
        out_n[r] = len(order)
        out_c[r, :len(order)], out_v[r, :len(order)] = j[order], c[order]
    return out_c, out_v, out_n


# ------------------------------------------------------------------------------------------ the cases
def _present(scores, q):
    """A score that is present: the q-quantile of the finite ones, as one of them."""
    s = np.sort(scores[np.isfinite(scores)])
    return s[min(int(q * len(s)), len(s) - 1)]


@functools.lru_cache(maxsize=None)
def floor_cases(dtype):
    dtype = np.dtype(dtype).type
    T = dtype
    base = C.cases(dtype)
    out = {}

    def scores_of(name):
        return candidate_scores(base[name])[3]

    def down(x):
        return np.nextafter(T(x), T(-np.inf))

    # ---- a floor equal to a score that is present (strict: it fails) and one ulp below it (it passes)
    for name in ("counts_short", "counts_long", "field_lengths_self", "dead_sides_and_fields_differ", "dead_same_handle"):
        s = scores_of(name)
        m = _present(s[1], 0.5)
        F = len(s) - 1
        out[f"{name}:equal"] = (base[name], [None, m] + [None] * (F - 1))
        out[f"{name}:ulp_below"] = (base[name], [None, down(m)] + [None] * (F - 1))
        out[f"{name}:primary_only"] = (base[name], [_present(s[0], 0.4)] + [None] * F)
        out[f"{name}:last_only"] = (base[name], [None] * F + [_present(s[F], 0.4)])
        out[f"{name}:all"] = (base[name], [_present(x, 0.2) for x in s])
    # ---- seven further fields: a floor on every one of the eight, on the last alone, None mixed in
    for name in ("weights_tenth_7", "weights_third_7"):
        s = scores_of(name)
        out[f"{name}:all_eight"] = (base[name], [_present(x, 0.1) for x in s])
        out[f"{name}:last_only"] = (base[name], [None] * 7 + [_present(s[7], 0.5)])
        out[f"{name}:mixed"] = (base[name], [None if f % 2 else _present(x, 0.3) for f, x in enumerate(s)])
    # ---- a floor that empties a row of candidates that c alone would keep
    case = base["top_n_above_stride"]                       # (threshold -1: everything passes it)
    rows, ent, j, s = candidate_scores(case)
    out["top_n_above_stride:row_emptied"] = (case, [None, s[1][rows == 1].max(), None])
    # ---- both select kernels, the full strides, many long rows
    for name in ("full_64_top64", "full_65_top64", "full_2048_top20", "many_long_rows", "all_fail", "reverse_order",
                 "ties_k10", "ties_k65", "threshold_exact", "field_structured"):
        s = scores_of(name)
        F = len(s) - 1
        out[f"{name}:median_last"] = (base[name], [None] * F + [_present(s[F], 0.5)])
        out[f"{name}:primary"] = (base[name], [_present(s[0], 0.3)] + [None] * F)
    # ---- special values: a NaN score never passes a floor, +inf passes every finite one, -inf none; zeros of either sign are
    # equal, so neither passes a floor of either zero
    nan_inf, zeros = base["nan_inf"], base["zeros"]
    out["nan_inf:floor_on_the_nan_field"] = (nan_inf, [None, 0.3, None])
    out["nan_inf:floor_behind_the_nan_field"] = (nan_inf, [None, None, 0.25])      # the NaN is the data's: it walks on
    out["nan_inf:huge"] = (nan_inf, [None, np.finfo(dtype).max, None])             # only +inf is above it
    out["nan_inf:lowest"] = (nan_inf, [None, -np.finfo(dtype).max, None])          # NaN and -inf alone fail
    out["zeros:plus_zero"] = (zeros, [None, 0.0, None])
    out["zeros:minus_zero"] = (zeros, [None, -0.0, None])
    out["zeros:primary_plus_zero"] = (zeros, [0.0, None, None])
    out["zeros:primary_minus_zero"] = (zeros, [-0.0, None, None])
    out["zeros:just_below"] = (zeros, [down(0.0), down(0.0), down(0.0)])
    # ---- the mask's bits: entries 0, 63 and 64 of a long row fail (the first bit, the top bit, the next group's first) while
    # 1, 62, 65 and 127 pass, with rows for either select kernel in the same call and nothing cut or filtered behind them
    long = base["counts_long"]
    row = int(np.argmax(long.counts))
    assert long.counts[row] == 129
    rng = np.random.default_rng(99)
    table = rng.uniform(0.3, 1.0, long.n_cols)
    table[long.cols[row, [1, 62, 65, 127]]] = 0.9
    table[long.cols[row, [0, 63, 64]]] = 0.25
    for r in (1, 2, 3):                                     # short rows (1, 7 and 8 candidates) lose their first entry too
        table[long.cols[r, 0]] = 0.25
    assert len(set(long.cols[row, [0, 63, 64, 1, 62, 65, 127]]) | {long.cols[r, 0] for r in (1, 2, 3)}) == 10
    first = C.table_field(long.cols.shape[0], table, dtype, 0.25)
    bits_case = long._replace(fields=[first, long.fields[1]], threshold=-1.0, top_n=long.cols.shape[1])
    out["mask_bits:first_field"] = (bits_case, [None, 0.25, None])
    swapped = long._replace(fields=[long.fields[0], first], threshold=-1.0, top_n=long.cols.shape[1])
    out["mask_bits:last_field"] = (swapped, [None, None, 0.25])
    # the same bits set by the PRIMARY's floor: the carried scores of those entries lowered
    vals = long.vals.copy()
    vals[row, [0, 63, 64]] = 0.25
    for r in (1, 2, 3):
        vals[r, 0] = 0.25
    vals.setflags(write=False)
    out["mask_bits:primary"] = (long._replace(vals=vals, threshold=-1.0, top_n=long.cols.shape[1]), [0.25, None, None])
    # ---- the cut moves: top_n below the row, a floor takes entries out ahead of it
    for name in ("counts_long", "full_2048_top20", "weights_third_2"):
        s = scores_of(name)
        F = len(s) - 1
        out[f"{name}:cut_moves"] = (base[name]._replace(top_n=3), [None] * F + [_present(s[F], 0.6)])
    return out


@functools.lru_cache(maxsize=None)
def expected(dtype, name):
    """The statement on a floor case, computed once."""
    case, floors = floor_cases(dtype)[name]
    want = ref_rescore_floors(case, floors)
    for a in want:
        a.setflags(write=False)
    return want


# ------------------------------------------------------------------------------------------ what the cases hold
def census(dtype):
    """The edges the floor cases are built for, as flags and sets, found in the cases themselves."""
    dtype = np.dtype(dtype).type
    T = dtype
    flags, failed_entries, passed_entries, floored_counts = set(), set(), set(), set()
    for name, (case, floors) in floor_cases(dtype).items():
        rows, ent, j, scores = candidate_scores(case)
        F = len(scores) - 1
        W = [T(case.w0)] + [T(f.w) for f in case.fields]
        failed = refused(scores, floors, W, ent, T)
        c = C._combined(scores, W, T, None)
        with np.errstate(all="ignore"):
            above = c > T(case.threshold)
        has = [m is not None for m in floors]
        floored_counts.add(sum(has))
        if has[0] and not any(has[1:]):
            flags.add("primary_only")
        if has[F] and not any(has[:F]):
            flags.add("last_field_only")
        if all(has) and F == 7:
            flags.add("all_of_eight")
        if any(has) and not all(has) and sum(has) > 1:
            flags.add("none_mixed_in")
        for f, m in enumerate(floors):
            if m is None:
                continue
            s = scores[f]
            if (s == T(m)).any():
                flags.add("a_score_equal_to_its_floor")
            if np.isfinite(T(m)) and T(m) < np.finfo(dtype).max and (s == np.nextafter(T(m), T(np.inf))).any():
                flags.add("a_score_one_ulp_above_its_floor")
            if np.isnan(s).any():
                flags.add("a_nan_score_under_a_floor")
            if np.isposinf(s).any():
                flags.add("plus_inf_under_a_floor")
            if np.isneginf(s).any():
                flags.add("minus_inf_under_a_floor")
            if (s == 0).any() and T(m) == 0:
                flags.add("zero_against_a_zero_floor")
                flags.add("minus_zero_floor" if np.signbit(T(m)) else "plus_zero_floor")
            if (np.signbit(s) & (s == 0)).any():
                flags.add("minus_zero_score_under_a_floor")
        for f in range(1, F + 1):                           # a NaN the data makes, on a field without a floor, before one with
            if floors[f] is None and np.isnan(scores[f]).any() and any(has[f + 1:]):
                flags.add("a_data_nan_ahead_of_a_floored_field")
        if (above & failed).any():
            flags.add("only_a_floor_refuses")
        if (~above & ~failed & ~np.isnan(c)).any():
            flags.add("a_floor_passes_and_the_threshold_refuses")
        plain = C.ref_rescore(case)
        want = expected(dtype, name)
        if ((plain[2] > 0) & (want[2] == 0)).any():
            flags.add("a_floor_empties_a_row")
        for r in range(case.cols.shape[0]):
            before, after = set(plain[0][r, :plain[2][r]]), set(want[0][r, :want[2][r]])
            if after - before:
                flags.add("the_cut_moves")
        cnt = case.counts[rows]
        if (failed & (cnt > ROW_CHUNK)).any() and (failed & (cnt <= ROW_CHUNK)).any() and case.cols.shape[1] > ROW_CHUNK:
            flags.add("failures_on_rows_of_both_select_kernels")
        long = cnt > ROW_CHUNK
        failed_entries |= set(int(e) for e in ent[failed & long])
        passed_entries |= set(int(e) for e in ent[~failed & long & above])
    return dict(flags=flags, failed_entries=failed_entries, passed_entries=passed_entries, floored_counts=floored_counts)
