"""What sg_matchlist_field_scores (csrc/sg_matchlist_fields.hip) is held to, for the CPU and the GPU tests alike.  TEST
INFRASTRUCTURE ONLY.

- ``ref_list_fields``: the statement in numpy -- plane f of a list ``(row_ptr, cols)`` is ``ref_pairs_dot`` of field f on the
  PHYSICAL rows of every entry's live pair (row of the entry, its column), in list order -- or, with a ``variant``, one of the
  wrong turns a kernel that walks runs of 64 consecutive entries could take;
- ``cases(dtype)``: lists built where that walk can go wrong (empty rows, runs that end at a row's end or span several rows, a
  hub row, totals around a multiple of 64, 0 and 1 entries, 1 and 8 fields, a self-join, dead lists around the named rows);
- ``census``: which edge each case holds, counted from the case itself."""
import functools
from collections import namedtuple

import numpy as np

from tests._pair_cases import _structured_rows, csr_of, ref_pairs_dot
from tests._rescore_cases import DTYPES, Field, _without_last_chunk, physical, table_field  # noqa: F401

RUN = 64                                                   # SG_PAIR_ROW_CHUNK: entries a group walks
HUB = 2100
ListCase = namedtuple("ListCase", "row_ptr cols n_cols fields")      # fields: Field(A, B, w, dead_a, dead_b); A is B: a self-join
WRONG = ("row_side_left", "run_row_kept", "swapped", "dead_ignored", "side_left", "last_chunk_lost")


# ------------------------------------------------------------------------------------------ the statement
def rows_of_entries(row_ptr, n_entries, variant=None):
    """The row of entry q is the LAST row whose pointer is <= q: empty rows in front of it share that pointer."""
    q = np.arange(n_entries, dtype=np.int64)
    n_rows = len(row_ptr) - 1
    if variant == "row_side_left":                          # the FIRST row whose pointer is >= q
        return np.clip(np.searchsorted(row_ptr, q, side="left"), 0, max(n_rows - 1, 0))
    rows = np.searchsorted(row_ptr, q, side="right") - 1
    if variant == "run_row_kept":                           # the row of a run's first entry, for the whole run
        rows = rows[(q // RUN) * RUN]
    return rows


def ref_list_fields(case: ListCase, variant=None) -> np.ndarray:
    """[fields, entries] of the statement -- or of one wrong turn."""
    cols = np.asarray(case.cols, np.int64)
    rows = rows_of_entries(np.asarray(case.row_ptr, np.int64), len(cols), variant)
    T = case.fields[0].A.dtype.type
    out = np.zeros((len(case.fields), len(cols)), T)
    for f, fld in enumerate(case.fields):
        A, B = fld.A, fld.B
        if variant == "last_chunk_lost":
            A = _without_last_chunk(A)
        side = "left" if variant == "side_left" else "right"
        dead_a, dead_b = (None, None) if variant == "dead_ignored" else (fld.dead_a, fld.dead_b)
        a, b = physical(dead_a, rows, side), physical(dead_b, cols, side)
        if variant == "swapped":
            a, b = b, a
        a, b = np.minimum(a, A.shape[0] - 1), np.minimum(b, B.shape[0] - 1)   # (a wrong turn may step outside: the last row then)
        out[f] = ref_pairs_dot(A, B, a, b)
    return out


# ------------------------------------------------------------------------------------------ building blocks
def _list(rng, counts, n_cols):
    """Rows of ``counts`` distinct random columns each, ascending inside a row (as K6 leaves them)."""
    row_ptr = np.r_[0, np.cumsum(counts)].astype(np.int64)
    cols = [np.sort(rng.choice(n_cols, c, replace=False)) for c in counts]
    return row_ptr, np.concatenate(cols + [np.zeros(0, np.int64)]).astype(np.int32)


def _rows(rng, n, dtype, universe=24):
    """n sparse rows over a small universe: lengths around a chunk of eight, so that any two rows share columns and every
    row differs from every other."""
    out = []
    for _ in range(n):
        k = int(rng.choice([0, 1, 3, 7, 8, 9, 17]))
        out.append((np.sort(rng.choice(universe, k, replace=False)), rng.uniform(0.25, 1.0, k).astype(dtype)))
    return out


def mixed_field(rng, n_left, n_right, dtype, dead_a=None, dead_b=None, self_join=False):
    """A field whose score depends on the left AND the right row.  Dead physical rows are rows like any other: a wrong row
    map reads another row's values."""
    dead_a = None if dead_a is None else np.asarray(dead_a, np.int64)
    dead_b = None if dead_b is None else np.asarray(dead_b, np.int64)
    A = csr_of(_rows(rng, n_left + (0 if dead_a is None else len(dead_a)), dtype), dtype, 24)
    if self_join:
        return Field(A, A, 1.0, dead_a, dead_a)
    B = csr_of(_rows(rng, n_right + (0 if dead_b is None else len(dead_b)), dtype), dtype, 24)
    return Field(A, B, 1.0, dead_a, dead_b)


def structured_field(rng, n_left, n_right, dtype):
    """The rows of tests/_pair_cases.py's structured pairs (common columns at the ends of chunks), repeated to the shape."""
    a_rows, b_rows, _ = _structured_rows(rng, dtype)
    n_cols = 1 + max(int(c.max()) for c, _ in a_rows + b_rows if len(c))
    return Field(csr_of([a_rows[i % len(a_rows)] for i in range(n_left)], dtype, n_cols),
                 csr_of([b_rows[j % len(b_rows)] for j in range(n_right)], dtype, n_cols), 1.0, None, None)


# ------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def _cases(dtype):
    T = dtype
    rng = np.random.default_rng(9300 + np.dtype(dtype).itemsize)
    out = {}

    def add(name, counts, n_cols, fields):
        row_ptr, cols = _list(rng, counts, n_cols)
        out[name] = ListCase(row_ptr, cols, n_cols, fields(len(counts), n_cols))

    def two(R, N):
        return [mixed_field(rng, R, N, T), structured_field(rng, R, N, T)]

    add("empty_rows_before_between_after", [0, 0, 3, 0, 0, 5, 0, 1, 0, 0], 40, two)
    add("runs_end_at_a_row_s_end", [64, 64, 10, 54, 1], 80, two)
    add("a_run_spans_three_rows", [60, 2, 0, 1, 5, 70, 0, 3], 90, two)
    add("hub_row", [3, HUB, 0, 4], HUB + 7, lambda R, N: [mixed_field(rng, R, N, T)])
    for total in (63, 64, 65, 127, 128, 129):               # entries n * 64 - 1, n * 64, n * 64 + 1
        counts = rng.multinomial(total, np.ones(9) / 9)
        add(f"total_{total}", counts, 70, lambda R, N: [mixed_field(rng, R, N, T)])
    add("no_entries", [0, 0, 0, 0, 0], 9, two)
    add("one_entry", [0, 0, 1, 0], 9, two)
    add("one_field", [4, 0, 9, 70, 1], 100, lambda R, N: [mixed_field(rng, R, N, T)])
    add("eight_fields", [4, 0, 9, 70, 1], 100,
        lambda R, N: [mixed_field(rng, R, N, T) for _ in range(6)] + [structured_field(rng, R, N, T),
                                                                        table_field(R, rng.uniform(0.1, 1.0, N), T, 1.0)])
    n = 30
    add("self_join", [int(x) for x in rng.integers(0, 12, n)], n, lambda R, N: [mixed_field(rng, R, N, T, self_join=True)])
    add("self_join_with_dead_rows", [int(x) for x in rng.integers(0, 12, n)], n,
        lambda R, N: [mixed_field(rng, R, N, T, dead_a=[0, 7, 8, 31], self_join=True)])
    # dead physical rows before, AT the place of and after the named rows, on either side: rows 2, 5 and 6 hold the entries
    counts = [0, 0, 6, 0, 0, 20, 3, 0]
    add("dead_left", counts, 40, lambda R, N: [mixed_field(rng, R, N, T, dead_a=[0, 2, 3, 6, 12]), table_field(R, rng.uniform(0.1, 1.0, N), T, 1.0, dead_a=[5])])
    add("dead_right", counts, 40, lambda R, N: [mixed_field(rng, R, N, T, dead_b=[0, 1, 5, 11, 44]), table_field(R, rng.uniform(0.1, 1.0, N), T, 1.0, dead_b=[0, 3, 4])])
    add("dead_both_sides_differ", counts, 40, lambda R, N: [mixed_field(rng, R, N, T, dead_a=[1, 2, 8], dead_b=[0, 19, 20]),
                                                            mixed_field(rng, R, N, T, dead_a=[5], dead_b=[2, 3, 4, 5])])
    return out


def cases(dtype):
    """name -> ListCase."""
    return _cases(np.dtype(dtype).type)


@functools.lru_cache(maxsize=None)
def _expected(dtype, name):
    return ref_list_fields(_cases(dtype)[name])


def expected(dtype, name) -> np.ndarray:
    """The statement of a case, computed once and shared: do not write into it."""
    return _expected(np.dtype(dtype).type, name)


def census(dtype) -> dict:
    """edge -> the cases that hold it, read off the cases themselves."""
    found = {}

    def note(edge, name):
        found.setdefault(edge, []).append(name)

    for name, case in cases(dtype).items():
        row_ptr, cols = np.asarray(case.row_ptr), case.cols
        counts, M = np.diff(row_ptr), len(case.cols)
        filled = np.flatnonzero(counts)
        if M and filled[0] > 0:
            note("empty rows before", name)
        if M and filled[-1] < len(counts) - 1:
            note("empty rows after", name)
        if M and (counts[filled[0]:filled[-1]] == 0).any():
            note("empty rows between", name)
        ends = row_ptr[1:][counts > 0]
        if M > RUN and any(e % RUN == 0 and e < M for e in ends):
            note("a run ends at a row's end", name)
        rows = rows_of_entries(row_ptr, M)
        if any(len(np.unique(rows[q:q + RUN])) >= 3 for q in range(0, M, RUN)):
            note("a run spans three rows", name)
        if counts.max(initial=0) >= HUB:
            note("hub row", name)
        for d in (-1, 0, 1):
            if M > RUN and (M - d) % RUN == 0:
                note(f"n * 64 {d:+d} entries", name)
        if M in (0, 1):
            note(f"{M} entries", name)
        if len(case.fields) in (1, 8):
            note(f"{len(case.fields)} fields", name)
        for fld in case.fields:
            if fld.A is fld.B:
                note("self-join", name)
            for side, dead, named in (("left", fld.dead_a, rows), ("right", fld.dead_b, cols)):
                if dead is None or not M:
                    continue
                phys = physical(dead, np.unique(named))
                if (dead < phys.min()).any():
                    note(f"dead {side} before", name)
                if (dead > phys.max()).any():
                    note(f"dead {side} after", name)
                if np.isin(dead, np.unique(named)).any():     # the live number of a named row is a dead physical row's
                    note(f"dead {side} at", name)
    return found


EDGES = (["empty rows before", "empty rows between", "empty rows after", "a run ends at a row's end", "a run spans three rows",
          "hub row", "n * 64 -1 entries", "n * 64 +0 entries", "n * 64 +1 entries", "0 entries", "1 entries", "1 fields", "8 fields",
          "self-join"] + [f"dead {side} {where}" for side in ("left", "right") for where in ("before", "at", "after")])
