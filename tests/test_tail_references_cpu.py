"""The inputs and references of tests/_tail_cases.py, checked without a GPU.  For every builder: the plain reference agrees
with the host code the project already trusts (StringGrouper._group_reps_on_host, the host branch of
_best_master_positions, oracle.zip_sp_matmul_topn), and every mutant that applies to the input -- the same reference with
one thing wrong -- gives a different answer.  The second half is a condition on the INPUTS: tests/test_tail_gpu.py feeds
them to the kernels, and an input that cannot tell a mutant from the reference could not tell a wrong kernel either."""
import types

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from oracle import oracle as O
from string_grouper_amd.string_grouper import GROUP_REP_CENTROID, GROUP_REP_FIRST, StringGrouper
from tests import _tail_cases as T


def same_topn(a: T.TopN, b: T.TopN) -> bool:
    mask = np.arange(a.cols.shape[1])[None, :] < a.counts[:, None]
    return a.cols.shape == b.cols.shape and np.array_equal(a.counts, b.counts) and \
        np.array_equal(a.cols[mask], b.cols[mask]) and np.array_equal(a.vals[mask], b.vals[mask])


def rows_that_differ(a: T.TopN, b: T.TopN) -> int:
    mask = np.arange(a.cols.shape[1])[None, :] < a.counts[:, None]
    return int(((a.counts != b.counts) | ((a.cols != b.cols) & mask).any(axis=1) | ((a.vals != b.vals) & mask).any(axis=1)).sum())


def host_stub(ml: T.CsrList, n_dupes=0, group_rep=GROUP_REP_FIRST):
    """What the two host reductions of StringGrouper read from `self`.  The similarity column of a match list is float64
    whatever the value type of the multiply (the reference stacks its blocks with dtype=np.float64, string_grouper.py:750)."""
    frame = pd.DataFrame({"master_side": T.rows_of(ml), "dupe_side": ml.cols.astype(np.int64),
                          "similarity": ml.vals.astype(np.float64)})
    return types.SimpleNamespace(_matches_list=frame, _duplicates=range(n_dupes), _config=types.SimpleNamespace(group_rep=group_rep))


# ---------------------------------------------------------------------------------------------------- zip
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", [n for n in T.ZIP_CASES if n != "reversed"])
def test_zip_reference_equals_oracle(name, dtype):
    case = T.zip_case(name, dtype)
    assert np.array_equal(case.offsets, np.concatenate([[0], np.cumsum([p.n_cols for p in case.parts])])[:-1])
    mats = [T.list_to_csr(T.topn_to_list(p), (len(p.counts), p.n_cols)) for p in case.parts]
    for top_n in T.ZIP_TOP_N + (1000,):
        want = O.zip_sp_matmul_topn(top_n, mats)
        ref = T.ref_zip(case, top_n)
        got = T.topn_to_list(ref)
        assert ref.cols.shape[1] == min(top_n, sum(p.cols.shape[1] for p in case.parts))
        assert want.shape == (len(ref.counts), case.n_cols) and want.dtype == got.vals.dtype
        assert np.array_equal(want.indptr, got.row_ptr) and np.array_equal(want.indices, got.cols)
        assert np.array_equal(want.data, got.vals)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_zip_inputs_reach_every_pass_and_edge(dtype):
    """Rows empty everywhere, a part without entries, rows filled beyond 64 in one part, top_n above all strides."""
    for name in T.ZIP_CASES:
        case = T.zip_case(name, dtype)
        total = sum(p.counts.astype(np.int64) for p in case.parts)
        assert total.max() > 128 and (name == "straddle" or (total == 0).any())
        assert 1000 > sum(p.cols.shape[1] for p in case.parts) > 200
    assert any((p.counts > 64).any() for n in ("parts1", "parts2", "parts5", "parts9") for p in T.zip_case(n, dtype).parts)
    assert any((p.counts == 0).all() for p in T.zip_case("parts5", dtype).parts)
    assert [len(T.zip_case(f"parts{k}", dtype).parts) for k in (1, 2, 5, 9)] == [1, 2, 5, 9]
    assert T.zip_case("reversed", dtype).offsets[0] == T.zip_case("reversed", dtype).offsets.max()


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_zip_equal_scores_straddle_both_pass_boundaries(dtype):
    """In 'straddle' most rows have equal scores on both sides of entry 64 and of entry 128, from more than one part; the
    mutant that resumes a pass below the floor's score without its column loses entries there, and only there."""
    case = T.zip_case("straddle", dtype)
    ref = T.ref_zip(case, 200)
    across64 = ref.vals[:, 63] == ref.vals[:, 64]
    across128 = ref.vals[:, 127] == ref.vals[:, 128]
    assert across64.sum() >= 75 and across128.sum() >= 75
    widths = np.cumsum([p.n_cols for p in case.parts])
    part_of = np.searchsorted(widths, ref.cols, side="right")
    assert (part_of[across64, 63] != part_of[across64, 64]).sum() >= 20      # the run continues in another part
    for top_n in (65, 127, 128, 129, 200):
        assert rows_that_differ(ref, T.mutant_zip_forgets_floor_column(case, 200)) >= 75
        assert rows_that_differ(T.ref_zip(case, top_n), T.mutant_zip_forgets_floor_column(case, top_n)) >= 75
    for top_n in (1, 6, 63, 64):                                               # one pass: no floor to forget
        assert same_topn(T.ref_zip(case, top_n), T.mutant_zip_forgets_floor_column(case, top_n))
    for name in ("parts1", "parts2", "parts5", "parts9"):                      # the levelled scores cross the boundaries as well
        mixed = T.zip_case(name, dtype)
        assert rows_that_differ(T.ref_zip(mixed, 200), T.mutant_zip_forgets_floor_column(mixed, 200)) >= 10


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_zip_unsorted_parts_tell_arrival_order_from_column_order(dtype):
    case = T.zip_case("unsorted", dtype)
    for top_n in (63, 64, 65, 127, 128, 129, 200):
        assert rows_that_differ(T.ref_zip(case, top_n), T.mutant_zip_arrival_order(case, top_n)) >= 20
    rev = T.zip_case("reversed", dtype)        # parts in descending column order: arrival order is not column order either
    assert rows_that_differ(T.ref_zip(rev, 64), T.mutant_zip_arrival_order(rev, 64)) >= 20
    srt = T.zip_case("parts5", dtype)          # sorted parts in ascending column order arrive in column order: no difference
    assert same_topn(T.ref_zip(srt, 64), T.mutant_zip_arrival_order(srt, 64))


# ---------------------------------------------------------------------------------------------------- match list
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", T.MATCHLIST_SQUARE)
def test_matchlist_reference_equals_host_post_processing(name, dtype):
    """The lil sequence of the reference gives what the project's own host formulation (coo / unique, no lil) gives."""
    t = T.matchlist_case(name, dtype)
    n = len(t.counts)
    for fix, sym in ((False, True), (True, False), (True, True)):
        m = T.list_to_csr(T.topn_to_list(t), (n, n))
        if fix:
            m = StringGrouper._fix_diagonal(m)
        if sym:
            m = StringGrouper._symmetrize_matrix(m)
        m = sp.csr_matrix(m)
        m.sort_indices()
        ref = T.ref_matchlist(t, fix, sym, False)
        assert ref.vals.dtype == dtype and ref.row_ptr.dtype == np.int64 and ref.cols.dtype == np.int32
        assert np.array_equal(m.indptr, ref.row_ptr) and np.array_equal(m.indices, ref.cols) and np.array_equal(m.data, ref.vals)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_matchlist_inputs_hold_the_edges(dtype):
    sq = T.matchlist_case("square", dtype)
    ml = T.topn_to_list(sq)
    rows = T.rows_of(ml)
    stored = set(zip(rows.tolist(), ml.cols.tolist()))
    diag = rows == ml.cols
    assert diag.sum() > 100 and (ml.vals[diag] != 1).all()                    # stored diagonals that fix_diagonal must overwrite
    assert (sq.counts == 0).sum() >= 50 and (sq.counts == sq.cols.shape[1]).sum() >= 100
    mirrored = sum((c, r) in stored for r, c in stored if r != c)
    assert 0 < mirrored < len(stored) - diag.sum()                             # some pairs stored from both sides, most not
    value = dict(zip(zip(rows.tolist(), ml.cols.tolist()), ml.vals.tolist()))
    assert all(value[(r, c)] == value[(c, r)] for r, c in stored if (c, r) in stored)   # K6's precondition
    # the flags change the list, each in its own way
    lists = {f: T.ref_matchlist(sq, *f, False) for f in ((False, False), (True, False), (False, True), (True, True))}
    assert len({len(v.cols) for v in lists.values()}) == 4
    assert not np.array_equal(T.ref_matchlist(sq, False, False, True).cols, lists[(False, False)].cols)
    hub = T.matchlist_case("hub", dtype)
    assert hub.cols.shape == (20002, 3) and (T.topn_to_list(hub).cols == 20001).sum() == 20002
    grown = np.diff(T.ref_matchlist(hub, False, True, False).row_ptr)
    assert grown[20001] == 20002 and hub.counts[20001] == 2
    wide = T.matchlist_case("wide", dtype)
    assert wide.n_cols != len(wide.counts)
    assert not np.array_equal(T.ref_matchlist(wide, False, False, True).cols, T.ref_matchlist(wide, False, False, False).cols)


# ---------------------------------------------------------------------------------------------------- best master
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", T.BEST_MASTER_CASES)
def test_best_master_reference_equals_host_branch_and_ties_matter(name, dtype):
    t = T.best_master_case(name, dtype)
    ml = T.topn_to_list(t)
    ref = T.ref_best_master(ml, t.n_cols)
    host = StringGrouper._best_master_positions(host_stub(ml, n_dupes=t.n_cols))
    assert ref.dtype == np.int32 and ref.shape == (t.n_cols,) and np.array_equal(ref, host)
    if name == "norows":
        assert (ref == -1).all()
        return
    assert (ref == -1).sum() >= (2000 if name == "wide" else 0)               # columns nobody names
    assert (ref != T.mutant_best_master_highest_row(ml, t.n_cols)).sum() >= (500 if name == "wide" else 6)
    # the maximum of a column and its runner-up differ in the last bit: a comparison that drops it picks another row
    coarse = T.CsrList(ml.row_ptr, ml.cols, np.round(ml.vals.astype(np.float64), 3).astype(dtype))
    assert (ref != T.ref_best_master(coarse, t.n_cols)).sum() >= (500 if name == "wide" else 5)


# ---------------------------------------------------------------------------------------------------- group representatives
# Every length of BOUNDARY_RESTS is swept for both value types on the GPU; the conditions below leave out
#   float64, rest 0 and 1: a row of one or two values has one summation order (and rest < 7 is numpy's sequential branch);
#   float32, rest 0: a single value is never rounded, so accumulating in float32 cannot show.
@pytest.mark.parametrize("rest", T.BOUNDARY_RESTS)
def test_centroid_sweep_float64_tells_the_summation_order(rest):
    case = T.centroid_sweep_case(rest, np.float64)
    ml = T.topn_to_list(case.topn)
    n = len(case.topn.counts)
    ref = T.ref_group_reps(ml, n, True)
    host = StringGrouper._group_reps_on_host(host_stub(ml, group_rep=GROUP_REP_CENTROID), n)
    assert np.array_equal(ref, host)
    a, b = case.sweep_pairs[:, 0], case.sweep_pairs[:, 1]
    assert len(a) == T.SWEEP_COMPONENTS and ((ref[a] == a) | (ref[a] == b)).all() and np.array_equal(ref[a], ref[b])
    assert (case.topn.counts[a] == rest + 1).all() and (case.topn.counts[b] == rest + 1).all()
    assert case.topn.counts.sum() == 2 * T.SWEEP_COMPONENTS * (rest + 1)        # nobody else has a row: two candidates
    if rest >= 7:
        changed = (ref[a] != T.mutant_reps_left_to_right(ml, n)[a]).sum()
        assert changed >= T.SWEEP_COMPONENTS // 4, f"rest {rest}: only {changed} components tell left-to-right from numpy's order"
    # a component's lowest index is a column node, not a candidate, in most components: 'first' and 'centroid' differ
    first = T.ref_group_reps(ml, n, False)
    assert np.array_equal(first, StringGrouper._group_reps_on_host(host_stub(ml), n))
    assert (first[a] != ref[a]).sum() >= (T.SWEEP_COMPONENTS // 2 if rest >= 7 else 0)
    assert (first == np.arange(n)).sum() > T.SWEEP_COMPONENTS                   # isolated nodes are their own group


@pytest.mark.parametrize("rest", T.BOUNDARY_RESTS)
def test_centroid_sweep_float32_tells_the_accumulator_and_the_tie_rule(rest):
    case = T.centroid_sweep_case(rest, np.float32)
    ml = T.topn_to_list(case.topn)
    n = len(case.topn.counts)
    assert ml.vals.dtype == np.float32
    ref = T.ref_group_reps(ml, n, True)
    assert np.array_equal(ref, StringGrouper._group_reps_on_host(host_stub(ml, group_rep=GROUP_REP_CENTROID), n))
    a, b = case.sweep_pairs[:, 0], case.sweep_pairs[:, 1]
    tie, raised = np.arange(len(a)) % 2 == 0, np.arange(len(a)) % 2 == 1
    assert np.array_equal(ref[a[tie]], np.minimum(a, b)[tie])                   # exact tie: the lower index
    assert np.array_equal(ref[a[raised]], b[raised])                            # one ulp more: that candidate
    assert (ref[a] != T.mutant_reps_highest_index(ml, n)[a]).sum() == tie.sum()
    if rest >= 1:
        changed = (ref[a] != T.mutant_reps_float32_sum(ml, n)[a]).sum()
        assert changed >= 10, f"rest {rest}: only {changed} components tell a float32 accumulator from float64"
    assert np.array_equal(ref, T.mutant_reps_left_to_right(ml, n))              # exact sums: the order cannot show (issue, point 1)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", T.GRAPH_CASES)
def test_graph_reference_equals_host_and_needs_weak_connectivity(name, dtype):
    case = T.graph_case(name, dtype)
    ml = T.topn_to_list(case.topn)
    n = len(case.topn.counts)
    for centroid, rep in ((False, GROUP_REP_FIRST), (True, GROUP_REP_CENTROID)):
        ref = T.ref_group_reps(ml, n, centroid)
        assert ref.dtype == np.int32 and np.array_equal(ref, StringGrouper._group_reps_on_host(host_stub(ml, group_rep=rep), n))
        assert (ref != T.mutant_reps_strong(ml, n, centroid)).sum() >= n // 4   # one-directional edges: strong connectivity splits
    first = T.ref_group_reps(ml, n, False)
    if name.startswith("path"):
        assert (first == 0).all()
    if name.startswith("stars"):
        assert np.array_equal(np.unique(first), np.arange(400) * 31)            # the lowest index of a star is a leaf
    if name == "small":
        assert len(np.unique(first)) == 3000 + 3000 + 500
        centroid = T.ref_group_reps(ml, n, True)
        changed = (centroid != T.mutant_reps_highest_index(ml, n)).sum()
        assert changed >= 2 * 3000                                              # every two-node component is a tie


# ---------------------------------------------------------------------------------------------------- row-wise dot
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_rowwise_dot_inputs_tell_kept_zeros_and_the_order(dtype):
    case = T.dot_case(dtype)
    a, b = case.a, case.b
    assert a.dtype == dtype and b.dtype == dtype and a.has_canonical_format and b.has_canonical_format
    ref = T.ref_rowwise_dot(a, b)
    assert ref.dtype == dtype and ref.shape == (a.shape[0],)
    kept = np.diff(a.multiply(b).indptr)                                       # non-zero products per row
    assert set(r + 1 for r in T.BOUNDARY_RESTS) | {0} <= set(kept.tolist())
    common = np.array([len(np.intersect1d(a[i].indices, b[i].indices)) for i in range(a.shape[0])])
    assert (common[case.zero_rows] > kept[case.zero_rows]).all()               # products that underflowed to exactly 0
    assert np.array_equal(np.flatnonzero(common > kept), case.zero_rows)       # ... and nowhere else: subnormal ones are kept
    tiny = np.finfo(dtype).tiny
    subnormal_sum = (ref != 0) & (np.abs(ref) < tiny)
    assert subnormal_sum.sum() >= len(T.BOUNDARY_RESTS)                        # the all-subnormal rows
    prods = a.multiply(b)
    assert ((prods.data != 0) & (np.abs(prods.data) < tiny)).sum() > 100 and (np.abs(prods.data) >= tiny).sum() > 1000
    assert (np.diff(a.indptr) == 0).sum() == 2 and (np.diff(b.indptr) == 0).sum() == 2 and (common == 0).sum() >= 7
    # the mutants
    zeros_kept = T.mutant_dot_keeps_zero_products(a, b)
    differ = np.flatnonzero(zeros_kept != ref)
    assert len(differ) >= 5 and set(differ.tolist()) <= set(case.zero_rows.tolist())
    sequential = T.mutant_dot_left_to_right(a, b)
    assert (sequential != ref).sum() >= 20
    assert np.array_equal(sequential[kept < 3], ref[kept < 3])                 # one or two products: there is one order


# ---------------------------------------------------------------------------------------------------- row costs
def test_row_cost_inputs():
    rep, long, dis = T.cost_case("repeats"), T.cost_case("repeats_long"), T.cost_case("distinct")
    assert rep.b.shape == long.b.shape == dis.b.shape == (9000, 300) and rep.a.shape == (700, 300)
    assert T.distinct_rows(rep.b).shape[0] == T.distinct_rows(long.b).shape[0] == 3000 and T.distinct_rows(dis.b).shape[0] == 9000
    norm2 = lambda m: np.asarray(m.multiply(m).sum(axis=1, dtype=np.float64)).ravel()
    assert norm2(rep.b).max() <= 1.00001 and norm2(dis.b).max() <= 1.00001 and norm2(long.b).min() > 8   # cosine-like or not
    full, grouped = T.ref_row_costs(rep.a, rep.b), T.ref_row_costs(rep.a, T.distinct_rows(rep.b))
    assert full.dtype == np.int64 and np.array_equal(full, 3 * grouped) and (grouped > 0).sum() == 560
    empty = np.diff(rep.a.indptr) == 0
    assert empty.sum() == 140 and (full[empty] == 0).all() and (full[~empty] > 0).all()
    # the definition, spelled out for one row
    i = 3
    assert full[i] == sum((rep.b[:, k] != 0).sum() for k in rep.a[i].indices)
