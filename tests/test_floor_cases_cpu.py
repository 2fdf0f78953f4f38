"""CPU tests of the cases sg_topn_rescore with floors is held to (tests/_floor_cases.py): a census proves that every edge of the
floor mask is present, and every wrong turn the mask could take changes the answer on at least one case -- so the GPU test that
holds the kernel to ``ref_rescore_floors`` bit for bit can tell them apart."""
import numpy as np
import pytest

from tests import _floor_cases as FC
from tests import _rescore_cases as C

DTYPES = C.DTYPES


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_census_finds_every_edge(dtype):
    seen = FC.census(dtype)
    assert seen["flags"] >= {"primary_only", "last_field_only", "all_of_eight", "none_mixed_in", "a_score_equal_to_its_floor",
                             "a_score_one_ulp_above_its_floor", "a_nan_score_under_a_floor", "plus_inf_under_a_floor",
                             "minus_inf_under_a_floor", "zero_against_a_zero_floor", "plus_zero_floor", "minus_zero_floor",
                             "minus_zero_score_under_a_floor", "a_data_nan_ahead_of_a_floored_field", "only_a_floor_refuses",
                             "a_floor_passes_and_the_threshold_refuses", "a_floor_empties_a_row", "the_cut_moves",
                             "failures_on_rows_of_both_select_kernels"}
    assert seen["floored_counts"] >= {1, 3, 8}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["mask_bits:first_field", "mask_bits:last_field", "mask_bits:primary"])
def test_the_mask_s_first_bit_its_top_bit_and_the_next_group_s_first(dtype, name):
    case, floors = FC.floor_cases(dtype)[name]
    T = np.dtype(dtype).type
    rows, ent, j, scores = FC.candidate_scores(case)
    W = [T(case.w0)] + [T(f.w) for f in case.fields]
    failed = FC.refused(scores, floors, W, ent, T)
    row = int(np.argmax(case.counts))
    assert case.counts[row] == 129 and case.cols.shape[1] == 129
    gone = set(int(e) for e in ent[failed & (rows == row)])
    assert {0, 63, 64} <= gone and not gone & {1, 62, 65, 127}
    short = [r for r in range(len(case.counts)) if 0 < case.counts[r] <= 64 and failed[rows == r].any()]
    assert len(short) >= 3                                                  # the short select kernel's rows in the same call
    cols, vals, counts = FC.expected(dtype, name)                           # nothing else hides them: no filter, no cut
    kept = set(int(x) for x in cols[row, :counts[row]])
    assert not kept & set(int(x) for x in case.cols[row, [0, 63, 64]])
    assert set(int(x) for x in case.cols[row, [1, 62, 65, 127]]) <= kept


@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_fails_and_one_ulp_below_passes(dtype):
    T = np.dtype(dtype).type
    cs = FC.floor_cases(dtype)
    case, floors = cs["counts_short:equal"]
    _, below = cs["counts_short:ulp_below"]
    m = T(floors[1])
    assert T(below[1]) == np.nextafter(m, T(-np.inf))
    rows, ent, j, scores = FC.candidate_scores(case)
    at = scores[1] == m
    assert at.any()
    W = [T(case.w0)] + [T(f.w) for f in case.fields]
    assert FC.refused(scores, floors, W, ent, T)[at].all() and not FC.refused(scores, below, W, ent, T)[at].any()
    assert not C.same_result(FC.expected(dtype, "counts_short:equal"), FC.expected(dtype, "counts_short:ulp_below"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(dtype):
    cols, vals, counts = FC.expected(dtype, "nan_inf:huge")                 # only the +inf of the first field is above it
    assert counts[0] == 2 and np.isposinf(vals[0, :2]).all() and counts[1] == 0
    plain = C.expected(dtype, "nan_inf")
    assert C.same_result(FC.expected(dtype, "nan_inf:lowest"), plain)       # (c drops the NaN and the -inf anyway)
    for name in ("zeros:plus_zero", "zeros:minus_zero"):                    # every score of that field is a zero
        assert FC.expected(dtype, name)[2][0] == 0
    for name in ("zeros:primary_plus_zero", "zeros:primary_minus_zero"):    # s_0 = +0.0, -0.0 and 0.25: the last one stays
        cols, vals, counts = FC.expected(dtype, name)
        assert counts[0] == 1 and cols[0, 0] == 4
    assert C.same_result(FC.expected(dtype, "zeros:just_below"), C.expected(dtype, "zeros"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_a_floor_the_statement_is_ref_rescore_s(dtype):
    for name, case in C.cases(dtype).items():
        if case.counts.sum() > 20000:
            continue
        assert C.same_result(FC.ref_rescore_floors(case, [None] * (len(case.fields) + 1)), C.expected(dtype, name)), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", FC.WRONG)
def test_every_wrong_turn_changes_an_answer(dtype, variant):
    cs = FC.floor_cases(dtype)
    by_size = sorted(cs, key=lambda name: int(cs[name][0].counts.sum()))
    assert any(not C.same_result(FC.ref_rescore_floors(*cs[name], variant), FC.expected(dtype, name)) for name in by_size), variant


def test_the_reference_is_deterministic_and_reads_only():
    case, floors = FC.floor_cases(np.float32)["counts_short:all"]
    before = [a.copy() for a in (case.cols, case.vals, case.counts)]
    assert C.same_result(FC.ref_rescore_floors(case, floors), FC.ref_rescore_floors(case, floors))
    assert all(np.array_equal(a, b) for a, b in zip(before, (case.cols, case.vals, case.counts)))
