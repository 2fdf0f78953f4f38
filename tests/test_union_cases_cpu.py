"""CPU tests of the cases sg_topn_union is held to (tests/_union_cases.py): a census proves that every edge the kernels have is
present, and every wrong turn a kernel could take changes the answer on at least one case -- so the GPU test that holds the
kernels to ``ref_union`` bit for bit can tell them apart."""
import numpy as np
import pytest

from tests import _union_cases as U

DTYPES = U.DTYPES


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_census_finds_every_edge(dtype):
    seen = U.census(dtype)
    assert seen["n_parts"] >= {2, 3, 8}
    assert seen["strides"] >= {1, 10, 64, 65, 1024} and (1024, 1024) in seen["stride_lists"]
    assert seen["union_sizes"] >= {0, 1, 63, 64, 65, 2047, 2048}
    assert seen["totals"] >= {0, 1, 63, 64, 65, 2048}                       # entries of a row: either side of the kernels' border
    assert seen["fill_row_lengths"] >= {0, 1, 7, 8, 9, 16, 17, 64, 65}
    assert seen["dead_lengths"] >= {0, 1, 32}
    many = U.cases(dtype)["many_long_rows"]                                 # a block of the long-row kernel takes several rows
    assert sum(U.counted(p) for p in many.parts).min() > U.SHORT and many.parts[0].cols.shape[0] == U.MANY_LONG_ROWS > 256 * 8
    sides = ("left", "right")
    assert seen["flags"] >= {"a_row_empty_in_part_0_alone", "a_row_empty_in_every_part", "a_count_above_the_stride",
                             "a_negative_count", "rows_for_both_kernels", "more_long_rows_than_blocks", "last_wave_partly_filled",
                             "last_block_partly_filled", "identical_rows_nothing_to_fill", "disjoint_rows",
                             "a_shared_column_whose_bits_differ", "columns_0_and_last", "a_part_names_a_column_twice",
                             "a_part_names_a_column_twice_part_0", "same_handle", "match_in_first_chunk_only",
                             "match_in_last_chunk_only", "no_common_column", "dead_first_and_last", "dead_on_one_side_only"}
    assert seen["flags"] >= {"part_0_holds_" + what for what in ("nan", "plus_inf", "minus_inf", "plus_zero", "minus_zero", "denormal")}
    assert seen["flags"] >= {f"dead_{where}_a_filled_row_{side}" for side in sides
                             for where in ("just_before", "at_the_number_of", "just_after")}


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_statement_on_rows_small_enough_to_read(dtype):
    T = np.dtype(dtype).type
    cols, vals, counts = U.expected(dtype, "named_twice")
    case = U.cases(dtype)["named_twice"]
    assert list(counts) == [4, 3] and cols.shape == (2, 4)                  # the stride is the longest row
    assert list(cols[0]) == [3, 7, 9, 12] and list(cols[1, :3]) == [3, 7, 9]
    assert vals[0, 1] == T(0.7) and vals[0, 0] == T(0.3) and vals[0, 3] == T(0.1)   # part 0's bits, the lowest place's
    fld = case.primary
    assert vals[0, 2] == U.ref_pairs_dot(fld.A, fld.B, [0], [9])[0]         # found by part 1 alone: the primary field's score
    assert vals[1, 0] == T(0.4)
    cols, vals, counts = U.expected(dtype, "special_values")                # special values are carried as they are
    p0 = U.cases(dtype)["special_values"].parts[0]
    for j, v in zip(p0.cols[0], p0.vals[0]):
        assert U.bits(vals[0, list(cols[0, :counts[0]]).index(j)][None])[0] == U.bits(np.array([v]))[0]
    cols, vals, counts = U.expected(dtype, "identical_parts")
    p0 = U.cases(dtype)["identical_parts"].parts[0]
    assert np.array_equal(counts, p0.counts) and all(set(cols[r, :counts[r]]) == set(p0.cols[r, :counts[r]]) for r in range(len(counts)))
    empty = U.UnionCase([U.part_of([([], [])], 3, T, 5)] * 2, 5, U._table(np.random.default_rng(0), 1, 5, T))
    cols, vals, counts = U.ref_union(empty)
    assert cols.shape == (1, 1) and list(counts) == [0]                     # at least 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", U.WRONG)
def test_every_wrong_turn_changes_an_answer(dtype, variant):
    cs = U.cases(dtype)
    by_size = sorted(cs, key=lambda name: int(sum(U.counted(p).sum() for p in cs[name].parts)))
    assert any(not U.same_result(U.ref_union(cs[name], variant), U.expected(dtype, name)) for name in by_size), variant


def test_the_reference_is_deterministic_and_reads_only():
    case = U.cases(np.float32)["two_parts_short"]
    before = [a.copy() for p in case.parts for a in p]
    assert U.same_result(U.ref_union(case), U.ref_union(case))
    assert all(np.array_equal(a, b) for a, b in zip(before, [a for p in case.parts for a in p]))
