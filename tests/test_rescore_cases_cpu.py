"""CPU tests of the cases sg_topn_rescore is held to (tests/_rescore_cases.py): a census proves that every edge the kernels
have is present, and every wrong turn a kernel could take changes the answer on at least one case -- so the GPU test that
holds the kernels to ``ref_rescore`` bit for bit can tell them apart."""
import numpy as np
import pytest

from tests import _rescore_cases as C

DTYPES = C.DTYPES


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_census_finds_every_edge(dtype):
    seen = C.census(dtype)
    assert seen["counts"] >= {0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129}
    assert seen["full_strides"] >= {10, 64, 65, C.MAX_STRIDE}
    assert seen["field_row_lengths"] >= {0, 1, 7, 8, 9, 16, 17, 64, 65}
    many = C.cases(dtype)["many_long_rows"]                                 # a block of the long-row kernel takes several rows
    assert np.count_nonzero(many.counts > 64) == C.MANY_LONG_ROWS > 256 * 8
    mixed = C.cases(dtype)["counts_long"]                                   # rows for either select kernel in one call
    assert (mixed.counts > 64).any() and (mixed.counts <= 64).any() and mixed.cols.shape[1] > 64
    assert seen["n_fields"] >= {1, 2, 7}
    assert seen["dead_lengths"] >= {0, 1, 32}
    assert seen["top_n"] >= {1, 10, 64, 65}
    assert seen["flags"] >= {"last_wave_partly_filled", "last_block_partly_filled", "match_in_first_chunk_only",
                             "match_in_last_chunk_only", "no_common_column", "same_handle", "dead_first_and_last",
                             "dead_just_before_a_named_row", "dead_at_the_number_of_a_named_row", "dead_just_after_a_named_row",
                             "dead_lists_differ_between_sides", "dead_lists_differ_between_fields",
                             "a_row_whose_entries_all_fail", "nothing_fails_and_k_covers_the_row"}


def _all_scores(case):
    """c of every candidate of a case, filter and cut apart."""
    everything = case._replace(threshold=-np.inf, top_n=case.cols.shape[1])
    return C.ref_rescore(everything)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scores_sit_at_the_threshold_and_one_ulp_to_either_side(dtype):
    case = C.cases(dtype)["threshold_exact"]
    T = np.dtype(dtype).type
    t = T(case.threshold)
    cols, vals, counts = _all_scores(case)
    c = vals[0, :counts[0]]
    assert np.count_nonzero(c == t) == 2                                    # (reached by two different sets of scores)
    assert np.nextafter(t, T(np.inf)) in c and np.nextafter(t, T(-np.inf)) in c
    cols, vals, counts = C.expected(dtype, "threshold_exact")
    assert counts[0] == 1 and vals[0, 0] == np.nextafter(t, T(np.inf))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 10, 64, 65])
def test_equal_scores_lie_across_the_cut_with_columns_against_the_candidate_order(dtype, k):
    case = C.cases(dtype)[f"ties_k{k}"]
    assert case.top_n == k
    cols, vals, counts = _all_scores(case)
    c, j = vals[0, :counts[0]], cols[0, :counts[0]]
    block = np.flatnonzero(c == c[k - 1])                                   # the ranks that share the cut's score
    assert block[0] <= max(k - 2, 0) and block[-1] >= k + 1 and len(block) == 5
    assert np.all(np.diff(j[block]) > 0)                                    # the statement's order: column ascending ...
    where = [int(np.flatnonzero(case.cols[0] == col)[0]) for col in j[block]]
    assert np.all(np.diff(where) < 0)                                       # ... the reverse of the candidates' order


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_are_in_the_cases(dtype):
    cs = C.cases(dtype)
    zeros = cs["zeros"]
    assert zeros.threshold < 0 and np.signbit(zeros.vals[0, 1]) and zeros.vals[0, 1] == 0 and not np.signbit(zeros.vals[0, 0])
    cols, vals, counts = C.expected(dtype, "zeros")
    assert counts[0] == 3 and list(cols[0]) == [4, 2, 7] and not np.signbit(vals[0, 1:]).any()   # +0.0 both, by column
    table = cs["nan_inf"].fields[0].B.data                                  # the first field's score of every column
    assert np.isnan(table).any() and np.isposinf(table).any() and np.isneginf(table).any()
    assert C.expected(dtype, "nan_inf")[2][0] == 4 < cs["nan_inf"].counts[0]                     # the NaN and the -inf fail
    cols, vals, counts = C.expected(dtype, "nan_inf")
    assert np.isposinf(vals[0, 0]) and not np.isnan(vals[0, :counts[0]]).any() and not np.isneginf(vals[0, :counts[0]]).any()
    rev = cs["reverse_order"]
    cols, vals, counts = _all_scores(rev)
    assert list(cols[0, :counts[0]]) == list(rev.cols[0, :rev.counts[0]][::-1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_row_map_is_the_corpus_state_s(dtype):
    from string_grouper_amd.corpus_engine import CorpusState
    state = CorpusState.__new__(CorpusState)
    rng = np.random.default_rng(3)
    for n_dead in (0, 1, 5, 32):
        state.dead = np.sort(rng.choice(100, n_dead, replace=False)).astype(np.int64)
        live = np.arange(100 - n_dead)
        assert np.array_equal(C.physical(state.dead, live), state.physical_rows(live))
        assert np.array_equal(C.physical(state.dead, live), np.delete(np.arange(100), state.dead))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", C.WRONG)
def test_every_wrong_turn_changes_an_answer(dtype, variant):
    cs = C.cases(dtype)
    by_size = sorted(cs, key=lambda name: int(cs[name].counts.sum()))
    assert any(not C.same_result(C.ref_rescore(cs[name], variant), C.expected(dtype, name)) for name in by_size), variant


def test_the_reference_is_deterministic_and_reads_only():
    case = C.cases(np.float32)["counts_short"]
    before = [a.copy() for a in (case.cols, case.vals, case.counts)]
    assert C.same_result(C.ref_rescore(case), C.ref_rescore(case))
    assert all(np.array_equal(a, b) for a, b in zip(before, (case.cols, case.vals, case.counts)))
