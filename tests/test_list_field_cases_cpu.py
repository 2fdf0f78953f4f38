"""CPU tests of tests/_list_field_cases.py: the statement sg_matchlist_field_scores is held to against plain pair scoring,
the census of the edges the cases must hold, and the wrong references -- every one must change an answer on some case, or
the cases would not tell a kernel that takes that turn from one that does not.  No GPU."""
import numpy as np
import pytest

from tests import _list_field_cases as L
from tests._pair_cases import bits, ref_pairs_dot
from tests._rescore_cases import physical

DTYPES = L.DTYPES


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_statement_is_pair_scoring_on_physical_rows(dtype):
    for name, case in L.cases(dtype).items():
        want = L.expected(dtype, name)
        assert want.shape == (len(case.fields), len(case.cols)) and want.dtype == np.dtype(dtype), name
        counts = np.diff(case.row_ptr)
        rows = np.repeat(np.arange(len(counts)), counts)                        # the row of every entry, by expansion
        assert np.array_equal(rows, L.rows_of_entries(case.row_ptr, len(case.cols))), name
        for f, fld in enumerate(case.fields):
            plain = ref_pairs_dot(fld.A, fld.B, physical(fld.dead_a, rows), physical(fld.dead_b, case.cols))
            assert np.array_equal(bits(plain), bits(want[f])), (name, f)
        assert case.cols.dtype == np.int32 and (0 <= case.cols).all() and (case.cols < case.n_cols).all(), name
        for r in range(len(counts)):                                            # ascending inside a row, as K6 leaves them
            assert (np.diff(case.cols[case.row_ptr[r]:case.row_ptr[r + 1]]) > 0).all(), name
        for fld in case.fields:
            assert fld.A.shape[0] - (0 if fld.dead_a is None else len(fld.dead_a)) == len(counts), name
            assert fld.B.shape[0] - (0 if fld.dead_b is None else len(fld.dead_b)) == case.n_cols, name


@pytest.mark.parametrize("dtype", DTYPES)
def test_census_every_edge_is_present(dtype):
    found = L.census(dtype)
    missing = [e for e in L.EDGES if not found.get(e)]
    assert not missing, (missing, found)
    assert "hub_row" in found["hub row"] and len(L.cases(dtype)["no_entries"].cols) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_wrong_reference_changes_an_answer(dtype):
    changed = {}
    for variant in L.WRONG:
        for name, case in L.cases(dtype).items():
            if name == "hub_row" and variant not in ("run_row_kept", "row_side_left"):
                continue                                                        # (2 100 entries: the cheap turns only)
            if not np.array_equal(bits(L.ref_list_fields(case, variant)), bits(L.expected(dtype, name))):
                changed.setdefault(variant, []).append(name)
    assert sorted(changed) == sorted(L.WRONG), [v for v in L.WRONG if v not in changed]
    assert "empty_rows_before_between_after" in changed["row_side_left"]
    assert "a_run_spans_three_rows" in changed["run_row_kept"]
    assert any(n.startswith("dead_") for n in changed["dead_ignored"]) and any(n.startswith("dead_") for n in changed["side_left"])
