"""The inputs of the skip_empty tests of sg_topn_rescore, checked without a GPU: every edge the cases are built for is present
(``census``), every wrong turn of ``WRONG`` changes the answer on some case, and on the cases without an empty row the
statement gives the bits of the references of the call without the option."""
import numpy as np
import pytest

from tests import _empty_field_cases as EC
from tests import _floor_cases as FC
from tests import _rescore_cases as C

DTYPES = C.DTYPES
SMALL = [n for n in EC.cases(np.float32) if "2048" not in n and "many_long_rows" not in n]   # (the variants need not walk these)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_edge_is_present(dtype):
    missing = EC.EDGES - EC.census(dtype)
    assert not missing, sorted(missing)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_wrong_turn_changes_an_answer(dtype):
    quiet = []
    for variant in EC.WRONG:
        if not any(not C.same_result(EC.ref_rescore_skip_empty(*EC.cases(dtype)[name], variant=variant), EC.expected(dtype, name))
                   for name in SMALL):
            quiet.append(variant)
    assert not quiet, quiet


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_an_empty_row_the_statement_is_the_old_one_to_the_bit(dtype):
    seen = 0
    for name, (case, primary, floors) in EC.cases(dtype).items():
        if not name.startswith("no_blank:"):
            continue
        seen += 1
        want = EC.expected(dtype, name)
        base = name.split(":", 1)[1]
        old = C.expected(dtype, base) if floors is None else FC.expected(dtype, base)
        assert C.same_result(want, old), name
    assert seen >= 8


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_option_changes_the_answer_where_a_field_is_empty(dtype):
    changed = [name for name in SMALL if not name.startswith("no_blank:")
               and not C.same_result(EC.expected(dtype, name), EC.expected_without(dtype, name))]
    assert len(changed) >= 15, changed


def test_the_statement_on_one_pair_by_hand():
    """Names and cities identical, the address of one record blank, at 0.5 / 0.3 / 0.2: 0.7 as a zero, 1.0 left out."""
    T = np.float64
    f1 = EC.blank_field(1, [1.0], T, 0.3, right_blank={0})
    f2 = C.table_field(1, [1.0], T, 0.2)
    case = C.Case(*C.make_cand([(np.array([0]), np.array([1.0], T))], 1, T, 1), 1, 0.5, [f1, f2], 0.8, 1)
    assert C.ref_rescore(case)[2][0] == 0
    cols, vals, counts = EC.ref_rescore_skip_empty(case, None, None)
    assert counts[0] == 1 and vals[0, 0] == T(T(T(0.5) + T(0.2)) * T(T(T(0.5) + T(0.3)) + T(0.2))) / T(T(0.5) + T(0.2))
    assert EC.ref_rescore_skip_empty(case, None, [None, 0.5, None])[2][0] == 1          # a floor on the blank field: not held
    assert EC.ref_rescore_skip_empty(case, None, [None, None, 1.0])[2][0] == 0          # on the city: held (strict)
