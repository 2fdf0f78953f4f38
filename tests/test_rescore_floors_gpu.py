"""GPU tests of sg_topn_rescore with floors through ``Context.topn_rescore(..., floors=...)``: every case of tests/_floor_cases.py
held to ``ref_rescore_floors``' bits, the same call twice, the candidates untouched, floors that are all None against the
plain call's bits, every refusal followed by a good call, and the order check that looks only at the rows that are read.  No
tolerance anywhere."""
import numpy as np
import pytest

from string_grouper_amd import _native as N
from tests import _floor_cases as FC
from tests import _rescore_cases as C
from tests.test_rescore_gpu import OnDevice, upload_raw

pytestmark = pytest.mark.gpu
DTYPES = C.DTYPES


def rescore(dev, floors, **kw):
    case = dev.case
    with N.Scope() as s:
        res = s.own(dev.ctx.topn_rescore(kw.get("cand", dev.cand), kw.get("w0", case.w0), kw.get("fields", dev.fields),
                                         case.threshold, kw.get("top_n", case.top_n), floors=floors))
        return res.to_host()


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_case_equals_the_statement(ctx, dtype):
    held = {}                                                                   # a case's matrices go up once for all its floors
    with N.Scope() as s:
        for name, (case, floors) in FC.floor_cases(dtype).items():
            if id(case) not in held:
                held[id(case)] = OnDevice(ctx, s, case)
            dev = held[id(case)]
            want = FC.expected(dtype, name)
            assert C.same_result(rescore(dev, floors), want), name
            assert C.same_result(rescore(dev, floors), want), name              # the same call twice: the same bits
            cols, vals, counts = dev.cand.to_host()                             # the candidates are only read
            assert np.array_equal(cols, case.cols) and np.array_equal(C.bits(vals), C.bits(case.vals)), name
            assert np.array_equal(counts, case.counts), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_floors_that_are_all_none_give_the_old_entry_s_bits(ctx, dtype):
    for name, case in C.cases(dtype).items():
        with N.Scope() as s:
            dev = OnDevice(ctx, s, case)
            old = dev.rescore()
            assert C.same_result(old, C.expected(dtype, name)), name
            assert C.same_result(rescore(dev, [None] * (len(case.fields) + 1)), old), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_and_a_good_call_after_each(ctx, dtype):
    name = "dead_sides_and_fields_differ:all"
    case, floors = FC.floor_cases(dtype)[name]
    good = list(floors)
    with N.Scope() as s:
        dev = OnDevice(ctx, s, case)
        A, B, w, da, db = dev.fields[0]

        def refused(word, floors=floors, **kw):
            with pytest.raises(ValueError, match=word):
                rescore(dev, floors, **kw)
            assert C.same_result(rescore(dev, good), FC.expected(dtype, name)), "the call after a refusal"

        for at in range(len(floors)):                                           # a floor that is infinite, on every field
            for bad in (np.inf, -np.inf):
                refused("floor is infinite", floors=[bad if f == at else m for f, m in enumerate(floors)])
        refused("floors for", floors=floors[:-1])                               # one a field, seen by the binding
        refused("floors for", floors=floors + [None])
        # the refusals of sg_topn_rescore hold here too
        refused("between 1 and 7", fields=[], floors=[None])
        refused("between 1 and 7", fields=[dev.fields[0]] * 8, floors=[None] * 9)
        refused("top_n", top_n=0)
        refused("not finite", w0=np.nan)
        refused("not finite", fields=[dev.fields[0], (A, B, np.inf, da, db)])
        refused("candidates' rows", fields=[(A, B, w, None, db), dev.fields[1]])
        refused("candidates' columns", fields=[(A, B, w, da, None), dev.fields[1]])
        cols = case.cols.copy()
        cols[0, 0] = case.n_cols
        bad_cand = s.own(ctx.topn_from_host(cols, case.vals, case.counts, case.n_cols))
        refused("column lies outside", cand=bad_cand)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_unsorted_row_that_only_refused_candidates_name_is_not_looked_at(ctx, dtype):
    """Two further fields; one column's row of B_2 is out of order.  A floor on field 1 refuses every candidate that names the
    column, so the row is never read and the call is served; once the floor is lifted the same row is refused."""
    T = np.dtype(dtype).type
    n, bad_col = 12, 5
    rng = np.random.default_rng(31)
    rows = [(np.arange(n), np.round(rng.uniform(0.5, 1.0, n), 2).astype(T))] * 3
    table = rng.uniform(0.5, 1.0, n)
    table[bad_col] = 0.125                                                      # field 1 scores the column below the floor
    f1 = C.table_field(3, table, T, 0.25)
    wide = C.csr_of([(np.array([0, 1, 2, 3]), np.array([0.5, 0.25, 0.125, 0.5], T))] * n, T, 4)
    left = C.csr_of([(np.array([0, 2]), np.array([1.0, 0.5], T))] * 3, T, 4)
    f2 = C.Field(left, wide, 0.25, None, None)
    case = C.Case(*C.make_cand(rows, n, T, n), n, 0.5, [f1, f2], 0.0, n)
    floors = [None, 0.25, None]
    want = FC.ref_rescore_floors(case, floors)
    assert (want[2] == n - 1).all() and not (want[0] == bad_col).any()
    unsorted = wide.copy()
    at = unsorted.indptr[bad_col]
    unsorted.indices[[at + 1, at + 2]] = unsorted.indices[[at + 2, at + 1]]
    with N.Scope() as s:
        dev = OnDevice(ctx, s, case, replace={id(wide): upload_raw(ctx, unsorted)})
        assert C.same_result(rescore(dev, floors), want)                        # served: the row is not read
        assert C.same_result(rescore(dev, floors), want)
        for lifted in ([None, None, None], [None, 0.0625, None], None):
            with pytest.raises(ValueError, match="field 2's right matrix .* not sorted"):
                rescore(dev, lifted)
            assert C.same_result(rescore(dev, floors), want)                    # and a good call after the refusal
