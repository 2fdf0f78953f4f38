"""GPU tests of sg_topn_rescore with skip_empty through ``Context.topn_rescore(..., skip_empty=True, primary=...)``: every case of
tests/_empty_field_cases.py held to ``ref_rescore_skip_empty``'s bits in fp32 and fp64 -- columns, value bits and counts; the
division is numpy's, one correctly rounded IEEE division --, the same call twice, the candidates untouched, the call
without the option unchanged on the same inputs, and every refusal followed by a good call.  No tolerance anywhere."""
import numpy as np
import pytest

from string_grouper_amd import _native as N
from tests import _empty_field_cases as EC
from tests import _rescore_cases as C
from tests.test_rescore_gpu import OnDevice

pytestmark = pytest.mark.gpu
DTYPES = C.DTYPES


class WithPrimary(OnDevice):
    """A case and its primary on the device: the primary goes up as one more field, so that a handle is shared where the
    host shares a matrix."""

    def __init__(self, ctx, scope, case, primary):
        super().__init__(ctx, scope, case if primary is None else case._replace(fields=list(case.fields) + [primary]))
        self.case, self.primary = case, None
        if primary is not None:
            A, B, _, dead_a, dead_b = self.fields.pop()
            self.primary = (A, B, dead_a, dead_b)

    def skip(self, floors, **kw):
        case = self.case
        with N.Scope() as s:
            res = s.own(self.ctx.topn_rescore(kw.get("cand", self.cand), kw.get("w0", case.w0), kw.get("fields", self.fields),
                                              case.threshold, kw.get("top_n", case.top_n), floors=floors, skip_empty=True,
                                              primary=kw.get("primary", self.primary)))
            assert res.dims()[:2] == (case.cols.shape[0], min(kw.get("top_n", case.top_n), case.cols.shape[1]))
            return res.to_host()

    def without(self, floors):
        case = self.case
        with N.Scope() as s:
            return s.own(self.ctx.topn_rescore(self.cand, case.w0, self.fields, case.threshold, case.top_n, floors=floors)).to_host()


def _differences(got, want):
    """The pairs that differ, for the report: (row, place, column got / wanted, value got / wanted)."""
    out = []
    for r in range(len(want[2])):
        for e in range(max(int(got[2][r]), int(want[2][r]))):
            g = (int(got[0][r, e]), got[1][r, e]) if e < got[2][r] else None
            w = (int(want[0][r, e]), want[1][r, e]) if e < want[2][r] else None
            if g is None or w is None or g[0] != w[0] or C.bits(np.array([g[1]]))[0] != C.bits(np.array([w[1]]))[0]:
                out.append((r, e, g, w))
    return out[:8]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_case_equals_the_statement(ctx, dtype):
    for name, (case, primary, floors) in EC.cases(dtype).items():
        with N.Scope() as s:
            dev = WithPrimary(ctx, s, case, primary)
            want = EC.expected(dtype, name)
            got = dev.skip(floors)
            assert C.same_result(got, want), (name, _differences(got, want))
            assert C.same_result(dev.skip(floors), want), name                  # the same call twice: the same bits
            cols, vals, counts = dev.cand.to_host()                             # the candidates are only read
            assert np.array_equal(cols, case.cols) and np.array_equal(C.bits(vals), C.bits(case.vals)), name
            assert np.array_equal(counts, case.counts), name
            # without the option, floors or none, on the same inputs: what it was
            assert C.same_result(dev.without(floors), EC.expected_without(dtype, name)), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_and_a_good_call_after_each(ctx, dtype):
    name = "dead_sides_and_fields_differ:floor"
    case, primary, floors = EC.cases(dtype)[name]
    other = np.float64 if dtype == np.float32 else np.float32
    good = list(floors)
    with N.Scope() as s:
        dev = WithPrimary(ctx, s, case, primary)
        A, B, w, da, db = dev.fields[0]
        pA, pB, pda, pdb = dev.primary

        def refused(word, floors=floors, **kw):
            with pytest.raises(ValueError, match=word):
                dev.skip(floors, **kw)
            assert C.same_result(dev.skip(good), EC.expected(dtype, name)), "the call after a refusal"

        for at in range(len(floors)):                                           # a floor that is infinite, on every field
            for bad in (np.inf, -np.inf):
                refused("floor is infinite", floors=[bad if f == at else m for f, m in enumerate(floors)])
        refused("floors for", floors=floors[:-1])
        # a primary of the wrong shape or type
        refused("primary field's left matrix has not the candidates' rows", primary=(pA, pB, None, pdb))
        refused("primary field's right matrix has not the candidates' columns", primary=(pA, pB, pda, None))
        refused("primary field's left matrix has not the candidates' rows", primary=(pB, pB, pda, pdb))
        wrong_type = s.own(ctx.csr_from_scipy(primary.B.astype(other)))
        refused("primary field's matrices differ from the candidates in value type", primary=(pA, wrong_type, pda, pdb))
        # the refusals without the option hold here too
        refused("between 1 and 7", fields=[], floors=[None])
        refused("top_n", top_n=0)
        refused("not finite", w0=np.nan)
        refused("candidates' rows", fields=[(A, B, w, None, db), dev.fields[1]])
        for bad in (-1, case.n_cols):                                           # a column outside [0, N)
            cols = case.cols.copy()
            cols[3, 2] = bad
            bad_cand = s.own(ctx.topn_from_host(cols, case.vals, case.counts, case.n_cols))
            refused("column lies outside", cand=bad_cand)
        with pytest.raises(ValueError, match="skip_empty alone"):               # a primary without the option: the binding
            ctx.topn_rescore(dev.cand, case.w0, dev.fields, case.threshold, case.top_n, primary=dev.primary)
        assert C.same_result(dev.skip(floors), EC.expected(dtype, name))
