"""GPU tests of sg_topn_rescore through ``Context.topn_rescore``: every case of tests/_rescore_cases.py held to ``ref_rescore``'s
bits (columns, values and counts of the first ``count`` entries of every row), the same call twice, the candidates untouched,
and every refusal of include/sg_hip.h followed by a good call.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from string_grouper_amd import _native as N
from tests import _rescore_cases as C

pytestmark = pytest.mark.gpu
DTYPES = C.DTYPES


def upload_raw(ctx, m: sp.csr_matrix) -> N.Csr:
    """sg_csr_from_host on the arrays as they are: Context.csr_from_scipy would sort the rows first."""
    indptr = np.ascontiguousarray(m.indptr, np.int64)
    indices = np.ascontiguousarray(m.indices, np.int32)
    data = np.ascontiguousarray(m.data)
    out = ctypes.c_void_p()
    N.check(N.lib().sg_csr_from_host(ctx.h, m.shape[0], m.shape[1], N._ptr(indptr), N._ptr(indices), N._ptr(data),
                                     N.np_dtype_code(data.dtype), ctypes.byref(out)))
    return N.Csr(ctx, out)


class OnDevice:
    """A case on the device: the candidates, every matrix once (A is B on the host: one handle), the dead lists."""

    def __init__(self, ctx, scope, case, replace=None):
        self.ctx, self.case = ctx, case
        held = {}

        def of(m):
            if id(m) not in held:
                held[id(m)] = scope.own((replace or {}).get(id(m)) or ctx.csr_from_scipy(m))
            return held[id(m)]

        def ints(dead):
            return None if dead is None else scope.own(ctx.upload_sorted_ints(dead))

        self.cand = scope.own(ctx.topn_from_host(case.cols, case.vals, case.counts, case.n_cols))
        self.fields = [(of(f.A), of(f.B), f.w, ints(f.dead_a), ints(f.dead_b)) for f in case.fields]
        self.n_matrices = len(held)

    def rescore(self, cand=None, w0=None, fields=None, threshold=None, top_n=None):
        case = self.case
        with N.Scope() as s:
            res = s.own(self.ctx.topn_rescore(self.cand if cand is None else cand, case.w0 if w0 is None else w0,
                                              self.fields if fields is None else fields,
                                              case.threshold if threshold is None else threshold,
                                              case.top_n if top_n is None else top_n))
            rows, stride, dtype, n_cols = res.dims()
            assert (rows, stride, n_cols) == (case.cols.shape[0], min(case.top_n if top_n is None else top_n, case.cols.shape[1]),
                                              case.n_cols)
            return res.to_host()


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_case_equals_the_statement(ctx, dtype):
    for name, case in C.cases(dtype).items():
        with N.Scope() as s:
            dev = OnDevice(ctx, s, case)
            if any(f.A is f.B for f in case.fields):
                assert dev.n_matrices < 2 * len(case.fields)                    # (a self-join went in as ONE handle)
            want = C.expected(dtype, name)
            first = dev.rescore()
            assert C.same_result(first, want), name
            again = dev.rescore()                                               # the same call twice: the same bits
            assert C.same_result(again, want), name
            cols, vals, counts = dev.cand.to_host()                             # the candidates are only read
            assert np.array_equal(cols, case.cols) and np.array_equal(C.bits(vals), C.bits(case.vals)), name
            assert np.array_equal(counts, case.counts), name


def _good(dev, dtype, name):
    assert C.same_result(dev.rescore(), C.expected(dtype, name)), "the call after a refusal"


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_seen_on_the_host_and_a_good_call_after_each(ctx, dtype):
    name = "dead_sides_and_fields_differ"
    case = C.cases(dtype)[name]
    other = np.float64 if dtype == np.float32 else np.float32
    with N.Scope() as s:
        dev = OnDevice(ctx, s, case)
        A, B, w, da, db = dev.fields[0]
        f0 = case.fields[0]

        def refused(word, **kw):
            with pytest.raises(ValueError, match=word):
                dev.rescore(**kw)
            _good(dev, dtype, name)

        refused("between 1 and 7", fields=[])
        refused("between 1 and 7", fields=[dev.fields[0]] * 8)
        dev.rescore(fields=[dev.fields[0]] * 7)                                 # seven are served
        refused("top_n", top_n=0)
        refused("top_n", top_n=-3)
        for bad in (np.nan, np.inf, -np.inf):
            refused("not finite", w0=bad)
            refused("not finite", fields=[dev.fields[0], (A, B, bad, da, db)])
        if dtype == np.float32:
            refused("not finite", w0=1e39)                                      # finite as a double, not in the value type
        wrong_type = s.own(ctx.csr_from_scipy(f0.B.astype(other)))
        refused("value type", fields=[(A, wrong_type, w, da, db)])
        refused("value type", fields=[(wrong_type, wrong_type, w, db, db)])
        wider = s.own(ctx.csr_from_scipy(sp.csr_matrix((f0.B.data, f0.B.indices, f0.B.indptr), shape=(f0.B.shape[0], f0.B.shape[1] + 1))))
        refused("differ in shape", fields=[(A, wider, w, da, db)])
        refused("candidates' rows", fields=[(A, B, w, None, db)])               # rows(A) - 0 != R
        refused("candidates' columns", fields=[(A, B, w, da, None)])
        refused("candidates' rows", fields=[(B, B, w, da, db)])
        refused("candidates' columns", fields=[(A, A, w, da, db)])
        too_wide = s.own(ctx.topn_from_host(np.zeros((1, C.MAX_STRIDE + 1), np.int32), np.zeros((1, C.MAX_STRIDE + 1), dtype),
                                            np.zeros(1, np.int32), case.n_cols))
        with pytest.raises(ValueError, match="2048"):
            ctx.topn_rescore(too_wide, 0.5, dev.fields, 0.0, 5)
        _good(dev, dtype, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["counts_short", "counts_long"])                # both select kernels
def test_a_column_outside_the_result_is_refused_and_nothing_is_read_for_it(ctx, dtype, name):
    case = C.cases(dtype)[name]
    with N.Scope() as s:
        dev = OnDevice(ctx, s, case)
        row = int(np.argmax(case.counts))
        for bad in (-1, case.n_cols, 2 ** 31 - 1, -2 ** 31):
            for at in (0, int(case.counts[row]) - 1):
                cols = case.cols.copy()
                cols[row, at] = bad
                cand = s.own(ctx.topn_from_host(cols, case.vals, case.counts, case.n_cols))
                with pytest.raises(ValueError, match="column lies outside"):
                    dev.rescore(cand=cand)
                _good(dev, dtype, name)
                s.release(cand)
        cols = case.cols.copy()                                                 # behind a row's count nothing is looked at
        cols[np.arange(cols.shape[1])[None, :] >= case.counts[:, None]] = -7
        cand = s.own(ctx.topn_from_host(cols, case.vals, case.counts, case.n_cols))
        assert C.same_result(dev.rescore(cand=cand), C.expected(dtype, name))


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_unsorted_row_is_refused_only_when_a_candidate_reads_it(ctx, dtype):
    name = "field_structured"
    case = C.cases(dtype)[name]
    fld = case.fields[0]
    want = C.expected(dtype, name)
    named_cols = set(int(c) for r in range(case.cols.shape[0]) for c in case.cols[r, :case.counts[r]])
    for side, m in (("left", fld.A), ("right", fld.B)):
        lengths = np.diff(m.indptr)
        row = int(np.flatnonzero(lengths == 2 * C.CHUNK + 1)[0])
        for step in ("descending", "repeated"):
            bad = m.copy()
            at = bad.indptr[row + 1] - 2
            if step == "descending":
                bad.indices[[at, at + 1]] = bad.indices[[at + 1, at]]
            else:
                bad.indices[at + 1] = bad.indices[at]
            with N.Scope() as s:
                dev = OnDevice(ctx, s, case, replace={id(m): upload_raw(ctx, bad)})    # (the scope owns it from here)
                with pytest.raises(ValueError, match=f"field 1's {side} matrix .* not sorted"):
                    dev.rescore()
                # the same matrices where no candidate names that row: served
                if side == "left":
                    counts = case.counts.copy()
                    counts[row] = 0
                    cand = s.own(ctx.topn_from_host(case.cols, case.vals, counts, case.n_cols))
                    got = dev.rescore(cand=cand)
                    keep = np.arange(len(counts)) != row
                else:
                    assert row in named_cols
                    cols = np.where(case.cols == row, (row + 5) % case.n_cols, case.cols).astype(np.int32)
                    cand = s.own(ctx.topn_from_host(cols, case.vals, case.counts, case.n_cols))
                    got = dev.rescore(cand=cand)
                    ref = C.ref_rescore(case._replace(cols=cols))
                    assert C.same_result(got, ref)
                    continue
                assert np.array_equal(got[2][keep], want[2][keep]) and got[2][row] == 0
                assert np.array_equal(got[0][keep], want[0][keep]) and np.array_equal(C.bits(got[1][keep]), C.bits(want[1][keep]))


def test_a_result_without_rows_is_served(ctx):
    case = C.cases(np.float32)["field_structured"]
    with N.Scope() as s:
        cand = s.own(ctx.topn_from_host(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), np.zeros(0, np.int32), 6))
        a = s.own(ctx.csr_from_scipy(sp.csr_matrix((0, 8), dtype=np.float32)))
        b = s.own(ctx.csr_from_scipy(sp.csr_matrix((6, 8), dtype=np.float32)))
        res = s.own(ctx.topn_rescore(cand, 0.5, [(a, b, 0.5, None, None)], 0.1, 3))
        assert res.dims()[:2] == (0, 3) and case is not None
