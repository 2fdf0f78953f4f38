"""GPU tests of sg_topn_union through ``Context.topn_union``: every case of tests/_union_cases.py held to ``ref_union``'s bits
(columns, values, counts and the stride), the same call twice, the parts untouched, every refusal of include/sg_hip.h followed
by a good call, and the union fed to ``topn_rescore`` against ``ref_rescore`` of ``ref_union``.  No tolerance anywhere."""
import numpy as np
import pytest
import scipy.sparse as sp

from string_grouper_amd import _native as N
from tests import _union_cases as U
from tests._rescore_cases import ref_rescore
from tests.test_rescore_gpu import upload_raw

pytestmark = pytest.mark.gpu
DTYPES = U.DTYPES


class OnDevice:
    """A case on the device: the parts, the primary field's matrices (A is B on the host: one handle), its dead lists."""

    def __init__(self, ctx, scope, case, replace=None):
        self.ctx, self.case = ctx, case
        fld = case.primary
        replace = replace or {}

        def ints(dead):
            return None if dead is None else scope.own(ctx.upload_sorted_ints(dead))

        self.parts = [scope.own(ctx.topn_from_host(p.cols, p.vals, p.counts, case.n_cols)) for p in case.parts]
        self.A = scope.own(replace.get(id(fld.A)) or ctx.csr_from_scipy(fld.A))
        self.B = self.A if fld.B is fld.A else scope.own(replace.get(id(fld.B)) or ctx.csr_from_scipy(fld.B))
        self.primary = (self.A, self.B, ints(fld.dead_a), ints(fld.dead_b))

    def union(self, parts=None, primary=None):
        with N.Scope() as s:
            res = s.own(self.ctx.topn_union(self.parts if parts is None else parts, self.primary if primary is None else primary))
            rows, stride, dtype, n_cols = res.dims()
            cols, vals, counts = res.to_host()
            assert (rows, n_cols) == (self.case.parts[0].cols.shape[0], self.case.n_cols)
            assert cols.shape == (rows, stride) and stride == max(1, int(counts.max(initial=0)))
            return cols, vals, counts


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_case_equals_the_statement(ctx, dtype):
    for name, case in U.cases(dtype).items():
        with N.Scope() as s:
            dev = OnDevice(ctx, s, case)
            want = U.expected(dtype, name)
            first = dev.union()
            assert U.same_result(first, want), name                           # (the shapes too: the stride is the longest row)
            again = dev.union()                                               # the same call twice: the same bits
            assert U.same_result(again, want), name
            for part, on_device in zip(case.parts, dev.parts):                # the parts are only read
                cols, vals, counts = on_device.to_host()
                assert np.array_equal(cols, part.cols) and np.array_equal(U.bits(vals), U.bits(part.vals)), name
                assert np.array_equal(counts, part.counts), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["two_parts_short", "union_sizes", "dead_32", "dead_same_handle"])
def test_the_union_feeds_the_rescoring(ctx, dtype, name):
    case = U.cases(dtype)[name]
    then = U.rescore_case(case, U.expected(dtype, name))
    want = ref_rescore(then)
    fld = then.fields[0]
    with N.Scope() as s:
        dev = OnDevice(ctx, s, case)
        union = s.own(ctx.topn_union(dev.parts, dev.primary))
        a, b = s.own(ctx.csr_from_scipy(fld.A)), s.own(ctx.csr_from_scipy(fld.B))
        res = s.own(ctx.topn_rescore(union, then.w0, [(a, b, fld.w, None, None)], then.threshold, then.top_n))
        assert U.same_result(res.to_host(), want)
        assert want[2].max() > 0


def _good(dev, dtype, name):
    assert U.same_result(dev.union(), U.expected(dtype, name)), "the call after a refusal"


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_seen_on_the_host_and_a_good_call_after_each(ctx, dtype):
    name = "dead_32"
    case = U.cases(dtype)[name]
    other = np.float64 if dtype == np.float32 else np.float32
    fld = case.primary
    with N.Scope() as s:
        dev = OnDevice(ctx, s, case)
        A, B, da, db = dev.primary
        p0, p1 = dev.parts

        def refused(word, **kw):
            with pytest.raises(ValueError, match=word):
                dev.union(**kw)
            _good(dev, dtype, name)

        refused("between 2 and 8", parts=[p0])
        refused("between 2 and 8", parts=[])
        refused("between 2 and 8", parts=[p0, p1] + [p1] * 7)
        dev.union(parts=[p0, p1] + [p1] * 6)                                    # eight are served
        part = case.parts[1]
        fewer_rows = s.own(ctx.topn_from_host(part.cols[:-1], part.vals[:-1], part.counts[:-1], case.n_cols))
        refused("differ in rows, columns or value type", parts=[p0, fewer_rows])
        more_cols = s.own(ctx.topn_from_host(part.cols, part.vals, part.counts, case.n_cols + 1))
        refused("differ in rows, columns or value type", parts=[p0, more_cols])
        wrong_part = s.own(ctx.topn_from_host(part.cols, part.vals.astype(other), part.counts, case.n_cols))
        refused("differ in rows, columns or value type", parts=[p0, wrong_part])
        R = part.cols.shape[0]
        wide = s.own(ctx.topn_from_host(np.zeros((R, U.MAX_ENTRIES - 3), np.int32), np.zeros((R, U.MAX_ENTRIES - 3), dtype),
                                        np.zeros(R, np.int32), case.n_cols))
        refused("2048", parts=[p0, wide])                                       # 4 + 2045: one above the cap
        wrong_type = s.own(ctx.csr_from_scipy(fld.B.astype(other)))
        refused("value type", primary=(A, wrong_type, da, db))
        refused("value type", primary=(wrong_type, wrong_type, db, db))
        wider = s.own(ctx.csr_from_scipy(sp.csr_matrix((fld.B.data, fld.B.indices, fld.B.indptr), shape=(fld.B.shape[0], fld.B.shape[1] + 1))))
        refused("differ in shape", primary=(A, wider, da, db))
        refused("parts' rows", primary=(A, B, None, db))                        # rows(A) - 0 != R
        refused("parts' columns", primary=(A, B, da, None))
        refused("parts' rows", primary=(B, B, da, db))
        refused("parts' columns", primary=(A, A, da, db))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["two_parts_short", "union_sizes"])            # the short kernel alone, and both
def test_a_column_outside_the_result_is_refused_and_nothing_is_read_for_it(ctx, dtype, name):
    case = U.cases(dtype)[name]
    with N.Scope() as s:
        dev = OnDevice(ctx, s, case)
        total = sum(U.counted(p) for p in case.parts)
        for k, part in enumerate(case.parts):
            for row in (int(np.argmax(np.where(total <= U.SHORT, part.counts, -1))), int(np.argmax(part.counts))):
                for bad in (-1, case.n_cols, 2 ** 31 - 1, -2 ** 31):
                    cols = part.cols.copy()
                    cols[row, int(part.counts[row]) - 1] = bad
                    parts = list(dev.parts)
                    parts[k] = s.own(ctx.topn_from_host(cols, part.vals, part.counts, case.n_cols))
                    with pytest.raises(ValueError, match="column lies outside"):
                        dev.union(parts=parts)
                    _good(dev, dtype, name)
                    s.release(parts[k])
        parts = []                                                              # behind a row's count nothing is looked at
        for part in case.parts:
            cols = part.cols.copy()
            cols[np.arange(cols.shape[1])[None, :] >= part.counts[:, None]] = -7
            parts.append(s.own(ctx.topn_from_host(cols, part.vals, part.counts, case.n_cols)))
        assert U.same_result(dev.union(parts=parts), U.expected(dtype, name))


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_unsorted_row_is_refused_only_when_a_filled_candidate_reads_it(ctx, dtype):
    name = "fill_structured"
    case = U.cases(dtype)[name]
    fld = case.primary
    for side, m in (("left", fld.A), ("right", fld.B)):
        lengths = np.diff(m.indptr)
        row = int(np.flatnonzero(lengths == 2 * U.CHUNK + 1)[0])
        for step in ("descending", "repeated"):
            bad = m.copy()
            at = bad.indptr[row + 1] - 2
            if step == "descending":
                bad.indices[[at, at + 1]] = bad.indices[[at + 1, at]]
            else:
                bad.indices[at + 1] = bad.indices[at]
            with N.Scope() as s:
                dev = OnDevice(ctx, s, case, replace={id(m): upload_raw(ctx, bad)})     # (the scope owns it from here)
                with pytest.raises(ValueError, match=f"primary field's {side} matrix .* not sorted"):
                    dev.union()
                # the same matrices where no filled candidate reads that row: served.  Left: the row names what part 0 holds
                # already, nothing is filled for it.  Right: the column is named by part 0 wherever it is named
                p0, p1 = case.parts
                if side == "left":
                    c1 = p1.counts.copy()
                    c1[row] = 0
                    parts = [p0, p1._replace(counts=c1)]
                else:
                    n = case.n_cols
                    swap = lambda cols: np.where(cols == row, (row + 7) % n, cols).astype(np.int32)   # noqa: E731
                    parts = [p0._replace(cols=swap(p0.cols)), p1._replace(cols=swap(p1.cols))]
                on_device = [s.own(ctx.topn_from_host(p.cols, p.vals, p.counts, case.n_cols)) for p in parts]
                got = dev.union(parts=on_device)
                want = U.ref_union(case._replace(parts=parts))
                assert U.same_result(got, want)


def test_parts_without_rows_are_served(ctx):
    with N.Scope() as s:
        parts = [s.own(ctx.topn_from_host(np.zeros((0, k), np.int32), np.zeros((0, k), np.float32), np.zeros(0, np.int32), 6)) for k in (4, 2)]
        a = s.own(ctx.csr_from_scipy(sp.csr_matrix((0, 8), dtype=np.float32)))
        b = s.own(ctx.csr_from_scipy(sp.csr_matrix((6, 8), dtype=np.float32)))
        res = s.own(ctx.topn_union(parts, (a, b, None, None)))
        assert res.dims()[:2] == (0, 1)
