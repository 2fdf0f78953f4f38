"""GPU tests of sg_matchlist_field_scores through ``MatchList.field_scores``: the lists of tests/_list_field_cases.py, built on
the device by ``matchlist_build`` from ``topn_from_host`` -- plain, and for the square ones with ``fix_diagonal`` /
``symmetrize``, a hub row made by the symmetrisation among them -- held to the statement's bits on the list as it lies there;
the same call twice, the list untouched, and every refusal followed by a good call.  No tolerance anywhere."""
import numpy as np
import pytest

from string_grouper_amd import _native as N
from tests import _list_field_cases as L
from tests._pair_cases import bits
from tests.test_rescore_gpu import upload_raw

pytestmark = pytest.mark.gpu
DTYPES = L.DTYPES


def as_topn(ctx, scope, case, rng):
    """The list of a case as a fixed-stride result: its rows in list order, scores that no test reads."""
    counts = np.diff(case.row_ptr).astype(np.int32)
    stride = max(int(counts.max(initial=0)), 1)
    T = case.fields[0].A.dtype.type
    cols, vals = np.zeros((len(counts), stride), np.int32), np.zeros((len(counts), stride), T)
    for r, c in enumerate(counts):
        cols[r, :c] = case.cols[case.row_ptr[r]:case.row_ptr[r + 1]]
        vals[r, :c] = rng.uniform(0.25, 0.75, c)
    return scope.own(ctx.topn_from_host(cols, vals, counts, case.n_cols))


def upload_fields(ctx, scope, fields):
    held = {}

    def of(m):
        if id(m) not in held:
            held[id(m)] = scope.own(ctx.csr_from_scipy(m))
        return held[id(m)]

    def ints(dead):
        return None if dead is None else scope.own(ctx.upload_sorted_ints(dead))

    return [(of(f.A), of(f.B), ints(f.dead_a), ints(f.dead_b)) for f in fields]


def held_to_the_statement(ml, dev_fields, case, name):
    """The planes of the list as it lies on the device against the statement over that very list; returns the list."""
    row_ptr, cols, vals = ml.to_host()
    on_device = L.ListCase(row_ptr, cols, case.n_cols, case.fields)
    want = L.ref_list_fields(on_device)
    got = ml.field_scores(dev_fields)
    assert got.shape == want.shape and got.dtype == want.dtype, name
    assert np.array_equal(bits(got), bits(want)), name
    assert np.array_equal(bits(ml.field_scores(dev_fields)), bits(want)), name  # the same call twice: the same bits
    again = ml.to_host()                                                        # the list is only read
    assert np.array_equal(again[0], row_ptr) and np.array_equal(again[1], cols) and np.array_equal(bits(again[2]), bits(vals)), name
    return on_device


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_case_equals_the_statement(ctx, dtype):
    rng = np.random.default_rng(5)
    for name, case in L.cases(dtype).items():
        with N.Scope() as s:
            ml = s.own(ctx.matchlist_build(as_topn(ctx, s, case, rng), False, False))
            on_device = held_to_the_statement(ml, upload_fields(ctx, s, case.fields), case, name)
            assert np.array_equal(on_device.row_ptr, case.row_ptr), name        # the case's own rows, edges and all
            counts = np.diff(case.row_ptr)
            for r in np.flatnonzero(counts):
                lo, hi = case.row_ptr[r], case.row_ptr[r + 1]
                assert np.array_equal(np.sort(on_device.cols[lo:hi]), case.cols[lo:hi]), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fix_diagonal,symmetrize", [(True, True), (True, False), (False, True)])
def test_square_lists_with_the_diagonal_and_the_mirror(ctx, dtype, fix_diagonal, symmetrize):
    rng = np.random.default_rng(6)
    for name in ("self_join", "self_join_with_dead_rows"):
        case = L.cases(dtype)[name]
        with N.Scope() as s:
            ml = s.own(ctx.matchlist_build(as_topn(ctx, s, case, rng), fix_diagonal, symmetrize))
            on_device = held_to_the_statement(ml, upload_fields(ctx, s, case.fields), case, name)
            assert len(on_device.cols) > len(case.cols)                         # entries were added, and scored like any other


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_hub_row_made_by_the_symmetrisation(ctx, dtype):
    """Every record names record 0: the mirror gives row 0 some 2 100 entries, which many groups share, while every other row
    holds two."""
    T = np.dtype(dtype).type
    n = L.HUB + 1
    rng = np.random.default_rng(7)
    field = L.mixed_field(rng, n, n, T, dead_a=[3, n], self_join=True)
    case = L.ListCase(np.r_[0, 0, np.arange(1, n)].astype(np.int64), np.zeros(n - 1, np.int32), n, [field])
    with N.Scope() as s:
        ml = s.own(ctx.matchlist_build(as_topn(ctx, s, case, rng), True, True))
        on_device = held_to_the_statement(ml, upload_fields(ctx, s, case.fields), case, "hub")
        assert np.diff(on_device.row_ptr)[0] == n and len(on_device.cols) == 3 * n - 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_and_a_good_call_after_each(ctx, dtype):
    T = np.dtype(dtype).type
    other = np.float64 if T == np.float32 else np.float32
    name = "dead_both_sides_differ"
    case = L.cases(dtype)[name]
    rng = np.random.default_rng(8)
    with N.Scope() as s:
        ml = s.own(ctx.matchlist_build(as_topn(ctx, s, case, rng), False, False))
        good = upload_fields(ctx, s, case.fields)
        A, B, da, db = good[0]

        def refused(word, fields):
            with pytest.raises(ValueError, match=word):
                ml.field_scores(fields)
            assert np.array_equal(bits(ml.field_scores(good)), bits(L.expected(dtype, name))), "the call after a refusal"

        refused("between 1 and 8", [])
        refused("between 1 and 8", [good[0]] * 9)
        refused("list' rows", [(A, B, None, db), good[1]])
        refused("list' columns", [good[0], (A, B, da, None)])
        wrong_type = L.mixed_field(rng, len(case.row_ptr) - 1, case.n_cols, other)
        refused("value type", [good[0]] + upload_fields(ctx, s, [wrong_type]))
        narrow = L.table_field(len(case.row_ptr) - 1, np.ones(case.n_cols), T, 1.0)
        mixed = L.Field(case.fields[1].A, narrow.B, 1.0, case.fields[1].dead_a, None)
        refused("differ in shape", upload_fields(ctx, s, [mixed]))
        # a row of B that an entry reads is out of column order, in a matrix not known to be sorted
        plain = L.mixed_field(rng, len(case.row_ptr) - 1, case.n_cols, T)
        unsorted = plain.B.copy()
        long_enough = [int(j) for j in case.cols if unsorted.indptr[j + 1] - unsorted.indptr[j] >= 2]
        lo = unsorted.indptr[long_enough[0]]                                    # a right row that an entry of the list names
        unsorted.indices[[lo, lo + 1]] = unsorted.indices[[lo + 1, lo]]
        bad = (s.own(ctx.csr_from_scipy(plain.A)), s.own(upload_raw(ctx, unsorted)), None, None)
        refused("field 1's right matrix .* not sorted", [(bad[0], s.own(ctx.csr_from_scipy(plain.B)), None, None), bad])
