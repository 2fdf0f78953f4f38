"""The gate in front of the pruned multiply (sg_csr_props, csr_props_kernel in sg_spgemm_pruned.hip), ONE ENTRY AT A TIME.
The pruned kernels' bounds hold for values >= 0, columns strictly ascending and squared row norms <= 1.0001; anything else
must take the exact kernel -- and whichever kernel runs, the answer is the port's, bit for bit, or the call refuses with a
ValueError (SG_ERR_BADARG): silently different numbers are the one outcome not allowed.

The base is the small unit ladder of tests/_offnorm_cases.py with 150 candidates per anchor and 4 000 filler rows (5 812
rows = 22 blocks of 256 and 180: the last row is the last lane of a partial wave in a partial block); ONE row of it is changed per variant, at row 0, 63, 64, 255, 256 or n - 1,
and the changed matrix runs as the left matrix only, the right matrix only, and as both (the self-product).  The decision is
observed, not guessed: postings_bytes(index) == 0 says the index was not built for the pruned multiply (right side), and
after a multiply at 0.75 with the pruned kernels' bar lowered, prune_rows says which kernel ran.

Must take the exact kernel: one negative value (-2^-20, -1e-300), one NaN, one +inf, one row of squared norm 1.0002, one
row with a descending pair (uploaded through the raw ABI, so that nothing sorts it), one row that names a column twice.
The last is REFUSED as a right-hand matrix: the same row twice in one posting segment loses a product in the exact
kernel's read-add-write (include/sg_hip.h: sg_postings_build); as a left matrix it is summed like any other entry.
Must stay on the pruned kernels: one -0.0, one stored 0.0, one float32 denormal, one row of a single entry 1.0 (column 0 /
column 4096; also as the first row of each of the index's tiles: filter_posting's full value in a tile's first column), one
empty row, one row of squared norm 1.00005, and a scipy matrix whose indices are not sorted (the binding sorts it)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import port as P
from string_grouper_amd import _native as N
from tests import _offnorm_cases as F
from tests.test_multiply_threshold_gpu import assert_identical

pytestmark = pytest.mark.gpu

N_ROWS = F.GATE_ROWS
POSITIONS = (0, 63, 64, 255, 256, N_ROWS - 1)
THR, TOP_N = 0.75, 10
OPTIONS = {"SG_PRUNE_MIN_THRESHOLD": "0.25", "SG_PRUNE_PILOT": "0"}
E = 3          # the entry of the row that is changed (the fourth in column order), and with E + 1 the pair that is swapped


def base_matrix(dtype):
    return F.small(dtype, F.GATE_FILLER_ROWS, F.GATE_CANDIDATES)


def _parts(dtype):
    A = base_matrix(dtype)
    return A.indptr.astype(np.int64).copy(), A.indices.copy(), A.data.copy()


def _csr(indptr, indices, data, sorted_flag=None):
    m = sp.csr_matrix((data, indices, indptr), shape=(N_ROWS, F.T.LADDER_COLS))
    if sorted_flag is not None:
        m.has_sorted_indices = sorted_flag
    return m


def _one_value(value):
    def make(dtype, r):
        indptr, indices, data = _parts(dtype)
        data[indptr[r] + E] = value(dtype)
        return _csr(indptr, indices, data, True)
    return make


def _row_scaled(norm2):
    def make(dtype, r):
        indptr, indices, data = _parts(dtype)
        data[indptr[r]:indptr[r + 1]] *= dtype(np.sqrt(norm2))
        m = _csr(indptr, indices, data, True)
        got = float(F.max_norm2_as_the_gate_sees_it(m))
        assert abs(got - norm2) < 2e-6 and (got > 1.0001) == (norm2 > 1.0001)
        return m
    return make


def _row_replaced(cols):
    def make(dtype, r):
        indptr, indices, data = _parts(dtype)
        lo, hi = indptr[r], indptr[r + 1]
        indices = np.concatenate([indices[:lo], np.asarray(cols, indices.dtype), indices[hi:]])
        data = np.concatenate([data[:lo], np.ones(len(cols), dtype), data[hi:]])
        indptr[r + 1:] += len(cols) - (hi - lo)
        return _csr(indptr, indices, data, True)
    return make


def _repeated_column(dtype, r):
    indptr, indices, data = _parts(dtype)
    indices[indptr[r] + E + 1] = indices[indptr[r] + E]
    m = _csr(indptr, indices, data)
    assert m.nnz == 16 * N_ROWS and m.has_sorted_indices           # (scipy keeps the two entries, and calls the row sorted)
    return m


def _swapped_pair(dtype, r):
    indptr, indices, data = _parts(dtype)
    p = indptr[r] + E
    indices[[p, p + 1]] = indices[[p + 1, p]]
    data[[p, p + 1]] = data[[p + 1, p]]
    m = _csr(indptr, indices, data)
    assert not m.has_sorted_indices
    return m


# name -> (builder, pruned kernels?, upload through the raw ABI?, refused as a right-hand matrix?)
VARIANTS = {
    "negative": (_one_value(lambda dt: dt(-2.0 ** -20) if dt == np.float32 else dt(-1e-300)), False, False, False),
    "nan": (_one_value(lambda dt: dt(np.nan)), False, False, False),
    "inf": (_one_value(lambda dt: dt(np.inf)), False, False, False),
    "norm2-1.0002": (_row_scaled(1.0002), False, False, False),
    "descending-pair": (_swapped_pair, False, True, False),
    "column-twice": (_repeated_column, False, False, True),
    "minus-zero": (_one_value(lambda dt: dt(-0.0)), True, False, False),
    "stored-zero": (_one_value(lambda dt: dt(0.0)), True, False, False),
    "denormal": (_one_value(lambda dt: dt(np.float32(1e-40))), True, False, False),
    "single-entry-column-0": (_row_replaced([0]), True, False, False),
    "single-entry-column-4096": (_row_replaced([4096]), True, False, False),
    "empty-row": (_row_replaced([]), True, False, False),
    "norm2-1.00005": (_row_scaled(1.00005), True, False, False),
    "scipy-unsorted": (_swapped_pair, True, False, False),
}


def upload_raw(ctx, m: sp.csr_matrix) -> N.Csr:
    """sg_csr_from_host on the arrays as they are: Context.csr_from_scipy would sort the rows first."""
    indptr = np.ascontiguousarray(m.indptr, np.int64)
    indices = np.ascontiguousarray(m.indices, np.int32)
    data = np.ascontiguousarray(m.data)
    out = C.c_void_p()
    N.check(N.lib().sg_csr_from_host(ctx.h, m.shape[0], m.shape[1], N._ptr(indptr), N._ptr(indices), N._ptr(data),
                                     N.np_dtype_code(data.dtype), C.byref(out)))
    return N.Csr(ctx, out)


def multiply(ctx, dL, post):
    res = ctx.spgemm_topn(dL, post, TOP_N, THR, True)
    st = ctx.stats()
    got = res.to_scipy()
    res.free()
    return got, st


@pytest.fixture(scope="module")
def base_results():
    """the port's answer on the unchanged ladder, per dtype: what a matrix that only LOOKS different must give"""
    return {dt: P.sp_matmul_topn_port(base_matrix(dt), base_matrix(dt).T, TOP_N, THR, True, 8) for dt in F.DTYPES}


@pytest.mark.parametrize("dtype", F.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_changed_row_decides_the_kernel_and_the_answer_is_the_ports(ctx, variant, dtype, base_results):
    make, pruned, raw, refused_right = VARIANTS[variant]
    base = base_matrix(dtype)
    ways = [(None, True, POSITIONS)]
    if variant.startswith("single-entry"):            # ... and as the FIRST row of each tile of an index in row order
        ways.append(("0", False, (0, F.TILE_ROWS)))
    for collapse, permute, positions in ways:
        ctx.reset_options()
        for k, v in OPTIONS.items():
            ctx.set_option(k, v)
        if collapse is not None:
            ctx.set_option("SG_COLLAPSE", collapse)
        d_base = ctx.csr_from_scipy(base)
        post_base = ctx.postings_build(d_base, permute=permute)
        assert ctx.postings_bytes(post_base) > 0
        for r in positions:
            V = make(dtype, r)
            assert V.dtype == dtype
            dV = upload_raw(ctx, V) if raw else ctx.csr_from_scipy(V)
            if variant == "scipy-unsorted":
                assert not V.has_sorted_indices            # (the port sorts a copy, as the binding does)
            what = f"{variant} {np.dtype(dtype).name} row {r} SG_COLLAPSE={collapse} permute={permute}"
            # ---- as the left matrix only
            got, st = multiply(ctx, dV, post_base)
            assert (st["prune_rows"] > 0) == pruned, f"{what}, left: prune_rows = {st['prune_rows']}"
            assert_identical(got, P.sp_matmul_topn_port(V, base.T, TOP_N, THR, True, 8), what + ", left")
            # ---- as the right matrix only, and as both
            if refused_right:
                with pytest.raises(ValueError, match="names a column twice"):
                    ctx.postings_build(dV, permute=permute)
                dV.free()
                continue
            post = ctx.postings_build(dV, permute=permute)
            assert (ctx.postings_bytes(post) > 0) == pruned, f"{what}: postings_bytes = {ctx.postings_bytes(post)}"
            for side, dL, L in (("right", d_base, base), ("both", dV, V)):
                got, st = multiply(ctx, dL, post)
                assert (st["prune_rows"] > 0) == pruned, f"{what}, {side}: prune_rows = {st['prune_rows']}"
                want = P.sp_matmul_topn_port(L, V.T, TOP_N, THR, True, 8)
                assert_identical(got, want, f"{what}, {side}")
                if variant == "scipy-unsorted":
                    assert_identical(want, base_results[dtype], what + ": the port on the sorted copy")
            post.free()
            dV.free()
        post_base.free()
        d_base.free()


@pytest.mark.parametrize("dtype", F.DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_column_named_twice_far_apart_in_an_unsorted_row_is_refused_too(ctx, dtype):
    """[.., c, x, c, ..] in a row that is not in ascending order: no two ADJACENT entries are equal, the gate's one walk does
    not see the repeat; a second look at the rows that are out of order does (csr_repeated_column_kernel)."""
    indptr, indices, data = _parts(dtype)
    for r in POSITIONS:
        idx = indices.copy()
        p = indptr[r]
        idx[p + E + 2] = idx[p + E]             # c, x, c -- and x > c: the row has a descending pair, no adjacent equals
        m = _csr(indptr, idx, data)
        assert not m.has_sorted_indices
        dV = upload_raw(ctx, m)
        with pytest.raises(ValueError, match="names a column twice"):
            ctx.postings_build(dV)
        dV.free()


@pytest.mark.parametrize("dtype", F.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("value", [0.0, 2.0 ** -70], ids=["all-zero", "all-2^-70"])
def test_degenerate_scales_of_the_right_hand_matrix(ctx, value, dtype):
    """A right-hand matrix whose stored values are all 0.0 (nnz > 0, largest norm 0: norm_up is the smallest denormal and
    1 / norm_up is inf) and one whose values are all 2^-70 (the squares underflow in float32; norm_up ~ 2^-68), at 0.5 with
    the pruned path forced and at threshold 0; a multiply of the plain ladder on the same context comes after each.  All
    equal the port.  (By reading plan_build / filter_posting / q8_write_unit: 1 / norm_up only ever reaches VALUE fields --
    ceilf(0 * inf) cut to the field's range -- never an address or a loop bound.)"""
    base = base_matrix(dtype)
    Z = sp.csr_matrix((np.full(base.nnz, value, dtype), base.indices, base.indptr), shape=base.shape)
    Z.has_sorted_indices = True
    assert Z.nnz == base.nnz and Z.dtype == dtype
    for k, v in OPTIONS.items():
        ctx.set_option(k, v)
    d_base, dZ = ctx.csr_from_scipy(base), ctx.csr_from_scipy(Z)
    post = ctx.postings_build(dZ)
    assert ctx.postings_bytes(post) > 0                          # zeros and tiny values are cosine-like
    for thr in (0.5, 0.0):
        res = ctx.spgemm_topn(d_base, post, TOP_N, thr, True)
        st = ctx.stats()
        got = res.to_scipy()
        res.free()
        assert (st["prune_rows"] > 0) == (thr == 0.5), (thr, st["prune_rows"])
        want = P.sp_matmul_topn_port(base, Z.T, TOP_N, thr, True, 8)
        assert want.nnz == (0 if (value == 0.0 or thr == 0.5) else want.nnz) and (want.nnz > 0) == (value != 0.0 and thr == 0.0)
        assert_identical(got, want, f"{value!r} {np.dtype(dtype).name} thr={thr}")
    post.free()
    dZ.free()
    post = ctx.postings_build(d_base)
    got, st = multiply(ctx, d_base, post)
    assert st["prune_rows"] > 0
    assert_identical(got, P.sp_matmul_topn_port(base, base.T, TOP_N, THR, True, 8), "the plain ladder afterwards")
    post.free()
    d_base.free()
