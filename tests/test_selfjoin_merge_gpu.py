"""sg_selfjoin_merge called directly -- a caller-made result (sg_topn_from_host), caller-made records (sg_device_upload), no
multiply in front of it -- on the inputs of tests/_merge_cases.py, built at the edges of the three paths of
pairs_select_kernel (sg_spgemm_pruned.hip): the rank sort up to 64 candidates, one register list fed in batches of 64 behind
a bar, and two register lists for strides of 65 .. 128.  BIT FOR BIT, float32 and float64: shape, stride, value type, counts
and the counted cells of every row are the contract's (``ref_merge``), every cell of a row the merge must not touch is as it
was, or the test fails; no tolerance anywhere.  tests/test_merge_cases_cpu.py shows without a GPU that the inputs reach every
path, batch boundary and cut and that a select wrong at one of them would change an answer; a failure here names the row and
what the case says of it.

  - every case in row order (Bt == NULL), each called twice on a fresh upload;
  - the cases over positions through a real index of 9 000 names built over the library's permutation, whose pos_of table is
    downloaded and handed to the reference;
  - the same pairs_select_kernel behind pairs_fill_kernel: sg_spgemm_topn in the self-join form on a small ladder whose hub
    rows receive more than 64 and more than 128 mirrored matches, at top_n 10, 64 and 100, against the oracle's port."""
import numpy as np
import pytest

from tests import _merge_cases as M
from tests import _threshold_cases as T

pytestmark = pytest.mark.gpu

DT = lambda d: np.dtype(d).name


def assert_merged(cs: M.MergeCase, want, res, what):
    """res: the device result after the merge; want: the contract's answer (cols, vals, counts)"""
    from string_grouper_amd import _native as N
    n, stride = cs.cols.shape
    assert res.dims() == (n, stride, N.np_dtype_code(cs.vals.dtype), cs.n_cols), f"{what}: {res.dims()}"
    cols, vals, counts = res.to_host()
    assert cols.shape == (n, stride) and cols.dtype == np.int32 and vals.dtype == cs.vals.dtype and counts.dtype == np.int32
    bits = f"u{vals.itemsize}"
    said = {r.row: r for r in cs.rows}
    touched = np.zeros(n, bool)
    touched[[r.row for r in cs.rows if r.path != "outside"]] = True
    counted = np.arange(stride)[None, :] < want[2][:, None]
    held = counted | ~touched[:, None]          # a row the merge must not touch: EVERY cell
    differs = (counts != want[2]) | ((cols != want[0]) & held).any(axis=1) | ((vals.view(bits) != want[1].view(bits)) & held).any(axis=1)
    if differs.any():
        j = int(np.flatnonzero(differs)[0])
        k = int(want[2][j]) if touched[j] else stride
        raise AssertionError(f"{what}: {int(differs.sum())} rows differ; the first is row {j}, {said.get(j, 'named by no record')}: "
                             f"count {int(counts[j])} want {int(want[2][j])}\n  columns {cols[j, :k].tolist()}\n  want    {want[0][j, :k].tolist()}\n"
                             f"  values  {vals[j, :k].tolist()}\n  want    {want[1][j, :k].tolist()}")


def merge_and_compare(ctx, cs: M.MergeCase, want, post, what):
    res = ctx.topn_from_host(cs.cols, cs.vals, cs.counts, cs.n_cols)
    d_pairs = ctx.upload_ints(cs.pairs.reshape(-1)) if len(cs.pairs) else None
    ctx.selfjoin_merge(res, post, d_pairs.ptr if d_pairs else 0, len(cs.pairs), cs.words, cs.lo, cs.hi, cs.step)
    assert_merged(cs, want, res, what)
    res.free()
    if d_pairs:
        d_pairs.free()


@pytest.mark.parametrize("dtype", M.DTYPES, ids=DT)
@pytest.mark.parametrize("name", [c for c in M.CASES if not c.startswith("permuted")])
def test_merge_equals_the_contract_in_row_order(ctx, name, dtype):
    cs = M.case(name, dtype)
    assert cs.pos_of is None
    for run in ("first", "second"):
        merge_and_compare(ctx, cs, M.want(name, dtype), None, f"{name} {DT(dtype)}, {run} run")


@pytest.mark.parametrize("dtype", M.DTYPES, ids=DT)
def test_merge_equals_the_contract_over_positions(ctx, dtype):
    """the share (1000, 8000, 3) is one of POSITIONS of an index over 9 000 names: membership goes through the index's table"""
    from oracle import oracle as O
    from string_grouper_amd.synth import synth_names
    n = M.PERMUTED_ROWS
    names = synth_names(n, seed=11)
    (A,), _, _ = O.tfidf_sklearn(names, [names], dtype=dtype)
    ctx.set_option("SG_COLLAPSE", "0")          # one index row per name, repeated names too
    dA = ctx.csr_from_scipy(A)
    post = ctx.postings_build(dA, permute=True)
    assert ctx.postings_rows(post) == (n, n, 0)
    p_orig, p_pos = ctx.postings_permutation(post)
    assert p_orig and p_pos, "the index is in row order"
    ctx.sync()
    pos_of = ctx.download_ints(p_pos, n).astype(np.int64)
    assert np.array_equal(np.sort(pos_of), np.arange(n)) and not np.array_equal(pos_of, np.arange(n))
    for S in M.PERMUTED_STRIDES:
        cs = M.case(f"permuted-{S}", dtype)
        # the case chose its rows on the restated permutation; the reference gets the table the library made
        assert np.array_equal(pos_of, cs.pos_of), "the library's permutation is not the one the case was built on"
        cs = cs._replace(pos_of=pos_of)
        merge_and_compare(ctx, cs, M.ref_case(cs), post, f"permuted-{S} {DT(dtype)}")
    # the same records without the index: the share is one of ROWS then, and other rows are the rank's
    cs = M.case("permuted-10", dtype)
    in_rows = cs._replace(name="permuted-10 in row order", pos_of=None, rows=tuple(
        r._replace(path=M.path_of(r.own + r.mirrored, cs.stride) if M.is_member(r.row, cs.lo, cs.hi, cs.step) else "outside") for r in cs.rows))
    M.check_case(in_rows)
    want = M.ref_case(in_rows)
    assert not M.same(want, M.want("permuted-10", dtype))
    merge_and_compare(ctx, in_rows, want, None, f"{in_rows.name} {DT(dtype)}")
    post.free()
    dA.free()


# ---------------------------------------------------------------------------------------------------- behind pairs_fill_kernel
HUB_ANCHORS, HUB_CANDIDATES, HUB_FILLER_ROWS = 3, 200, 1000        # 1 603 rows of 16 power-of-two entries: every score exact
HUB_TOP_N = (10, 64, 100)
HUB_THRESHOLDS = (0.5, 0.75)


@pytest.mark.parametrize("dtype", M.DTYPES, ids=DT)
def test_the_single_gpu_selfjoin_selects_its_hub_rows_like_the_port(ctx, dtype):
    """The ladder of tests/_threshold_cases.py with three families of 200: in the self-join form every pair is scored from
    the row with the larger index and row j RECEIVES its matches i > j as mirrored pairs -- dozens of rows more than 64,
    some more than 128 -- which pairs_select_kernel merges at top_n 10 and 64 (one register list) and 100 (two)."""
    from oracle import port as P
    from tests.test_multiply_threshold_gpu import assert_identical
    cols, vals = T._ladder_rows(T.LADDER_SEED, HUB_ANCHORS, HUB_CANDIDATES, HUB_FILLER_ROWS)
    A = T._rows_to_csr(cols, vals, T.LADDER_COLS, dtype)
    n = A.shape[0]
    assert n == HUB_ANCHORS * (1 + HUB_CANDIDATES) + HUB_FILLER_ROWS <= 2 * T.TILE_ROWS
    ctx.reset_options()
    for k, v in dict(T._STREAM, SG_SYM="1", SG_COLLAPSE="0").items():
        ctx.set_option(k, v)
    dA = ctx.csr_from_scipy(A)
    post = ctx.postings_build(dA)
    assert ctx.postings_rows(post) == (n, n, 0) and ctx.postings_permutation(post) == (0, 0), "positions are rows at this size"
    for t in HUB_THRESHOLDS:
        thr = T.pred(t, dtype)
        full = P.sp_matmul_topn_port(A, A.T, n, thr, True, 4)
        rows = np.repeat(np.arange(n), np.diff(full.indptr))
        received = np.bincount(full.indices[rows > full.indices], minlength=n)
        assert (received > 64).sum() >= 50 and (received > 128).sum() >= 5 and ((received > 0) & (received <= 64)).sum() >= 100, \
            f"thr {thr}: the hub rows are not what the test is about"
        for top_n in HUB_TOP_N:
            what = f"{DT(dtype)} top_n {top_n} thr {thr!r}"
            res = ctx.spgemm_topn(dA, post, top_n, thr)
            st = ctx.stats()
            got = res.to_scipy()
            res.free()
            assert st["prune_symmetric"] == 1 and st["prune_rows"] > 0, f"{what}: another form ran: {st}"      # FIRST: which form ran
            assert_identical(got, P.sp_matmul_topn_port(A, A.T, top_n, thr, True, 4), what)
    post.free()
    dA.free()
