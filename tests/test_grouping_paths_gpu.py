"""Every path of the grouping of identical rows (sg_collapse.hip) on inputs built for it (tests/_grouping_cases.py): the hash
table with its four ways of sorting a group's members (a swap, a thread, a workgroup in LDS, a pass of its own for a group
of more than 8 192), the fall-back to the sort-based path at more than 28 such groups, and the sort-based path alone
(SG_GROUP_SORT=1).  Checked bit for bit, f32 and f64: the row -> group table, every group's FULL member list (a multiply
shows only a hub's lowest top_n members), and the self-join and a one-sided product against the port."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import port as P
from tests import _grouping_cases as G
from tests.test_parity_gpu import _device_u32, assert_csr_identical
from tests.test_postings_build_paths_gpu import _options

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
PATHS = [{}, {"SG_GROUP_SORT": "1"}]


def _id(opts):
    return "+".join(f"{k}={v}" for k, v in opts.items()) or "defaults"


class _Case:
    """a matrix on the host and on the device, and what numpy and the port make of it -- computed once, never changed"""

    def __init__(self, ctx, A, port_from=None):
        self.A = A
        self.dA = ctx.csr_from_scipy(A)
        self.gid, self.n_groups = G.expected_gid(A)
        self.members, self.size = G.expected_members(self.gid)
        self.reps = self.members[np.concatenate([[0], np.cumsum(self.size)[:-1]])]
        self._want = {}
        self._port_from = port_from      # the same numbers in f32: its results, widened, are this case's where they are exact

    def want(self, one_sided):
        if one_sided not in self._want:
            left = self.A[:G.LEFT_ROWS] if one_sided else self.A
            if self._port_from is not None:
                self._want[one_sided] = self._widened(self._port_from.want(one_sided), left)
            else:
                self._want[one_sided] = P.sp_matmul_topn_port(left, self.A.T, G.TOP_N, G.THRESHOLD, True, 8)
        return self._want[one_sided]

    def _widened(self, want32, left):
        """The f32 result in this case's dtype.  A score made of powers of two alone (sums of at most 200 products of 2^-8)
        is the same number in f32 and f64; a score that involves the value one ulp under 0.5 is not (0.5 - 2^-26 rounds in
        f32), so the rows that share a column with such a value -- the first hub, its near-copy, the prefix -- are the
        port's in this dtype."""
        A = self.A
        odd = np.frexp(A.data)[0] != 0.5                                  # values that are no power of two
        odd_cols = np.unique(A.indices[odd])
        redo = np.unique(np.repeat(np.arange(left.shape[0]), np.diff(left.indptr))[np.isin(left.indices, odd_cols)])
        assert 0 < len(odd_cols) <= 2 and len(redo) > 0
        part = P.sp_matmul_topn_port(left[redo], A.T, G.TOP_N, G.THRESHOLD, True, 8)
        is_redo = np.zeros(left.shape[0], bool)
        is_redo[redo] = True
        counts = np.diff(want32.indptr)
        keep = np.repeat(~is_redo, counts)                                # entries of the f32 result that stay
        counts[redo] = np.diff(part.indptr)
        into = np.repeat(is_redo, counts)                                 # where the redone rows' entries go
        indices, data = np.empty(counts.sum(), want32.indices.dtype), np.empty(counts.sum(), A.dtype)
        indices[~into], data[~into] = want32.indices[keep], want32.data[keep].astype(A.dtype)
        indices[into], data[into] = part.indices, part.data
        return sp.csr_matrix((data, indices, np.concatenate([[0], np.cumsum(counts)])), shape=want32.shape)


@pytest.fixture(scope="module")
def cases(_session_ctx):
    made = {}

    def get(which, dtype):
        if (which, dtype) not in made:
            if which == "sizes":
                made[which, dtype] = _Case(_session_ctx, G.sizes(dtype))
            elif which in ("hubs28", "hubs29"):          # the port once, in f32, for all rows (the f64 matrix holds the same numbers)
                made[which, dtype] = _Case(_session_ctx, G.hubs(int(which[4:]), dtype),
                                           port_from=None if dtype == np.float32 else get(which, np.float32))
            elif which.startswith("barely"):
                made[which, dtype] = _Case(_session_ctx, G.barely(int(which[6:]), dtype))
            else:
                made[which, dtype] = _Case(_session_ctx, G.tiny(which, dtype))
        return made[which, dtype]

    yield get
    for c in made.values():
        c.dA.free()


def _check_gid(ctx, case, post, what):
    n_index, n_caller, p_gid = ctx.postings_rows(post)
    assert (n_index, n_caller) == (case.n_groups, case.A.shape[0]) and p_gid, what
    ctx.sync()
    np.testing.assert_array_equal(_device_u32(p_gid, n_caller), case.gid, err_msg=what)


def _check_members(ctx, case, post, what):
    """A result over the groups whose row g is {column g: 1.0}, expanded for one row per group (the representatives):
    output row g is the whole of group g, ascending."""
    n_groups, stride = case.n_groups, int(case.size.max())
    cols = np.zeros((n_groups, stride), np.int32)
    vals = np.zeros((n_groups, stride), case.A.dtype)
    cols[:, 0] = np.arange(n_groups)
    vals[:, 0] = 1.0
    groups = ctx.topn_from_host(cols, vals, np.ones(n_groups, np.int32), n_groups)
    d_reps = ctx.upload_sorted_ints(case.reps)
    out = ctx.topn_expand_groups(post, groups, d_reps.ptr, len(d_reps))
    got_cols, got_vals, got_cnt = out.to_host()
    for h in (out, groups, d_reps):
        h.free()
    np.testing.assert_array_equal(got_cnt, case.size, err_msg=what)
    mask = np.arange(stride)[None, :] < got_cnt[:, None]
    np.testing.assert_array_equal(got_cols[mask], case.members, err_msg=what)      # row-major: group 0's rows, group 1's, ...
    assert (got_vals[mask] == 1.0).all(), what


def _check_multiplies(ctx, case, post, what):
    res = ctx.spgemm_topn(case.dA, post, G.TOP_N, G.THRESHOLD, True)
    got = res.to_scipy()
    res.free()
    assert_csr_identical(got, case.want(False), what + " self-join")
    with _options(ctx, {"SG_COLLAPSE_LEFT": "1"}):   # identical LEFT rows grouped as well, by the path under test
        dL = ctx.csr_from_scipy(case.A[:G.LEFT_ROWS])    # (a matrix of its own: groups stay with the matrix they were made for)
        res = ctx.spgemm_topn(dL, post, G.TOP_N, G.THRESHOLD, True)
        got = res.to_scipy()
        res.free()
        dL.free()
    assert_csr_identical(got, case.want(True), what + " one-sided")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opts", PATHS, ids=_id)
def test_sizes_every_size_class_of_the_member_sort(ctx, cases, dtype, opts):
    """Groups of 2, 3, 32, 33, 8 192, 8 193 and 9 000 rows, a near-copy one ulp away, a prefix, wide rows and empty rows."""
    case = cases("sizes", dtype)
    what = f"sizes {dtype.__name__} {_id(opts)}"
    with _options(ctx, opts):
        post = ctx.postings_build(case.dA)
        _check_gid(ctx, case, post, what)
        _check_members(ctx, case, post, what)
        _check_multiplies(ctx, case, post, what)
        post.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opts", PATHS, ids=_id)
def test_hubs28_the_table_path_lists_as_many_very_large_groups_as_it_can(ctx, cases, dtype, opts):
    case = cases("hubs28", dtype)
    what = f"hubs28 {dtype.__name__} {_id(opts)}"
    with _options(ctx, opts):
        post = ctx.postings_build(case.dA)
        _check_gid(ctx, case, post, what)
        _check_members(ctx, case, post, what)
        post.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opts", PATHS, ids=_id)
def test_hubs29_one_very_large_group_too_many_falls_back_to_the_sort_path(ctx, cases, dtype, opts):
    case = cases("hubs29", dtype)
    what = f"hubs29 {dtype.__name__} {_id(opts)}"
    with _options(ctx, opts):
        post = ctx.postings_build(case.dA)
        _check_gid(ctx, case, post, what)
        _check_members(ctx, case, post, what)
        _check_multiplies(ctx, case, post, what)
        post.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opts", PATHS, ids=_id)
@pytest.mark.parametrize("n_groups", [9701, 9699])
@pytest.mark.parametrize("collapse", [None, "1", "0"])
def test_barely_worth_it_or_not(ctx, cases, dtype, opts, n_groups, collapse):
    """10 000 rows: 9 701 groups are more than 97 % of the rows (not grouped unless forced), 9 699 are fewer (grouped unless
    switched off)."""
    case = cases(f"barely{n_groups}", dtype)
    what = f"barely {n_groups} {dtype.__name__} {_id(opts)} SG_COLLAPSE={collapse}"
    grouped = collapse == "1" or (collapse is None and n_groups < 0.97 * 10000)
    with _options(ctx, dict(opts, **({} if collapse is None else {"SG_COLLAPSE": collapse}))):
        post = ctx.postings_build(case.dA)
        if grouped:
            _check_gid(ctx, case, post, what)
            _check_members(ctx, case, post, what)
        else:
            assert ctx.postings_rows(post) == (10000, 10000, 0), what
        res = ctx.spgemm_topn(case.dA, post, G.TOP_N, G.THRESHOLD, True)
        got = res.to_scipy()
        res.free()
        post.free()
    assert_csr_identical(got, case.want(False), what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opts", PATHS, ids=_id)
@pytest.mark.parametrize("which", ["two_same", "three_two_same", "three_distinct"])
def test_tiny_forced(ctx, cases, dtype, opts, which):
    """Two or three rows under SG_COLLAPSE=1; as many groups as rows: not grouped even when forced."""
    case = cases(which, dtype)
    what = f"{which} {dtype.__name__} {_id(opts)}"
    n = case.A.shape[0]
    with _options(ctx, dict(opts, SG_COLLAPSE="1")):
        post = ctx.postings_build(case.dA)
        if which == "three_distinct":
            assert ctx.postings_rows(post) == (n, n, 0), what
        else:
            _check_gid(ctx, case, post, what)
            _check_members(ctx, case, post, what)
        res = ctx.spgemm_topn(case.dA, post, G.TOP_N, G.THRESHOLD, True)
        got = res.to_scipy()
        res.free()
        post.free()
    assert_csr_identical(got, P.sp_matmul_topn_port(case.A, case.A.T, G.TOP_N, G.THRESHOLD, True, 8), what)
