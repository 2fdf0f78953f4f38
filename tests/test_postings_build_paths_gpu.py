"""Every path of the index build (sg_postings.hip, sg_postings_build_flags) under a multiply that is compared with the port
bit for bit: the fill with LDS counters and with global ones, the postings proper written at once or on demand
(sg_postings_ensure_full, for the rows the pruned multiply hands to the exact kernel), row blocks, the tile-by-tile layout,
rows in position order or not, identical rows grouped or not, and the two indexes a multiply builds for itself (the
tile-by-tile form's and the exact kernel's own).  f32 and f64; self-join and one-sided."""
import numpy as np
import pytest

from oracle import port as P
from tests.test_parity_gpu import _tfidf, assert_csr_identical

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TOP_N = 10
LEFT_ROWS = 4000          # the one-sided product: rows [0, LEFT_ROWS) against the whole list


def _wide_names():
    """three names of more than 128 distinct 3-grams (the pruned multiply hands such rows to the exact kernel); the first two
    are near-copies of each other, so that they have a match besides themselves"""
    rng = np.random.default_rng(77)
    w0, w2 = ("".join(rng.choice(list("ABCDEFGHIJKLMNOPQRSTUVWXYZ"), 180)) for _ in range(2))
    return [w0, w0[:174] + "QZ", w2]


def list_a():
    """About 11 000 names: 10 050 without a repeat among them, 1 000 exact repeats of them, three wide names, an empty name
    and one shorter than an n-gram.  More than 2 x 4096 rows stay after identical rows are grouped (the position permutation
    engages on 4096-column tiles, and on the 2048-column ones of the tile-by-tile form); the rows are no multiple of a tile."""
    from string_grouper_amd.synth import synth_names
    rng = np.random.default_rng(5)
    base = synth_names(10050, 31, dup_frac=0.0)
    names = list(base) + [base[i] for i in rng.choice(len(base), 1000, replace=False)]
    names = [names[i] for i in rng.permutation(len(names))]
    wide = _wide_names()
    for at, name in ((50, ""), (100, wide[0]), (2500, wide[2]), (7000, wide[1]), (9000, "AB")):
        names.insert(at, name)
    return names


def list_b():
    """3 000 names without a repeat: one tile, no permutation"""
    from string_grouper_amd.synth import synth_names
    return list(synth_names(3000, 32, dup_frac=0.0))


class _Case:
    """a list's matrix on the host and on the device, and the port's results -- computed once, never changed"""

    def __init__(self, ctx, names, dtype):
        self.names = names
        self.A = _tfidf(names, dtype)
        self.dA = ctx.csr_from_scipy(self.A)
        self.dL = ctx.csr_from_scipy(self.A[:LEFT_ROWS])
        self._want = {}

    def want(self, thr, one_sided=False):
        key = (thr, one_sided)
        if key not in self._want:
            left = self.A[:LEFT_ROWS] if one_sided else self.A
            self._want[key] = P.sp_matmul_topn_port(left, self.A.T, TOP_N, thr, True, 8)
        return self._want[key]


@pytest.fixture(scope="module")
def cases(_session_ctx):
    made = {}

    def get(which, dtype):
        if (which, dtype) not in made:
            made[which, dtype] = _Case(_session_ctx, list_a() if which == "A" else list_b(), dtype)
        return made[which, dtype]

    yield get
    for c in made.values():
        c.dL.free()
        c.dA.free()


class _options:
    """SG_* switches of the context for a `with` block; what was there before comes back"""

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        before = self.ctx.options()
        self.before = {k: before.get(k) for k in self.opts}
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            self.ctx.set_option(k, v)


def _multiply_and_compare(ctx, case, post, thr, one_sided, what):
    res = ctx.spgemm_topn(case.dL if one_sided else case.dA, post, TOP_N, thr, True)
    st = ctx.stats()
    got = res.to_scipy()
    res.free()
    assert_csr_identical(got, case.want(thr, one_sided), what)
    return st


OPTION_SETS = [{}, {"SG_ROW_BLOCKS": "1"}, {"SG_POSTINGS_LAZY": "0"}, {"SG_POSTINGS_LDS": "0"}, {"SG_K4_STREAM": "0"},
               {"SG_COLLAPSE": "0"}, {"SG_POSTINGS_LDS": "0", "SG_PERMUTE": "0"}]


def _id(opts):
    return "+".join(f"{k}={v}" for k, v in opts.items()) or "defaults"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_list_a_self_join_and_one_sided_equal_the_port(ctx, cases, dtype, opts):
    """List A at 0.8, top 10: the index built under each set of switches, then the self-join and rows [0, 4000) against the
    whole list.  The three wide rows (two of them among the first 4000) go to the exact kernel, whose postings a lazily
    built index writes only then."""
    case = cases("A", dtype)
    n = len(case.names)
    wide_rows = np.flatnonzero(np.diff(case.A.indptr) > 128)
    assert len(wide_rows) == 3 and (wide_rows < LEFT_ROWS).sum() == 2
    # the comparison is not vacuous: every row with entries has a match, thousands have one besides themselves (1 657 of the
    # first 4000), and so have two of the wide rows (the port alone, on the CPU: 17 929 entries; the two rows without entries,
    # the empty name and "AB", have none by necessity)
    for one_sided in (False, True):
        found = np.diff(case.want(0.8, one_sided).indptr)
        entries = np.diff(case.A.indptr)[:len(found)]
        assert ((found > 0) == (entries > 0)).all() and (entries == 0).sum() == (1 if one_sided else 2) and (found >= 2).sum() > 1500
        assert (found[wide_rows[wide_rows < len(found)]] >= 2).sum() >= 1
    with _options(ctx, opts):
        post = ctx.postings_build(case.dA)
        n_index, n_rows, gid = ctx.postings_rows(post)
        assert n_rows == n and n % 4096 != 0
        if opts.get("SG_COLLAPSE") == "0":
            assert n_index == n and not gid
        else:
            assert 2 * 4096 < n_index < n - 900 and gid          # grouped, and still more than two tiles
        assert (ctx.postings_permutation(post)[0] != 0) == (opts.get("SG_PERMUTE") != "0")
        for one_sided in (False, True):
            st = _multiply_and_compare(ctx, case, post, 0.8, one_sided, f"{dtype.__name__} {_id(opts)} one_sided={one_sided}")
            assert st["prune_rows"] > 0 and st["exact_rows"] >= (2 if one_sided else 3), st      # pruned; wide rows handed on
        post.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_list_a_at_0_5_takes_the_tile_by_tile_forms_own_index(ctx, cases, dtype):
    """Below 0.65 a self-join runs on an index the multiply builds for itself (SG_POSTINGS_TILE_FORM): 2048-column tiles, in
    position order (10 000 rows > 2 x 2048)."""
    case = cases("A", dtype)
    post = ctx.postings_build(case.dA)
    st = _multiply_and_compare(ctx, case, post, 0.5, False, f"{dtype.__name__} 0.5")
    assert st["prune_rows"] > 0, st
    post.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_list_a_at_0_3_takes_the_exact_kernels_own_index(ctx, cases, dtype):
    """Below the pruned multiply's thresholds the exact kernel runs the self-join form on an index of its own layout
    (SG_POSTINGS_EXACT_ONLY) -- from 16 384 rows by itself, here through the switch."""
    case = cases("A", dtype)
    with _options(ctx, {"SG_EXACT_SYM_MIN_ROWS": "1000"}):
        post = ctx.postings_build(case.dA)
        st = _multiply_and_compare(ctx, case, post, 0.3, False, f"{dtype.__name__} 0.3")
        assert st["prune_rows"] == 0 and st["prune_symmetric"] == 1 and st["exact_rows"] > 10000, st
        post.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opts", [{}, {"SG_ROW_BLOCKS": "1"}], ids=_id)
def test_list_b_one_tile_no_permutation(ctx, cases, dtype, opts):
    case = cases("B", dtype)
    with _options(ctx, opts):
        post = ctx.postings_build(case.dA)
        assert ctx.postings_rows(post)[:2] == (3000, 3000) and ctx.postings_permutation(post) == (0, 0)
        st = _multiply_and_compare(ctx, case, post, 0.8, False, f"{dtype.__name__} list B {_id(opts)}")
        assert st["prune_rows"] > 0, st
        post.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_build_multiply_free_and_build_again_on_the_same_matrix(ctx, cases, dtype):
    """The second build finds the matrix's properties cached (sg_csr_props); index and result must not depend on it."""
    case = cases("A", dtype)
    results = []
    for _ in range(2):
        post = ctx.postings_build(case.dA)
        res = ctx.spgemm_topn(case.dA, post, TOP_N, 0.8, True)
        results.append(res.to_scipy())
        res.free()
        post.free()
    assert_csr_identical(results[0], results[1], "second build")
    assert_csr_identical(results[1], case.want(0.8), "against the port")
