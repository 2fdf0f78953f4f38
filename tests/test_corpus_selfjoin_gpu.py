"""GPU tests of a self-join that a corpus keeps on the device (Corpus.keep_self_join; engine.corpus_append / corpus_remove) and
of the device operations under it: sg_topn_concat_rows, sg_topn_forget, sg_topn_put_rows, sg_csr_take_rows.  Every comparison
is bit for bit: the operations against their numpy / scipy restatements (tests/_corpus_selfjoin_cases.py), the corpus against
the oracle definition -- sklearn's TfidfVectorizer fitted on the ORIGINAL corpus transforms the current strings, then
sparse_dot_topn's multiply (oracle/port.py) over that matrix in one piece -- and against the same corpus with nothing kept."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from oracle import oracle as O
from oracle import port as P
from string_grouper_amd.string_grouper import StringGrouper
from string_grouper_amd.synth import synth_names
from tests import _corpus_selfjoin_cases as K
from tests._oracle_engine import HostMatrix, OracleEngine

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
STRIDES = [1, 10, 64, 65, 130]


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


def _upload(ctx, rows, stride, n_cols, dtype):
    return ctx.topn_from_host(*K.to_fixed(rows, stride, dtype), n_cols)


def _download(res):
    cols, vals, counts = res.to_host()
    return K.from_fixed(cols, vals, counts)


def _assert_rows(got, want, dtype, what):
    assert len(got) == len(want), what
    bad = K.differing_rows(got, want)
    assert not bad, f"{what}: rows {sorted(bad)[:8]} differ"
    assert all(v.dtype == dtype for _, v in got), what


# ------------------------------------------------------------------------------------------ sg_topn_concat_rows (C ABI)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", STRIDES)
def test_topn_concat_rows_equals_vstack(ctx, dtype, stride):
    rng = np.random.default_rng(300 + stride)
    n_cols = 5000
    host = {n: K.random_result(rng, n, stride, n_cols, dtype) for n in (0, 1, 63, 64, 65, 3000)}
    other_stride = {1: 10, 10: 64, 64: 65, 65: 130, 130: 1}[stride]
    host["other"] = K.random_result(rng, 130, other_stride, n_cols, dtype)          # a part of another stride
    host["empty_rows"] = [(np.zeros(0, np.int32), np.zeros(0, dtype))] * 70
    host["full_rows"] = [r for r in K.random_result(rng, 400, stride, n_cols, dtype) if len(r[0]) == stride][:40]
    strides = {k: (other_stride if k == "other" else stride) for k in host}
    dev = {k: _upload(ctx, v, strides[k], n_cols, dtype) for k, v in host.items()}
    assert len(host["full_rows"]) == 40
    try:
        for names in [(0,), (1,), (3000,), (63, 64), (65, 1, 0, 3000), (0, 0), ("other", 64), (64, "other", 0, "other"),
                      ("empty_rows", 65), ("full_rows", "empty_rows", "other", "full_rows"), ("other",)]:
            got = ctx.topn_concat_rows([dev[k] for k in names])
            want = K.concat_rows([host[k] for k in names])
            r, s, _, c = got.dims()
            assert (r, s, c) == (len(want), max(strides[k] for k in names), n_cols), names
            _assert_rows(_download(got), want, dtype, f"concat {names}")
            if r:                                                    # the kernel's own result as a part
                twice = ctx.topn_concat_rows([got, got])
                _assert_rows(_download(twice), want + want, dtype, f"twice {names}")
                twice.free()
            got.free()
        other_cols = _upload(ctx, host[1], stride, n_cols + 1, dtype)
        other_type = _upload(ctx, host[1], stride, n_cols, np.float64 if dtype == np.float32 else np.float32)
        for bad in ([dev[64], other_cols], [dev[64], other_type], []):
            with pytest.raises(ValueError):
                ctx.topn_concat_rows(bad)
        other_cols.free()
        other_type.free()
    finally:
        for h in dev.values():
            h.free()


# ------------------------------------------------------------------------------------------ sg_topn_forget (C ABI)
BIG = 4400                                    # rows of the one large case: half of them are more than the kernel's LDS table holds


def _dead_lists(rng, n):
    if n == BIG:
        yield "every_other", list(range(0, n, 2))                    # 2 200 entries: searched in global memory
        yield "more_than_the_lds_table", rng.choice(n, 2500, replace=False).tolist() + [0, n - 1]
        return
    yield "none", []
    if n == 0:
        return
    yield "first", [0]
    yield "last", [n - 1]
    if n < 4:
        return
    yield "runs", list(range(0, 3)) + list(range(n // 2, min(n // 2 + 40, n - 2))) + [n - 2, n - 1]
    yield "every_other", list(range(0, n, 2))
    yield "random_few", rng.choice(n, min(29, n // 2), replace=False).tolist()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", STRIDES)
def test_topn_forget_equals_its_numpy_restatement(ctx, dtype, stride):
    rng = np.random.default_rng(500 + stride)
    for n in (0, 1, 63, 64, 65, BIG):
        for what, dead in _dead_lists(rng, n):
            dead = np.array(sorted(set(dead)), np.int64)
            s = max(min(stride, n), 1)                                # (a result's stride is cut at its columns)
            rows = K.random_result(rng, n, s, n, dtype, must_name=dead)
            res = _upload(ctx, rows, s, n, dtype)
            d = ctx.upload_sorted_ints(dead)
            for top_n in sorted({s, max(s - 1, 1)} | ({s + 5} if n < BIG else set())):
                got, d_short = ctx.topn_forget(res, d, top_n)
                n_short = len(d_short)
                want, short = K.forget(rows, dead, top_n)
                tag = f"n {n} stride {s} dead {what} top_n {top_n}"
                r, gs, _, c = got.dims()
                assert (r, gs, c) == (n - len(dead), s, n - len(dead)), tag
                _assert_rows(_download(got), want, dtype, tag)
                assert n_short == len(short), tag
                assert np.array_equal(ctx.download_ints(d_short, n_short), short), tag
                if top_n == s and what in ("runs", "every_other", "more_than_the_lds_table") and s > 1:
                    assert n_short > 0, f"{tag}: no row was cut short, the case shows nothing"
                d_short.free()
                got.free()
            d.free()
            res.free()
    # bad arguments: a result that is not square, more dead rows than rows
    res = _upload(ctx, K.random_result(rng, 10, 3, 12, dtype), 3, 12, dtype)
    d = ctx.upload_sorted_ints([1])
    with pytest.raises(ValueError):
        ctx.topn_forget(res, d, 3)
    res.free()
    d.free()
    res = _upload(ctx, K.random_result(rng, 2, 2, 2, dtype), 2, 2, dtype)
    d = ctx.upload_sorted_ints([0, 1, 2])
    with pytest.raises(ValueError):
        ctx.topn_forget(res, d, 2)
    res.free()
    d.free()


# ------------------------------------------------------------------------------------------ sg_topn_put_rows (C ABI)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", STRIDES)
def test_topn_put_rows_equals_its_numpy_restatement(ctx, dtype, stride):
    rng = np.random.default_rng(700 + stride)
    n_cols = 4000
    narrower = {1: 1, 10: 4, 64: 10, 65: 64, 130: 65}[stride]
    for n in (1, 63, 64, 65, 3000):
        for k, src_stride in ((0, stride), (1, stride), (min(n, 65), narrower), (n, stride), (max(n // 3, 1), narrower)):
            rows = K.random_result(rng, n, stride, n_cols, dtype)
            src = K.random_result(rng, k, src_stride, n_cols, dtype)
            which = rng.permutation(n)[:k]                            # distinct, in any order
            res, dsrc = _upload(ctx, rows, stride, n_cols, dtype), _upload(ctx, src, src_stride, n_cols, dtype)
            d = ctx.upload_ints(which)
            ctx.topn_put_rows(res, d.ptr, k, dsrc)
            assert res.dims()[:2] == (n, stride)
            _assert_rows(_download(res), K.put_rows(rows, which, src), dtype, f"n {n} stride {stride} put {k} of stride {src_stride}")
            for h in (d, dsrc, res):
                h.free()
    rows = K.random_result(rng, 20, stride, n_cols, dtype)
    res = _upload(ctx, rows, stride, n_cols, dtype)
    d = ctx.upload_ints([3, 4])
    two = K.random_result(rng, 2, stride, n_cols, dtype)
    wider = _upload(ctx, K.random_result(rng, 2, stride + 1, n_cols, dtype), stride + 1, n_cols, dtype)
    other_cols = _upload(ctx, two, stride, n_cols + 1, dtype)
    other_type = _upload(ctx, two, stride, n_cols, np.float64 if dtype == np.float32 else np.float32)
    three = _upload(ctx, K.random_result(rng, 3, stride, n_cols, dtype), stride, n_cols, dtype)
    for bad in (wider, other_cols, other_type, three):
        with pytest.raises(ValueError):
            ctx.topn_put_rows(res, d.ptr, 2, bad)
        bad.free()
    _assert_rows(_download(res), rows, dtype, "refused calls wrote nothing")
    res.free()
    d.free()


# ------------------------------------------------------------------------------------------ sg_csr_take_rows (C ABI)
def _random_csr(rng, n_rows, n_cols, dtype, density=0.02):
    m = sp.random(n_rows, n_cols, density=density, format="csr", dtype=np.float64, random_state=rng)
    m.data = (rng.integers(1, 1 << 20, m.nnz) / float(1 << 20)).astype(dtype)
    m = m.astype(dtype)
    m.sort_indices()
    return m


def _assert_csr(got: sp.csr_matrix, want: sp.csr_matrix, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.asarray(got.indptr, np.int64), np.asarray(want.indptr, np.int64)), f"{what}: row pointers differ"
    assert np.array_equal(got.indices, want.indices), f"{what}: columns differ"
    assert got.data.dtype == want.data.dtype and np.array_equal(got.data, want.data), f"{what}: values differ"


@pytest.mark.parametrize("dtype", DTYPES)
def test_csr_take_rows_through_the_c_abi_equals_scipy_indexing(ctx, dtype):
    rng = np.random.default_rng(9)
    n_cols = 3000
    holes = _random_csr(rng, 2000, n_cols, dtype, density=0.01).tolil()
    empty = (0, 1, 2, 700, 701, 1500, 1998, 1999)
    for r in empty:
        holes[r] = 0
    holes = holes.tocsr().astype(dtype)
    holes.eliminate_zeros()
    holes.sort_indices()
    big = _random_csr(rng, 6000, n_cols, dtype)
    host = {"plain": _random_csr(rng, 5000, n_cols, dtype), "holes": holes, "view": big[1234:4321],
            "one": _random_csr(rng, 1, n_cols, dtype, density=0.01), "no_entries": sp.csr_matrix((64, n_cols), dtype=dtype)}
    dev = {k: ctx.csr_from_scipy(v) for k, v in host.items() if k != "view"}
    dev_big = ctx.csr_from_scipy(big)
    dev["view"] = dev_big.row_block(1234, 4321)                       # absolute offsets into big's arrays

    def lists(n):
        yield "none", []
        yield "first", [0]
        yield "last", [n - 1]
        yield "one_row_three_times", [n // 2] * 3
        if n < 3:
            return
        yield "all_descending", list(range(n - 1, -1, -1))
        yield "sixty_three", rng.choice(n, 63).tolist()
        yield "sixty_four", sorted(rng.choice(n, 64).tolist())
        yield "sixty_five_descending", sorted(rng.choice(n, 65).tolist(), reverse=True)
        yield "a_few_thousand_with_repeats", rng.integers(0, n, 3500).tolist()
        yield "all", list(range(n))
    try:
        for name, m in host.items():
            for what, rows in lists(m.shape[0]):
                d = ctx.upload_ints(rows)
                got = ctx.csr_take_rows(dev[name], d)
                want = m[np.asarray(rows, np.int64)] if len(rows) else sp.csr_matrix((0, n_cols), dtype=dtype)
                r, c, nnz, _ = got.dims()
                assert (r, c, nnz) == (len(rows), n_cols, want.nnz), (name, what)
                _assert_csr(got.to_scipy(), want.tocsr(), f"take {name} {what}")
                if r > 3 and what in ("sixty_five_descending", "all_descending"):
                    # the kernel's own result as the parent of a view, as a part of a concatenation, and taken from again
                    view = got.row_block(r // 3, r)
                    twice = ctx.csr_concat([got, view])
                    _assert_csr(twice.to_scipy(), sp.vstack([want, want[r // 3:]], format="csr", dtype=dtype), f"concat {name} {what}")
                    again = ctx.csr_take_rows(view, d2 := ctx.upload_ints([2, 0, 2]))
                    _assert_csr(again.to_scipy(), want[r // 3:][[2, 0, 2]], f"take from a view of a take {name} {what}")
                    for h in (again, d2, twice, view):
                        h.free()
                got.free()
                d.free()
        d = ctx.upload_ints(list(empty) + [3, 0, 0])                  # rows without entries, one of them twice
        got = ctx.csr_take_rows(dev["holes"], d)
        assert got.dims()[2] == holes[3].nnz
        _assert_csr(got.to_scipy(), holes[list(empty) + [3, 0, 0]], "rows without entries")
        got.free()
        d.free()
        for bad in ([5000], [10, 4999, 5000], [-1], [0, -1, 3]):      # outside the matrix: seen on the device
            d = ctx.upload_ints(bad)
            with pytest.raises(ValueError):
                ctx.csr_take_rows(dev["plain"], d)
            d.free()
        d = ctx.upload_ints([3087])                                   # the view has 3 087 rows, its parent more
        with pytest.raises(ValueError):
            ctx.csr_take_rows(dev["view"], d)
        d.free()
    finally:
        for h in list(dev.values()) + [dev_big]:
            h.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_taken_rows_of_vectoriser_made_rows_still_take_the_pruned_multiply(eng, ctx, dtype):
    names = list(synth_names(20_000, seed=11))
    rng = np.random.default_rng(4)
    rows = rng.integers(0, len(names), 6000)
    (m_all,), _, _ = O.tfidf_sklearn(names, [names], dtype=dtype)
    want_m = m_all.tocsr()[rows]
    state = eng.corpus_fit(pd.Series(names), 3, r'[,-./]|\s', True, True, dtype)
    try:
        d = ctx.upload_ints(rows)
        taken = ctx.csr_take_rows(state.matrix.csr, d)
        _assert_csr(taken.to_scipy(), want_m, "taken tf-idf rows")
        idx = ctx.postings_build(state.matrix.csr)
        res = ctx.spgemm_topn(taken, idx, 10, 0.8, True)
        stats = ctx.stats()
        C = res.to_scipy()
        want = P.sp_matmul_topn_port(want_m, m_all.T, 10, 0.8, True, 16)
        _assert_csr(sp.csr_matrix((C.data, C.indices, C.indptr), shape=want.shape), want, "taken rows x corpus")
        assert stats["prune_rows"] > 0, stats                        # the vectoriser's guarantee came along
        for h in (res, idx, taken, d):
            h.free()
    finally:
        eng.corpus_free(state)


# ------------------------------------------------------------------------------------------ a corpus that keeps its self-join
HUB = "NORTHERN LIGHTS HOLDING CO"
UNKNOWN = "qqqqqq xxxxxx"


class _OracleGrouper(StringGrouper):
    """The mirror's fit() and frames over a matrix the oracle made."""

    def __init__(self, matrix, *args, **kwargs):
        self._m = matrix
        super().__init__(*args, **kwargs)

    def _tfidf_on_engine(self):
        A = HostMatrix(self._m)
        return A, A


class _Living:
    """A kept corpus, the same corpus with nothing kept, the oracle's matrix of the current strings (rows of ONE transform of
    every string the test will ever use, by the vectoriser fitted on the original list) and the CPU restatement of the kept
    result, driven through the same steps."""

    def __init__(self, base, later, dtype, **options):
        self.dtype, self.options = dtype, options
        self.base = pd.Series(base, name="name")
        (m,), _, _ = O.tfidf_sklearn(list(base), [list(base) + list(later)], dtype=dtype)
        self.m_all = m.tocsr()
        self.row_of_later = {}
        for i, s in enumerate(later):
            self.row_of_later.setdefault(s, len(base) + i)
        self.rows = np.arange(len(base))                              # rows of m_all that are the current strings
        self.left = self.base
        self.kept = sga.Corpus(self.base, tfidf_matrix_dtype=dtype, **options)
        self.plain = sga.Corpus(self.base, tfidf_matrix_dtype=dtype, **options)
        self.kept.keep_self_join()
        self.top_n, self.thr = self.kept._state.kept_opts
        self.mirror = K.KeptSelfJoin(self.m_all[self.rows], self.top_n, self.thr)

    def close(self):
        self.kept.close()
        self.plain.close()

    @property
    def m(self):
        return self.m_all[self.rows]

    def append(self, strings):
        new = pd.Series(list(strings), name="name")
        self.kept.append(new)
        self.plain.append(new)
        add = np.array([self.row_of_later[s] for s in strings])
        self.mirror.append(self.m_all[add])
        self.rows = np.concatenate([self.rows, add])
        self.left = pd.concat([self.left, new])

    def remove(self, positions):
        """Returns the number of rows the restatement refills."""
        positions = sorted(set(int(p) for p in positions))
        self.kept.remove(positions)
        self.plain.remove(positions)
        keep = np.ones(len(self.rows), bool)
        keep[positions] = False
        self.rows, self.left = self.rows[keep], self.left[keep]
        return len(self.mirror.remove(positions))

    def oracle_frames(self, **kw):
        before = E._engine
        E.set_engine(OracleEngine(use_port=True))
        try:
            opts = dict(self.options, tfidf_matrix_dtype=self.dtype, **kw)
            fitted = _OracleGrouper(self.m, self.left, **opts).fit()
            first = _OracleGrouper(self.m, self.left, **dict(opts, group_rep="first")).fit()
            return fitted.get_matches(), fitted.get_groups(), first.get_groups()
        finally:
            E.set_engine(before)

    @staticmethod
    def frames(corpus, **kw):
        master = corpus.master
        return (corpus.match_strings(master, **kw), corpus.group_similar_strings(master, **kw),
                corpus.group_similar_strings(master, group_rep="first", **kw))

    def check(self, what):
        pd.testing.assert_series_equal(self.kept.master, self.left)
        served = self.kept.stats["self_join_served"]
        got = self.frames(self.kept)
        assert self.kept.stats["self_join_served"] == served + 3, what
        # the definition, bit for bit: counts, columns, scores and the order inside a row
        want = P.sp_matmul_topn_port(self.m, self.m.T, self.top_n, self.thr, True, 16)
        C = self.kept._state.kept.to_scipy()
        _assert_csr(C, sp.csr_matrix((want.data, want.indices, want.indptr), shape=C.shape), f"{what}: the kept result")
        assert C.shape == want.shape, what
        for g, o, p, name in zip(got, self.oracle_frames(), self.frames(self.plain), ("match_strings", "groups", "groups, first")):
            assert len(g) > 0
            (pd.testing.assert_frame_equal if isinstance(g, pd.DataFrame) else pd.testing.assert_series_equal)(g, o, obj=f"{what}: {name} against the oracle")
            (pd.testing.assert_frame_equal if isinstance(g, pd.DataFrame) else pd.testing.assert_series_equal)(g, p, obj=f"{what}: {name} against nothing kept")
        st = self.kept.stats
        assert st["self_join_full"] == 1, (what, st)
        assert st["base_index_builds"] <= 1 + st["compactions"], (what, st)
        assert self.plain.stats["self_join_served"] == 0


def _names_with_hubs(n, seed, n_hub=40):
    names = list(synth_names(n, seed=seed))
    rng = np.random.default_rng(seed)
    for at in rng.choice(n, n_hub, replace=False):
        names[at] = HUB
    names[100] = names[n - 200] = "SOUTHERN CROSS TRADING PARTNERS"
    return names


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_kept_self_join_follows_a_living_list_step_by_step(eng, dtype):
    base = _names_with_hubs(3200, 21)
    variants = synth_names(12, seed=22, perturb_of=base[:1500], perturb_frac=0.5)
    later = variants + [HUB, UNKNOWN] + list(synth_names(5, seed=23))
    live = _Living(base, later, dtype, min_similarity=0.8, max_n_matches=10)
    try:
        assert live.m_all[live.row_of_later[UNKNOWN]].nnz == 0
        live.check("first need")
        live.append(variants[:1])
        live.check("one row appended")
        live.append([HUB] * 5)
        live.check("five copies of the hub's name appended")
        live.append([UNKNOWN])
        live.check("a string without a known n-gram appended")
        assert live.kept.stats["self_join_rows_refilled"] == 0 and live.kept.stats["self_join_append_updates"] == 3
        hub_rows = np.flatnonzero(live.left.to_numpy() == HUB)
        assert len(hub_rows) == 45
        predicted = live.remove(hub_rows[:8])
        assert predicted >= 37 and live.kept.stats["self_join_rows_refilled"] == predicted > 0
        live.check("the eight lowest members of the hub removed")
        # rows nobody else names: nothing is refilled
        named = np.zeros(len(live.mirror.rows), np.int64)
        for i, (c, _) in enumerate(live.mirror.rows):
            named[c[c != i]] += 1
        alone = np.flatnonzero(named == 0)[[0, 7, -1]]
        assert live.remove(alone) == 0 and live.kept.stats["self_join_rows_refilled"] == predicted
        live.check("rows nobody names removed")
        n = len(live.left)
        predicted += live.remove([0, int(np.flatnonzero(live.left.to_numpy() == HUB)[0]), n - 1])
        live.append(variants[1:4] + [HUB])
        predicted += live.remove([len(live.left) - 1, len(live.left) - 3, 5])
        live.check("remove, append, remove")
        st = live.kept.stats
        assert st["self_join_rows_refilled"] == predicted and st["self_join_remove_updates"] == 4, st
        assert st["self_join_append_updates"] == 4 and st["self_join_full"] == 1, st
        # a self-join with other values is not served and leaves the kept result alone
        served = st["self_join_served"]
        other = live.kept.match_strings(live.kept.master, max_n_matches=3)
        pd.testing.assert_frame_equal(other, live.plain.match_strings(live.plain.master, max_n_matches=3))
        other = live.kept.group_similar_strings(live.kept.master, min_similarity=0.6)
        assert live.kept.stats["self_join_served"] == served and live.kept._state.kept is not None
        live.check("after calls with other values")
    finally:
        live.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_kept_self_join_survives_every_kind_of_compaction(eng, dtype):
    base = _names_with_hubs(3200, 31)
    more = list(synth_names(130, seed=32, perturb_of=base[:2000], perturb_frac=0.5))
    for i in range(0, len(more), 11):
        more[i] = HUB
    later = list(dict.fromkeys(more))
    live = _Living(base, later, dtype, min_similarity=0.8, max_n_matches=10)
    try:
        live.check("first need")
        assert 3 * 20 > eng.CORPUS_COMPACT_SHARE * len(base) > 2 * 20
        for k in range(3):                                            # the third append crosses CORPUS_COMPACT_SHARE
            live.append(more[20 * k:20 * k + 20])
            live.check(f"append {k}")
        st = live.kept.stats
        assert st["compactions"] == 1 and st["segments"] == 1 and st["self_join_append_updates"] == 3, st
        rng = np.random.default_rng(5)
        hub_rows = np.flatnonzero(live.left.to_numpy() == HUB)
        gone = np.union1d(rng.choice(len(live.left), eng.CORPUS_MAX_DEAD + 4, replace=False), hub_rows[:3])
        predicted = live.remove(gone)                                 # more than CORPUS_MAX_DEAD at once: compacts
        assert live.kept.stats["compactions"] == 2 and live.kept.stats["dead_rows"] == 0
        live.check("more removals than the corpus keeps dead rows")
        predicted += live.remove([1, 2, 3, len(live.left) - 1])      # dead rows pending ...
        live.append(more[60:100])                                    # ... and an append of more rows than the reverse path takes
        assert len(more[60:100]) > eng.CORPUS_REVERSE_MAX_ROWS
        live.check("a large append with dead rows pending")
        predicted += live.remove([0, int(np.flatnonzero(live.left.to_numpy() == HUB)[0])])
        live.append(more[100:103])
        assert live.kept.stats["dead_rows"] > 0 or live.kept.stats["segments"] == 2
        live.kept.compact()
        live.plain.compact()
        assert live.kept.stats["dead_rows"] == 0 and live.kept.stats["segments"] == 1
        live.check("compact()")
        st = live.kept.stats
        assert st["self_join_rows_refilled"] == predicted > 0 and st["self_join_full"] == 1, st
        assert st["compactions"] >= 3 and st["base_index_builds"] <= 1 + st["compactions"], st
    finally:
        live.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_corpus_smaller_than_max_n_matches_and_max_n_matches_of_one(eng, dtype):
    small = [HUB] * 4 + ["Acme Corporation", "Acme Corp", "Globex Inc", "Initech LLC"]
    later = [HUB, "Acme Corp.", "Globex Incorporated"]
    live = _Living(small, later, dtype, min_similarity=0.5)          # max_n_matches: 20, the corpus has 8 rows
    try:
        assert live.top_n == 20
        live.check("first need")
        live.append([HUB, "Acme Corp."])
        live.check("append")
        assert live.remove([0, 5]) == 0                               # no row was ever full
        live.check("remove")
        live.append(["Globex Incorporated"])
        live.remove([len(live.left) - 1])
        live.check("append, remove")
        assert live.kept.stats["self_join_rows_refilled"] == 0 and live.kept.stats["self_join_full"] == 1
    finally:
        live.close()
    base = _names_with_hubs(3000, 41)
    live = _Living(base, [HUB], dtype, min_similarity=0.8, max_n_matches=1)
    try:
        live.check("first need")
        live.append([HUB, HUB])
        live.check("append")
        hub_rows = np.flatnonzero(live.left.to_numpy() == HUB)
        predicted = live.remove(hub_rows[:1])                         # every member named the lowest one
        assert predicted == len(hub_rows) - 1 == live.kept.stats["self_join_rows_refilled"]
        live.check("the hub's lowest member removed")
    finally:
        live.close()


def test_close_frees_the_kept_result_and_a_handed_out_copy_is_the_caller_s(eng, ctx):
    import torch
    base = pd.Series(_names_with_hubs(20_000, 51), name="name")
    ctx.trim()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    cp = sga.Corpus(base, max_n_matches=64)
    cp.keep_self_join()
    cp.group_similar_strings(cp.master)
    state = cp._state
    copy = eng._topn_device(state.matrix, state.matrix, 64, 0.8)     # what a served call gets
    assert copy is not state.kept and copy.h.value != state.kept.h.value
    cp.append(pd.Series([HUB]))
    cp.remove([0])
    assert copy.dims()[0] == 20_000 and state.kept.dims()[0] == 20_000
    copy.free()
    cp.drop_self_join()
    assert state.kept is None
    cp.keep_self_join()
    cp.match_strings(cp.master)
    assert cp.stats["self_join_full"] == 2 and state.kept is not None
    cp.close()
    assert state.kept is None
    ctx.trim()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert abs(free1 - free0) <= 0.01 * free0, (free0, free1)
