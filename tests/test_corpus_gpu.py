"""GPU tests of the resident corpus (string_grouper_amd/corpus.py) and its reverse path (csrc/sg_corpus.hip): the
forward path, the reverse path and the automatic choice give, bit for bit, the oracle's result -- sklearn's
TfidfVectorizer fitted on the corpus and transforming the batch, then sparse_dot_topn's multiply (oracle/port.py)."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from oracle import oracle as O
from oracle import port as P
from string_grouper_amd.synth import synth_names

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


@functools.lru_cache(maxsize=None)
def corpus_names(n):
    return tuple(synth_names(n, seed=11))


@functools.lru_cache(maxsize=None)
def batch_names(n_corpus, n):
    """Variants of corpus names, every fifth one an exact copy of a corpus name."""
    corpus = corpus_names(n_corpus)
    names = synth_names(n, seed=23 + n, perturb_of=list(corpus[:200_000]), perturb_frac=0.5)
    for i in range(0, n, 5):
        names[i] = corpus[(i * 7919 + 3) % len(corpus)]
    return tuple(names)


@functools.lru_cache(maxsize=4)
def oracle_mats(corpus, batch, dtype):
    (mc, mn), _, _ = O.tfidf_sklearn(list(corpus), [list(corpus), list(batch)], dtype=dtype)
    return mc, mn


def assert_same(got: sp.csr_matrix, want: sp.csr_matrix, what=""):
    assert got.shape == want.shape, what
    assert np.array_equal(np.asarray(got.indptr, np.int64), np.asarray(want.indptr, np.int64)), f"{what}: counts differ"
    assert np.array_equal(got.indices, want.indices), f"{what}: columns differ"
    assert got.data.dtype == want.data.dtype and np.array_equal(got.data, want.data), f"{what}: scores differ"


def device_multiply(eng, corpus, batch, dtype, top_n, thr, path, monkeypatch):
    """The corpus rows' top-n against the batch (match_strings(corpus, batch)'s multiply) on the given path."""
    if path == "auto":
        monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
    else:
        monkeypatch.setenv("SG_CORPUS_REVERSE", "1" if path == "reverse" else "0")
    state = eng.corpus_fit(pd.Series(corpus), 3, r'[,-./]|\s', True, True, dtype)
    try:
        B = eng.corpus_transform(state, pd.Series(batch))
        before = dict(state.stats)
        res = eng._topn_device(state.matrix, B, top_n, thr)
        C = res.to_scipy()
        res.free()
        took = "reverse" if state.stats["reverse"] > before["reverse"] else "forward"
        return sp.csr_matrix((C.data, C.indices, C.indptr), shape=(len(corpus), len(batch))), took
    finally:
        eng.corpus_free(state)


CASES = [  # (corpus rows, batch rows, dtype, threshold, top_n)
    (20_000, 1, np.float64, 0.8, 10),
    (20_000, 100, np.float32, 0.6, 1),
    (20_000, 10_000, np.float64, 0.45, 128),
    (20_000, 10_000, np.float32, 0.3, 200),
    (20_000, 200_000, np.float32, 0.8, 10),
    (20_000, 200_000, np.float64, 0.6, 1),
    (663_000, 1, np.float32, 0.3, 10),
    (663_000, 100, np.float32, 0.45, 200),
    (663_000, 10_000, np.float64, 0.8, 128),
]


@pytest.mark.parametrize("n_corpus,n_batch,dtype,thr,top_n", CASES)
def test_forward_reverse_and_auto_equal_the_oracle(eng, monkeypatch, n_corpus, n_batch, dtype, thr, top_n):
    corpus, batch = corpus_names(n_corpus), batch_names(n_corpus, n_batch)
    mc, mn = oracle_mats(corpus, batch, dtype)
    want = P.sp_matmul_topn_port(mc, mn.T, top_n, thr, True, 16)
    assert want.nnz > 0
    for path in ("forward", "reverse", "auto"):
        got, took = device_multiply(eng, corpus, batch, dtype, top_n, thr, path, monkeypatch)
        if path != "auto":
            assert took == path
        assert_same(got, want, f"{path} path")


def test_hub_batch_cut_binds_with_ties(eng, monkeypatch):
    corpus = corpus_names(20_000)
    hub = corpus[17]
    variants = [hub + " inc", hub.upper(), hub + ".", hub.replace(" ", "  "), hub + " co"]
    batch = tuple([hub] * 5000 + variants * 40 + list(batch_names(20_000, 100)))
    for dtype, top_n in ((np.float32, 10), (np.float64, 128)):
        mc, mn = oracle_mats(corpus, batch, dtype)
        want = P.sp_matmul_topn_port(mc, mn.T, top_n, 0.6, True, 16)
        row = want.getrow(17)
        assert row.nnz == top_n and (row.data == row.data[-1]).sum() > 1      # the cut binds, ties at the cut
        for path in ("forward", "reverse"):
            got, took = device_multiply(eng, corpus, batch, dtype, top_n, 0.6, path, monkeypatch)
            assert took == path
            assert_same(got, want, f"hub {path}")


def test_corpus_with_identical_rows_and_empty_strings(eng, monkeypatch):
    base = list(corpus_names(20_000))
    corpus = tuple(base + base[:3000] + ["", "", base[5]] * 50)
    batch = tuple(list(batch_names(20_000, 10_000)) + [""] * 10 + base[:50])
    mc, mn = oracle_mats(corpus, batch, np.float64)
    want = P.sp_matmul_topn_port(mc, mn.T, 20, 0.5, True, 16)
    for path in ("forward", "reverse"):
        got, took = device_multiply(eng, corpus, batch, np.float64, 20, 0.5, path, monkeypatch)
        assert took == path
        assert_same(got, want, f"identical rows {path}")


@pytest.mark.parametrize("normalize", [True, False])
def test_characters_the_corpus_never_had(eng, normalize):
    """Byte path (an ASCII corpus) and symbol path (a corpus with its own non-ASCII characters): the batch's unseen
    characters give out-of-vocabulary n-grams, as sklearn's transform has it."""
    corpus = list(corpus_names(20_000)[:5000]) + (["Café Zürich", "Straße"] if not normalize else [])
    batch = ["Café Acme", "Ωmega Corp", "日本 Trading", "Straße AG", "", "naïve résumé", corpus[3]]
    kw = dict(normalize_to_ascii=normalize)
    for ascii_corpus in ((True, False) if not normalize else (True,)):
        c = corpus[:5000] if ascii_corpus else corpus
        for dtype in (np.float32, np.float64):
            state = eng.corpus_fit(pd.Series(c), 3, r'[,-./]|\s', True, normalize, dtype)
            try:
                got = eng.corpus_transform(state, pd.Series(batch)).to_scipy()
            finally:
                eng.corpus_free(state)
            (want,), _, _ = O.tfidf_sklearn(c, [batch], dtype=dtype, **kw)
            assert_same(got, want.tocsr(), f"transform ascii_corpus={ascii_corpus} {dtype}")
    with sga.Corpus(pd.Series(corpus), min_similarity=0.3, normalize_to_ascii=normalize) as cp:
        frame = cp.match_strings(pd.Series(batch))
    assert (frame[frame.left_index == frame.right_index].similarity == 1.0).sum() == len(batch)


def test_pair_budget_exceeded_falls_back_to_forward(eng, monkeypatch):
    corpus, batch = corpus_names(20_000), batch_names(20_000, 10_000)
    mc, mn = oracle_mats(corpus, batch, np.float32)
    want = P.sp_matmul_topn_port(mc, mn.T, 10, 0.45, True, 16)
    monkeypatch.setattr(eng, "CORPUS_PAIR_BUDGET", 1000)
    got, took = device_multiply(eng, corpus, batch, np.float32, 10, 0.45, "reverse", monkeypatch)
    assert took == "forward"
    assert_same(got, want, "fallback")


def test_scores_are_the_same_from_either_side(eng, ctx):
    corpus, batch = corpus_names(20_000), synth_names(20_000, seed=5, perturb_of=list(corpus_names(20_000)),
                                                      perturb_frac=0.5)
    for dtype in (np.float32, np.float64):
        state = eng.corpus_fit(pd.Series(corpus), 3, r'[,-./]|\s', True, True, dtype)
        try:
            B = eng.corpus_transform(state, pd.Series(batch))
            idx_b = ctx.postings_build(B.csr)
            fwd = ctx.spgemm_topn(state.matrix.csr, idx_b, 2048, 0.3, True)
            rev = ctx.spgemm_topn(B.csr, eng.corpus_index(state), 2048, 0.3, True)
            assert fwd.counts().max() < 2048 and rev.counts().max() < 2048
            f, r = fwd.to_scipy(), rev.to_scipy()
            for h in (fwd, rev, idx_b):
                h.free()
        finally:
            eng.corpus_free(state)
        f = sp.csr_matrix((f.data, f.indices, f.indptr), shape=(len(corpus), len(batch)))
        r = sp.csr_matrix((r.data, r.indices, r.indptr), shape=(len(batch), len(corpus))).T.tocsr()
        f.sort_indices()
        r.sort_indices()
        assert f.nnz > 10_000
        assert_same(r, f, f"score(d, m) == score(m, d), {dtype}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_transpose_select_through_the_c_abi(ctx, dtype):
    rng = np.random.default_rng(3)
    n_in, n_out, stride = 3000, 700, 40
    counts = rng.integers(0, stride + 1, n_in).astype(np.int32)
    counts[:50] = 0
    cols = np.zeros((n_in, stride), np.int32)
    vals = np.zeros((n_in, stride), dtype)
    for r in range(n_in):
        c = rng.choice(n_out - 100, counts[r], replace=False)        # rows 600.. stay empty
        if r % 2 == 0 and counts[r] > 0:
            c[0] = 7 if 7 not in c[1:] else c[0]                      # row 7: a hub of more than 1 024 pairs
        cols[r, :counts[r]] = c
        vals[r, :counts[r]] = rng.integers(1, 12, counts[r]) / 16.0    # few distinct values: many equal scores
    pairs = ctx.topn_from_host(cols, vals, counts, n_out)
    for top_n in (1, 5, 40, 1500, 2048):
        res = ctx.topn_transpose_select(pairs, n_out, top_n)
        got_c, got_v, got_n = res.to_host()
        res.free()
        rr = np.repeat(np.arange(n_in), counts)
        mask = np.arange(stride)[None, :] < counts[:, None]
        cc, vv = cols[mask], vals[mask]
        assert (cc == 7).sum() > 1024
        order = np.lexsort((rr, -vv, cc))
        cc, rr, vv = cc[order], rr[order], vv[order]
        start = np.searchsorted(cc, np.arange(n_out + 1))
        for m in range(n_out):
            k = min(start[m + 1] - start[m], top_n)
            assert got_n[m] == k, (top_n, m)
            assert np.array_equal(got_c[m, :k], rr[start[m]:start[m] + k]), (top_n, m)
            assert np.array_equal(got_v[m, :k], vv[start[m]:start[m] + k]), (top_n, m)
    pairs.free()


def test_twenty_calls_tokenise_and_index_the_corpus_once(eng):
    corpus = pd.Series(corpus_names(20_000))
    with sga.Corpus(corpus, min_similarity=0.6) as cp:
        for i in range(20):
            batch = pd.Series(synth_names(20, seed=100 + i, perturb_of=list(corpus), perturb_frac=0.5))
            if i % 3 == 0:
                cp.match_strings(batch, corpus)                  # the batch against the corpus index
            elif i % 3 == 1:
                cp.match_strings(corpus, batch)                  # a small batch: the reverse path, the same index
            else:
                cp.match_most_similar(corpus, batch)
        st = cp.stats
    assert st["tokenisations"] == 1 and st["index_builds"] == 1 and st["transforms"] == 20
    assert st["resident_index"] == 7 and st["reverse"] == 13 and st["forward"] == 0


def test_frames_of_both_paths_and_the_module_functions_agree(eng, monkeypatch):
    corpus = pd.Series(corpus_names(20_000), name="name")
    batch = pd.Series(batch_names(20_000, 100), name="new")
    frames = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SG_CORPUS_REVERSE", mode)
        with sga.Corpus(corpus) as cp:
            frames[mode] = (cp.match_strings(corpus, batch, min_similarity=0.5),
                            cp.match_most_similar(corpus, batch, min_similarity=0.5))
            assert cp.stats["reverse" if mode == "1" else "forward"] == 2
    pd.testing.assert_frame_equal(frames["0"][0], frames["1"][0])
    pd.testing.assert_frame_equal(frames["0"][1], frames["1"][1])
    # the corpus's frame = the module-level function's frame on the oracle's fixed-corpus matrices
    from tests.test_corpus_cpu import _expected
    pd.testing.assert_frame_equal(frames["1"][0], _expected(list(corpus), "match_strings", corpus, batch, min_similarity=0.5))


def test_close_frees_what_the_corpus_held(eng, ctx):
    import torch
    ctx.trim()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    corpus = pd.Series(corpus_names(663_000))
    cp = sga.Corpus(corpus, min_similarity=0.8)
    cp.match_strings(corpus, pd.Series(batch_names(663_000, 100)))
    cp.match_strings(pd.Series(batch_names(663_000, 100)), corpus)
    held = free0 - torch.cuda.mem_get_info(0)[0]
    cp.close()
    ctx.trim()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert held > 0
    assert abs(free1 - free0) <= 0.01 * free0, (free0, free1, held)
