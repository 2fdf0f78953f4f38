"""GPU tests of a resident corpus that grows (Corpus.append / compact, engine.corpus_append / corpus_compact) and of the device
operation under it (sg_csr_concat).  Every comparison is bit for bit against the oracle definition: sklearn's
TfidfVectorizer fitted on the ORIGINAL corpus transforms the original + appended strings and the batch, then
sparse_dot_topn's multiply (oracle/port.py) over those matrices in one piece."""
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

REGEX = r'[,-./]|\s'


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


def assert_same(got: sp.csr_matrix, want: sp.csr_matrix, what=""):
    assert got.shape == want.shape, what
    assert np.array_equal(np.asarray(got.indptr, np.int64), np.asarray(want.indptr, np.int64)), f"{what}: counts differ"
    assert np.array_equal(got.indices, want.indices), f"{what}: columns differ"
    assert got.data.dtype == want.data.dtype and np.array_equal(got.data, want.data), f"{what}: scores differ"


# ------------------------------------------------------------------------------------------ sg_csr_concat (C ABI)
def _random_csr(rng, n_rows, n_cols, dtype, density=0.02):
    m = sp.random(n_rows, n_cols, density=density, format="csr", dtype=np.float64, random_state=rng)
    m.data = (rng.integers(1, 1 << 20, m.nnz) / float(1 << 20)).astype(dtype)
    m = m.astype(dtype)
    m.sort_indices()
    return m


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_csr_concat_through_the_c_abi_equals_vstack(ctx, dtype):
    rng = np.random.default_rng(5)
    n_cols = 3000
    big = _random_csr(rng, 5000, n_cols, dtype)
    host = {
        "a": _random_csr(rng, 1201, n_cols, dtype),
        "b": _random_csr(rng, 37, n_cols, dtype, density=0.3),
        "one": _random_csr(rng, 1, n_cols, dtype, density=0.01),
        "no_rows": sp.csr_matrix((0, n_cols), dtype=dtype),
        "empty_rows": sp.csr_matrix((64, n_cols), dtype=dtype),
        "view": big[1234:4321],                      # on the device: a row-block view (absolute offsets into big's arrays)
        "odd": _random_csr(rng, 333, n_cols, dtype, density=0.011),
    }
    dev = {k: ctx.csr_from_scipy(v) for k, v in host.items() if k != "view"}
    dev_big = ctx.csr_from_scipy(big)
    dev["view"] = dev_big.row_block(1234, 4321)
    cases = [("a", "b"), ("view", "a"), ("a", "view"), ("no_rows", "a"), ("a", "no_rows"), ("empty_rows", "b"),
             ("b", "empty_rows"), ("one", "one"), ("no_rows", "no_rows"), ("empty_rows", "empty_rows"), ("a",),
             ("a", "no_rows", "view", "empty_rows", "b"), ("one", "odd", "b", "view", "a"),
             ("empty_rows", "no_rows", "one", "no_rows", "odd")]
    try:
        for names in cases:
            got = ctx.csr_concat([dev[k] for k in names])
            want = sp.vstack([host[k] for k in names], format="csr", dtype=dtype)
            r, c, nnz, _ = got.dims()
            assert (r, c, nnz) == (want.shape[0], n_cols, want.nnz), names
            assert_same(got.to_scipy(), want, f"concat{names}")
            if r:                                # the kernel's own result as a part, and as the parent of a view
                view = got.row_block(r // 3, r)
                twice = ctx.csr_concat([got, view])
                assert_same(twice.to_scipy(), sp.vstack([want, want[r // 3:]], format="csr", dtype=dtype), f"twice{names}")
                twice.free()
                view.free()
            got.free()
        other_cols = ctx.csr_from_scipy(_random_csr(rng, 10, n_cols + 1, dtype))
        other_type = ctx.csr_from_scipy(_random_csr(rng, 10, n_cols, np.float64 if dtype == np.float32 else np.float32))
        for bad in ([dev["a"], other_cols], [dev["a"], other_type], []):
            with pytest.raises(ValueError):
                ctx.csr_concat(bad)
        other_cols.free()
        other_type.free()
    finally:
        for h in list(dev.values()) + [dev_big]:
            h.free()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_concatenation_of_vectoriser_made_parts_still_takes_the_pruned_multiply(eng, ctx, dtype):
    names = synth_names(20_000, seed=11)
    (want_m,), _, _ = O.tfidf_sklearn(names, [names], dtype=dtype)
    want = P.sp_matmul_topn_port(want_m, want_m.T, 10, 0.8, True, 16)
    state = eng.corpus_fit(pd.Series(names), 3, REGEX, True, True, dtype)
    try:
        whole = state.matrix.csr
        stats = {}
        views = [whole.row_block(0, 12_345), whole.row_block(12_345, 12_345), whole.row_block(12_345, 20_000)]
        cat = ctx.csr_concat(views)
        assert_same(cat.to_scipy(), want_m.tocsr(), "concatenated tf-idf rows")
        for label, m in (("one_piece", whole), ("concatenated", cat)):
            idx = ctx.postings_build(m)
            res = ctx.spgemm_topn(m, idx, 10, 0.8, True)
            stats[label] = ctx.stats()
            C = res.to_scipy()
            res.free()
            idx.free()
            assert_same(sp.csr_matrix((C.data, C.indices, C.indptr), shape=want.shape), want, label)
        assert stats["one_piece"]["prune_rows"] > 0, stats["one_piece"]
        for k in ("prune_rows", "prune_postings", "prune_survivors", "prune_scored", "prune_symmetric"):
            if stats["one_piece"][k] > 0:
                assert stats["concatenated"][k] > 0, (k, stats)
        for h in [cat] + views:
            h.free()
    finally:
        eng.corpus_free(state)


# ------------------------------------------------------------------------------------------ a corpus that grows
@functools.lru_cache(maxsize=None)
def base_names(n=20_000):
    return tuple(synth_names(n, seed=11))


@functools.lru_cache(maxsize=None)
def growth():
    """Three appends of 1, 31 and 2 000 strings: variants of base names, exact copies of base rows, empty strings, and
    fresh names."""
    base = base_names()
    fresh = synth_names(1200, seed=91)
    variants = synth_names(800, seed=92, perturb_of=list(base[:5000]), perturb_frac=0.5)
    x3 = list(fresh) + list(variants)
    for i in range(0, len(x3), 9):
        x3[i] = base[(i * 31 + 5) % len(base)]                    # exact copies of base rows
    for i in range(4, len(x3), 97):
        x3[i] = ""
    x2 = list(synth_names(25, seed=93, perturb_of=list(base[:300]), perturb_frac=0.5)) + ["", base[3], base[3], "", base[17], "zzqqxx"]
    return (base[40],), tuple(x2), tuple(x3)


@functools.lru_cache(maxsize=None)
def batches():
    base, grown = base_names(), sum((list(x) for x in growth()), [])
    big = list(synth_names(200, seed=94, perturb_of=list(base[:400]), perturb_frac=0.5)) + grown[::20] + [""]
    big += list(synth_names(60, seed=95, perturb_of=grown, perturb_frac=0.5))
    small = [grown[0], grown[40], base[3], synth_names(3, seed=96, perturb_of=grown, perturb_frac=1.0)[0], "", base[17] + " co", grown[-1]]
    return tuple(big), tuple(small)


@functools.lru_cache(maxsize=4)
def oracle_rows(dtype):
    base = list(base_names())
    grown = base + sum((list(x) for x in growth()), [])
    big, small = batches()
    (mc, mb, ms), _, _ = O.tfidf_sklearn(base, [grown, list(big), list(small)], dtype=dtype)
    return mc, mb, ms


def topn_host(eng, A, B, top_n, thr):
    res = eng._topn_device(A, B, top_n, thr)
    C = res.to_scipy()
    res.free()
    return sp.csr_matrix((C.data, C.indices, C.indptr), shape=(A.shape[0], B.shape[0]))


def check_every_orientation(eng, state, monkeypatch, dtype, what):
    mc, mb, ms = oracle_rows(dtype)
    Bb = eng.corpus_transform(state, pd.Series(batches()[0]))
    Bs = eng.corpus_transform(state, pd.Series(batches()[1]))
    assert_same(state.matrix.to_scipy(), mc.tocsr(), f"{what}: the corpus's rows")
    try:
        for top_n in (1, 10):
            for thr in (0.8, 0.5):
                tag = f"{what} {np.dtype(dtype).name} top{top_n} thr{thr}"
                for B, mB, size in ((Bb, mb, "big"), (Bs, ms, "small")):
                    want = P.sp_matmul_topn_port(mc, mB.T, top_n, thr, True, 16)
                    assert want.nnz > 0
                    for path in ("forward", "reverse", "auto"):
                        if path == "auto":
                            monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
                        else:
                            monkeypatch.setenv("SG_CORPUS_REVERSE", "1" if path == "reverse" else "0")
                        before = dict(state.stats)
                        got = topn_host(eng, state.matrix, B, top_n, thr)
                        took = "reverse" if state.stats["reverse"] > before["reverse"] else "forward"
                        assert took == (path if path != "auto" else ("reverse" if size == "small" else "forward")), tag
                        assert_same(got, want, f"{tag} corpus x {size} batch, {path}")
                    monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
                    want = P.sp_matmul_topn_port(mB, mc.T, top_n, thr, True, 16)
                    assert_same(topn_host(eng, B, state.matrix, top_n, thr), want, f"{tag} {size} batch x corpus")
                want = P.sp_matmul_topn_port(mc, mc.T, top_n, thr, True, 16)
                assert_same(topn_host(eng, state.matrix, state.matrix, top_n, thr), want, f"{tag} self-join")
    finally:
        Bb.csr.free()
        Bs.csr.free()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_corpus_grown_by_three_appends_equals_the_one_piece_oracle(eng, monkeypatch, dtype):
    monkeypatch.setattr(eng, "CORPUS_COMPACT_SHARE", 1.0)          # no automatic compaction in this test
    state = eng.corpus_fit(pd.Series(base_names()), 3, REGEX, True, True, dtype)
    try:
        for x in growth():
            eng.corpus_append(state, pd.Series(x))
        assert state.stats["segments"] == 2 and state.stats["compactions"] == 0 and state.stats["appends"] == 3
        assert state.stats["rows_appended"] == 2032 and state.matrix.shape[0] == 22_032
        check_every_orientation(eng, state, monkeypatch, dtype, "two segments")
        assert state.stats["base_index_builds"] == 1 and state.stats["index_builds"] == 2
        eng.corpus_compact(state)
        assert state.stats["segments"] == 1 and state.stats["compactions"] == 1
        check_every_orientation(eng, state, monkeypatch, dtype, "compacted")
        assert state.stats["base_index_builds"] == 2 and state.stats["index_builds"] == 3
        assert state.stats["tokenisations"] == 1
    finally:
        eng.corpus_free(state)


def test_a_hub_that_spans_the_segments_keeps_the_lowest_rows(eng, monkeypatch):
    monkeypatch.setattr(eng, "CORPUS_COMPACT_SHARE", 1.0)
    rng = np.random.default_rng(2)
    base = list(base_names())
    hub = "NORTHERN LIGHTS HOLDING CO"
    for at in rng.choice(len(base), 25, replace=False):
        base[at] = hub
    x1 = list(synth_names(300, seed=71))
    for at in rng.choice(len(x1), 15, replace=False):
        x1[at] = hub
    x2 = ["", base[5], base[5], "", base[7]]                        # exact copies of base rows, empty strings
    grown = base + x1 + x2
    batch = [hub] * 50 + [hub + " inc", hub.lower(), base[5], "", base[7] + "."] * 6 + list(synth_names(40, seed=72, perturb_of=grown, perturb_frac=0.5))
    for dtype in (np.float32, np.float64):
        (mc, mn), _, _ = O.tfidf_sklearn(base, [grown, batch], dtype=dtype)
        state = eng.corpus_fit(pd.Series(base), 3, REGEX, True, True, dtype)
        try:
            eng.corpus_append(state, pd.Series(x1))
            eng.corpus_append(state, pd.Series(x2))
            assert state.stats["segments"] == 2
            B = eng.corpus_transform(state, pd.Series(batch))
            for top_n in (10, 30):
                # the batch's copies of the hub against the corpus: 40 equal scores, the cut keeps the lowest rows --
                # with top 30 the 25 of the base and the 5 lowest of the appended
                want = P.sp_matmul_topn_port(mn, mc.T, top_n, 0.6, True, 16)
                row = want.getrow(0)
                assert row.nnz == top_n and (row.data == row.data[0]).all()
                assert (row.indices >= len(base)).sum() == (0 if top_n == 10 else 5)
                assert_same(topn_host(eng, B, state.matrix, top_n, 0.6), want, f"hub, batch x corpus, top {top_n}")
                # the corpus's copies against the batch: 50 equal scores per hub row, on both paths
                want = P.sp_matmul_topn_port(mc, mn.T, top_n, 0.6, True, 16)
                hub_rows = [i for i, s in enumerate(grown) if s == hub]
                assert len(hub_rows) == 40 and all(want.getrow(i).nnz == top_n for i in hub_rows)
                for path in ("0", "1"):
                    monkeypatch.setenv("SG_CORPUS_REVERSE", path)
                    assert_same(topn_host(eng, state.matrix, B, top_n, 0.6), want, f"hub, corpus x batch, reverse={path}, top {top_n}")
                monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
                want = P.sp_matmul_topn_port(mc, mc.T, top_n, 0.6, True, 16)
                assert_same(topn_host(eng, state.matrix, state.matrix, top_n, 0.6), want, f"hub, self-join, top {top_n}")
            B.csr.free()
        finally:
            eng.corpus_free(state)


@pytest.mark.parametrize("normalize", [True, False])
def test_appended_strings_with_characters_the_corpus_never_had(eng, monkeypatch, normalize):
    monkeypatch.setattr(eng, "CORPUS_COMPACT_SHARE", 1.0)
    ascii_base = list(base_names()[:5000])
    new = ["Café Acme", "Ωmega Corp", "日本 Trading", "Straße AG", "", "naïve résumé", ascii_base[3], "~^{}|", ascii_base[9] + " ß"]
    batch = ["Cafe Acme", "Café Acme", "Straße AG", "Strasse AG", ascii_base[3], "日本", ""]
    for base in ([ascii_base] if normalize else [ascii_base, ascii_base + ["Café Zürich", "Straße"]]):
        for dtype in (np.float32, np.float64):
            (mc, mn), _, _ = O.tfidf_sklearn(base, [base + new + new[:2], batch], dtype=dtype, normalize_to_ascii=normalize)
            state = eng.corpus_fit(pd.Series(base), 3, REGEX, True, normalize, dtype)
            try:
                eng.corpus_append(state, pd.Series(new))
                eng.corpus_append(state, pd.Series(new[:2]))
                what = f"normalize={normalize} own non-ASCII={len(base) > 5000} {np.dtype(dtype).name}"
                assert_same(state.matrix.to_scipy(), mc.tocsr(), f"rows, {what}")
                B = eng.corpus_transform(state, pd.Series(batch))
                for path in ("0", "1"):
                    monkeypatch.setenv("SG_CORPUS_REVERSE", path)
                    assert_same(topn_host(eng, state.matrix, B, 5, 0.3), P.sp_matmul_topn_port(mc, mn.T, 5, 0.3, True, 16),
                                f"corpus x batch reverse={path}, {what}")
                monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
                assert_same(topn_host(eng, B, state.matrix, 5, 0.3), P.sp_matmul_topn_port(mn, mc.T, 5, 0.3, True, 16),
                            f"batch x corpus, {what}")
                B.csr.free()
            finally:
                eng.corpus_free(state)


def test_appends_that_cross_the_share_compact_once(eng):
    base = pd.Series(base_names(), name="name")
    share = eng.CORPUS_COMPACT_SHARE
    per = int(len(base) * share / 2.5)                             # the third append crosses the share
    parts = [pd.Series(synth_names(per, seed=60 + i, perturb_of=list(base), perturb_frac=0.5), name="name") for i in range(3)]
    batch = pd.Series(synth_names(50, seed=64, perturb_of=list(base[:500]) + list(parts[2][:500]), perturb_frac=0.5))
    from tests.test_corpus_cpu import _expected
    with sga.Corpus(base, min_similarity=0.6) as cp:
        for i, x in enumerate(parts):
            cp.append(x)
            assert cp.stats["segments"] == (2 if i < 2 else 1) and cp.stats["compactions"] == (0 if i < 2 else 1)
            grown = pd.concat([base] + parts[:i + 1])
            pd.testing.assert_frame_equal(cp.match_strings(cp.master, batch), _expected(list(base), "match_strings", grown, batch, min_similarity=0.6))
            pd.testing.assert_frame_equal(cp.match_strings(batch, cp.master), _expected(list(base), "match_strings", batch, grown, min_similarity=0.6))
        assert cp.stats["appends"] == 3 and cp.stats["rows_appended"] == 3 * per and cp.stats["tokenisations"] == 1


def test_two_hundred_single_row_appends_never_reindex_the_whole_list(eng):
    from tests.test_corpus_cpu import _expected
    base = pd.Series(base_names(), name="name")
    rows = synth_names(200, seed=81, perturb_of=list(base[:2000]), perturb_frac=0.5)
    queries = synth_names(200, seed=82, perturb_of=rows, perturb_frac=0.5)
    queries[-1] = rows[-1]                       # the last query is answered by the row appended just before it
    with sga.Corpus(base, min_similarity=0.5) as cp:
        for r, q in zip(rows, queries):
            cp.append(pd.Series([r], name="name"))
            got = cp.match_strings(cp.master, pd.Series([q]))
        st = cp.stats
        grown = pd.concat([base, pd.Series(rows, index=[0] * 200, name="name")])
        pd.testing.assert_series_equal(cp.master, grown)
        pd.testing.assert_frame_equal(got, _expected(list(base), "match_strings", grown, pd.Series([queries[-1]]), min_similarity=0.5))
        assert ((got.left_name == rows[-1]) & (got.similarity > 0.999)).any()
    assert st["tokenisations"] == 1 and st["appends"] == 200 and st["rows_appended"] == 200
    assert st["base_index_builds"] <= 1 + st["compactions"], st
    assert st["compactions"] == 0 and st["reverse"] == 200, st


def test_close_after_appends_and_compaction_frees_what_the_corpus_held(eng, ctx):
    import torch
    names = synth_names(713_000, seed=11)
    corpus, more = pd.Series(names[:663_000]), pd.Series(names[663_000:])
    batch = pd.Series(synth_names(100, seed=12, perturb_of=names[600_000:], perturb_frac=0.5))
    ctx.trim()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    cp = sga.Corpus(corpus, min_similarity=0.8)
    cp.match_strings(corpus, batch)
    cp.append(more[:20_000])
    cp.match_strings(cp.master, batch)                        # forward: the concatenated rows are made and kept
    cp.match_strings(batch, cp.master)                        # both indexes
    cp.append(more[20_000:])
    cp.match_strings(cp.master, batch[:5])                    # reverse
    cp.compact()
    cp.match_strings(batch, cp.master)
    cp.match_strings(cp.master, batch)
    assert cp.stats["segments"] == 1 and cp.stats["compactions"] >= 1 and len(cp.master) == 713_000
    held = free0 - torch.cuda.mem_get_info(0)[0]
    cp.close()
    ctx.trim()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert held > 0
    assert abs(free1 - free0) <= 0.01 * free0, (free0, free1, held)
