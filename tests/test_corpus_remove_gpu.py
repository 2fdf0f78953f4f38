"""GPU tests of a resident corpus that forgets rows (Corpus.remove, engine.corpus_remove / corpus_compact) and of the two device
operations under it (sg_csr_select_rows, sg_topn_drop_columns).  Every comparison is bit for bit: the operations against scipy /
numpy restatements, the corpus against the oracle definition -- sklearn's TfidfVectorizer fitted on the ORIGINAL corpus
transforms the strings that are left and the batch, then sparse_dot_topn's multiply (oracle/port.py) over those matrices in
one piece."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from oracle import oracle as O
from oracle import port as P
from string_grouper_amd.synth import synth_names
from tests.test_corpus_append_gpu import (REGEX, _random_csr, assert_same, base_names, batches, growth, oracle_rows,
                                          topn_host)

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


def _keep(n, drop):
    keep = np.ones(n, bool)
    keep[np.asarray(drop, dtype=np.int64)] = False
    return keep


# ------------------------------------------------------------------------------------------ sg_csr_select_rows (C ABI)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_csr_select_rows_through_the_c_abi_equals_scipy_keep(ctx, dtype):
    rng = np.random.default_rng(7)
    n_cols = 3000
    plain = _random_csr(rng, 5000, n_cols, dtype)
    holes = _random_csr(rng, 2000, n_cols, dtype, density=0.01).tolil()
    for r in (0, 1, 2, 700, 701, 1500, 1998, 1999):                  # rows without entries, dropped and kept ones among them
        holes[r] = 0
    holes = holes.tocsr().astype(dtype)
    holes.eliminate_zeros()
    holes.sort_indices()
    big = _random_csr(rng, 6000, n_cols, dtype)
    host = {"plain": plain, "holes": holes, "view": big[1234:4321], "one": _random_csr(rng, 1, n_cols, dtype, density=0.01),
            "no_entries": sp.csr_matrix((64, n_cols), dtype=dtype)}
    dev = {k: ctx.csr_from_scipy(v) for k, v in host.items() if k != "view"}
    dev_big = ctx.csr_from_scipy(big)
    dev["view"] = dev_big.row_block(1234, 4321)        # absolute offsets into big's arrays

    def lists(n):
        yield "none", []
        yield "first", [0]
        yield "last", [n - 1]
        if n < 3:
            return
        yield "one", [n // 3]
        yield "first_and_last", [0, n - 1]
        yield "runs", list(range(0, min(5, n))) + list(range(n // 2, min(n // 2 + 40, n))) + list(range(max(n - 3, 0), n))
        yield "every_other", list(range(0, n, 2))
        yield "random_few", sorted(rng.choice(n, min(37, n), replace=False).tolist())
        yield "random_many", sorted(rng.choice(n, n // 2, replace=False).tolist())
        yield "all_but_one", [r for r in range(n) if r != n // 2]
        yield "all_but_the_first", list(range(1, n))
        yield "all", list(range(n))
    try:
        for name, m in host.items():
            n = m.shape[0]
            for what, drop in lists(n):
                drop = sorted(set(drop))
                d = ctx.upload_sorted_ints(drop)
                got = ctx.csr_select_rows(dev[name], d)
                want = m[_keep(n, drop)]
                r, c, nnz, _ = got.dims()
                assert (r, c, nnz) == (want.shape[0], n_cols, want.nnz), (name, what)
                assert_same(got.to_scipy(), want, f"select {name} {what}")
                if r > 3 and what in ("runs", "random_few", "one"):
                    # the kernel's own result as a part of a concatenation, as the parent of a view, and selected again
                    view = got.row_block(r // 3, r)
                    twice = ctx.csr_concat([got, view])
                    assert_same(twice.to_scipy(), sp.vstack([want, want[r // 3:]], format="csr", dtype=dtype), f"concat {name} {what}")
                    again = ctx.csr_select_rows(view, d2 := ctx.upload_sorted_ints([0, 2]))
                    assert_same(again.to_scipy(), want[r // 3:][_keep(r - r // 3, [0, 2])], f"select of a view of a selection {name} {what}")
                    for h in (again, twice, view, d2):
                        h.free()
                got.free()
                d.free()
        # bad lists: seen on the host where the list is made, or on the device where only the matrix says so
        for bad in ([3, 2], [1, 1], [-1, 4], [0.5], [[1, 2]]):
            with pytest.raises(ValueError):
                ctx.upload_sorted_ints(bad)
        for bad in ([5000], [10, 4999, 5000], [7000]):
            d = ctx.upload_sorted_ints(bad)
            with pytest.raises(ValueError):
                ctx.csr_select_rows(dev["plain"], d)
            d.free()
        d = ctx.upload_sorted_ints([0, 1])
        with pytest.raises(ValueError):
            ctx.csr_select_rows(dev["one"], d)                    # more rows to drop than there are
        d.free()
    finally:
        for h in list(dev.values()) + [dev_big]:
            h.free()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_selection_of_vectoriser_made_rows_still_takes_the_pruned_multiply(eng, ctx, dtype):
    names = list(synth_names(20_000, seed=11))
    rng = np.random.default_rng(3)
    drop = sorted(rng.choice(len(names), 300, replace=False).tolist() + [0, 1, 2, 19_999])
    drop = sorted(set(drop))
    keep = _keep(len(names), drop)
    (want_all,), _, _ = O.tfidf_sklearn(names, [names], dtype=dtype)
    want_m = want_all[keep]
    want = P.sp_matmul_topn_port(want_m, want_m.T, 10, 0.8, True, 16)
    state = eng.corpus_fit(pd.Series(names), 3, REGEX, True, True, dtype)
    try:
        whole = state.matrix.csr
        d = ctx.upload_sorted_ints(drop)
        sel = ctx.csr_select_rows(whole, d)
        assert_same(sel.to_scipy(), want_m.tocsr(), "selected tf-idf rows")
        stats = {}
        for label, m in (("one_piece", whole), ("selected", sel)):
            idx = ctx.postings_build(m)
            res = ctx.spgemm_topn(m, idx, 10, 0.8, True)
            stats[label] = ctx.stats()
            C = res.to_scipy()
            res.free()
            idx.free()
            if label == "selected":
                assert_same(sp.csr_matrix((C.data, C.indices, C.indptr), shape=want.shape), want, label)
        assert stats["one_piece"]["prune_rows"] > 0, stats["one_piece"]
        for k in ("prune_rows", "prune_postings", "prune_survivors", "prune_scored", "prune_symmetric"):
            if stats["one_piece"][k] > 0:
                assert stats["selected"][k] > 0, (k, stats)
        sel.free()
        d.free()
    finally:
        eng.corpus_free(state)


# ------------------------------------------------------------------------------------------ sg_topn_drop_columns (C ABI)
def _random_result(rng, n_rows, stride, n_cols, dtype, dead):
    """A fixed-stride result as a multiply leaves it: per row counts[i] distinct columns, few distinct scores (many ties),
    ordered by score descending then column ascending; every seventh row names dead columns only."""
    cols = np.full((n_rows, stride), -7, np.int32)                   # (slots behind a row's count hold rubbish)
    vals = np.full((n_rows, stride), -1.0, dtype)
    counts = rng.integers(0, stride + 1, n_rows).astype(np.int32)
    counts[::5] = stride
    scores = (np.arange(1, 6) / 8.0).astype(dtype)
    for i in range(n_rows):
        c = int(min(counts[i], n_cols))
        if i % 7 == 3 and len(dead):
            c = min(c, len(dead))
            chosen = rng.choice(dead, c, replace=False)
        elif i % 7 == 5 and len(dead):                               # about half dead
            k = min(c // 2, len(dead))
            chosen = np.concatenate([rng.choice(dead, k, replace=False), rng.choice(n_cols, c - k, replace=False)])
            chosen = np.unique(chosen)
            c = len(chosen)
        else:
            chosen = rng.choice(n_cols, c, replace=False)
        counts[i] = c
        v = rng.choice(scores, c)
        order = np.lexsort((chosen, -v.astype(np.float64)))
        cols[i, :c] = chosen[order]
        vals[i, :c] = v[order]
    return cols, vals, counts


def _drop_columns_numpy(cols, vals, counts, dead, top_n):
    stride = max(min(top_n, cols.shape[1]), 1)
    out_c = np.zeros((len(counts), stride), np.int32)
    out_v = np.zeros((len(counts), stride), vals.dtype)
    out_n = np.zeros(len(counts), np.int32)
    for i, c in enumerate(counts):
        row_c, row_v = cols[i, :c], vals[i, :c]
        live = ~np.isin(row_c, dead)
        new_c = (row_c[live] - np.searchsorted(dead, row_c[live]))[:stride]
        out_n[i] = len(new_c)
        out_c[i, :len(new_c)] = new_c
        out_v[i, :len(new_c)] = row_v[live][:stride]
    return out_c, out_v, out_n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("stride", [1, 10, 64, 65, 200, 4096])
def test_topn_drop_columns_equals_its_numpy_restatement(ctx, dtype, stride):
    rng = np.random.default_rng(100 + stride)
    n_cols, n_rows = 9000, 150
    for n_dead in (1, 2, 17, 64, 300, 2500):                         # (2 500: longer than the kernel keeps in LDS)
        dead = np.sort(rng.choice(np.arange(1, n_cols - 1), n_dead, replace=False))
        if n_dead >= 2:
            dead[0], dead[-1] = 0, n_cols - 1                        # column 0 and the last one
        else:
            dead[0] = 0 if stride % 2 else n_cols - 1
        cols, vals, counts = _random_result(rng, n_rows, stride, n_cols, dtype, dead)
        res = ctx.topn_from_host(cols, vals, counts, n_cols)
        d = ctx.upload_sorted_ints(dead)
        alive = np.array([int(c - np.isin(cols[i, :c], dead).sum()) for i, c in enumerate(counts)])
        assert (alive[counts > 0] == 0).any() or n_dead < 2, "no row loses everything"
        survivors = int(alive.max())
        for top_n in sorted({1, 2, max(survivors - 1, 1), max(survivors, 1), survivors + 1, stride, stride + 10}):
            got = ctx.topn_drop_columns(res, d, top_n)
            r, s, _, c = got.dims()
            want_c, want_v, want_n = _drop_columns_numpy(cols, vals, counts, dead, top_n)
            assert (r, s, c) == (n_rows, want_c.shape[1], n_cols - len(dead)), (n_dead, top_n)
            got_c, got_v, got_n = got.to_host()
            got.free()
            what = f"stride {stride} dead {len(dead)} top_n {top_n}"
            assert np.array_equal(got_n, want_n), what
            used = np.arange(s)[None, :] < want_n[:, None]
            assert np.array_equal(got_c[used], want_c[used]), what
            assert got_v.dtype == want_v.dtype and np.array_equal(got_v[used], want_v[used]), what
        d.free()
        res.free()


# ------------------------------------------------------------------------------------------ a corpus that forgets
def _check_index_paths(eng, state, monkeypatch, dtype, mc, what, top_ns=(1, 10), thrs=(0.8, 0.5)):
    """The calls that keep tombstones: batch x corpus (resident indexes) and corpus x batch on the reverse path."""
    _, mb, ms = oracle_rows(dtype)
    Bb = eng.corpus_transform(state, pd.Series(batches()[0]))
    Bs = eng.corpus_transform(state, pd.Series(batches()[1]))
    try:
        for top_n in top_ns:
            for thr in thrs:
                tag = f"{what} {np.dtype(dtype).name} top{top_n} thr{thr}"
                for B, mB, size in ((Bb, mb, "big"), (Bs, ms, "small")):
                    want = P.sp_matmul_topn_port(mB, mc.T, top_n, thr, True, 16)
                    assert want.nnz > 0
                    assert_same(topn_host(eng, B, state.matrix, top_n, thr), want, f"{tag} {size} batch x corpus")
                    want = P.sp_matmul_topn_port(mc, mB.T, top_n, thr, True, 16)
                    monkeypatch.setenv("SG_CORPUS_REVERSE", "1")
                    before = state.stats["reverse"]
                    got = topn_host(eng, state.matrix, B, top_n, thr)
                    monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
                    assert state.stats["reverse"] == before + 1, tag
                    assert_same(got, want, f"{tag} corpus x {size} batch, reverse")
                want = P.sp_matmul_topn_port(mc, ms.T, top_n, thr, True, 16)          # auto: a small batch goes the reverse way
                before = state.stats["reverse"]
                assert_same(topn_host(eng, state.matrix, Bs, top_n, thr), want, f"{tag} corpus x small batch, auto")
                assert state.stats["reverse"] == before + 1, tag
    finally:
        Bb.csr.free()
        Bs.csr.free()


def _check_one_matrix_paths(eng, state, monkeypatch, dtype, mc, what, top_n=10, thr=0.8, self_join=True):
    """The calls that need the rows in one matrix: corpus x batch on the forward path, the self-join, the rows themselves."""
    _, mb, _ = oracle_rows(dtype)
    Bb = eng.corpus_transform(state, pd.Series(batches()[0]))
    try:
        monkeypatch.setenv("SG_CORPUS_REVERSE", "0")
        before = state.stats["forward"]
        got = topn_host(eng, state.matrix, Bb, top_n, thr)
        monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
        assert state.stats["forward"] == before + 1
        assert_same(got, P.sp_matmul_topn_port(mc, mb.T, top_n, thr, True, 16), f"{what}: corpus x big batch, forward")
        if self_join:
            want = P.sp_matmul_topn_port(mc, mc.T, top_n, thr, True, 16)
            assert_same(topn_host(eng, state.matrix, state.matrix, top_n, thr), want, f"{what}: self-join")
    finally:
        Bb.csr.free()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_removes_in_both_segments_with_tombstones_pending_equal_the_oracle(eng, monkeypatch, dtype):
    monkeypatch.setattr(eng, "CORPUS_COMPACT_SHARE", 1.0)          # no automatic compaction in this test
    monkeypatch.setattr(eng, "CORPUS_MAX_DEAD", 10_000)
    m_all = oracle_rows(dtype)[0].tocsr()
    n_base, n_all = len(base_names()), m_all.shape[0]
    big, small = batches()
    grown = list(base_names()) + sum((list(x) for x in growth()), [])
    at = {s: i for i, s in reversed(list(enumerate(grown)))}       # first row of every string
    # rows the batches' names match best (so that a filter that forgot them shows), the first and the last physical row,
    # neighbours, and rows of every appended part
    first = sorted({0, 1, 2, 3, 17, n_base - 1, n_base, n_base + 1, n_base + 5, n_all - 1, n_all - 2} |
                   {at[s] for s in list(small) + list(big[::9]) if s in at})
    state = eng.corpus_fit(pd.Series(base_names()), 3, REGEX, True, True, dtype)
    try:
        for x in growth():
            eng.corpus_append(state, pd.Series(x))
        _check_index_paths(eng, state, monkeypatch, dtype, m_all, "nothing removed yet", top_ns=(10,), thrs=(0.8,))
        builds = dict(state.stats)
        assert builds["base_index_builds"] == 1 and builds["index_builds"] == 2
        eng.corpus_remove(state, np.array(first))
        keep = _keep(n_all, first)
        assert (~keep[:n_base]).sum() > 4 and (~keep[n_base:]).sum() > 4
        assert state.matrix.shape == (int(keep.sum()), m_all.shape[1])
        assert state.stats["dead_rows"] == len(first) and state.stats["removals"] == 1
        _check_index_paths(eng, state, monkeypatch, dtype, m_all[keep], "first remove pending")
        # a second remove names LIVE rows: the rows left are numbered through the shorter list
        live = np.flatnonzero(keep)
        second = np.array(sorted({0, 1, 5, 100, 101, 102, len(live) - 1, len(live) - 40, int(np.searchsorted(live, n_base)) + 7}))
        eng.corpus_remove(state, second)
        keep[live[second]] = False
        assert state.stats["dead_rows"] == len(first) + len(second) and state.matrix.shape[0] == int(keep.sum())
        _check_index_paths(eng, state, monkeypatch, dtype, m_all[keep], "two removes pending")
        st = state.stats
        assert st["compactions"] == 0 and st["segments"] == 2, st
        assert st["base_index_builds"] == 1 and st["index_builds"] == 2, st      # nothing was rebuilt for a remove
        assert state.matrix.nnz == m_all[keep].nnz
        # the forward path needs the rows in one matrix: it compacts, once
        _check_one_matrix_paths(eng, state, monkeypatch, dtype, m_all[keep], "forward compacts", self_join=False)
        st = state.stats
        assert st["compactions"] == 1 and st["segments"] == 1 and st["dead_rows"] == 0, st
        assert_same(state.matrix.to_scipy(), m_all[keep], "rows after the compaction")
        _check_one_matrix_paths(eng, state, monkeypatch, dtype, m_all[keep], "compacted")
        assert state.stats["compactions"] == 1
        # tombstones again, then the self-join: it compacts, once
        live = np.flatnonzero(keep)
        third = np.array([0, 7, len(live) - 1])
        eng.corpus_remove(state, third)
        keep[live[third]] = False
        want = P.sp_matmul_topn_port(m_all[keep], m_all[keep].T, 10, 0.8, True, 16)
        assert_same(topn_host(eng, state.matrix, state.matrix, 10, 0.8), want, "self-join compacts")
        assert state.stats["compactions"] == 2 and state.stats["dead_rows"] == 0
        # ... and to_scipy() of the rows
        live = np.flatnonzero(keep)
        eng.corpus_remove(state, np.array([3]))
        keep[live[3]] = False
        assert state.stats["dead_rows"] == 1
        assert_same(state.matrix.to_scipy(), m_all[keep], "to_scipy compacts")
        assert state.stats["compactions"] == 3
        # an explicit compact() with removes and an append pending; the same checks on one clean segment
        live = np.flatnonzero(keep)
        eng.corpus_remove(state, np.array([11, 12]))
        keep[live[[11, 12]]] = False
        eng.corpus_append(state, pd.Series(growth()[1]))
        rows = sp.vstack([m_all[keep], m_all[n_base + 1:n_base + 1 + len(growth()[1])]], format="csr")
        eng.corpus_remove(state, np.array([rows.shape[0] - 1]))     # the last appended row, numbered through the live rows
        rows = rows[:-1]
        _check_index_paths(eng, state, monkeypatch, dtype, rows, "append and removes pending", top_ns=(10,), thrs=(0.8,))
        assert state.stats["compactions"] == 3 and state.stats["dead_rows"] == 3 and state.stats["segments"] == 2
        eng.corpus_compact(state)
        assert state.stats["compactions"] == 4 and state.stats["dead_rows"] == 0 and state.stats["segments"] == 1
        _check_index_paths(eng, state, monkeypatch, dtype, rows, "after compact()")
        _check_one_matrix_paths(eng, state, monkeypatch, dtype, rows, "after compact()")
        st = state.stats
        assert st["compactions"] == 4 and st["base_index_builds"] <= 1 + st["compactions"] and st["tokenisations"] == 1, st
    finally:
        eng.corpus_free(state)


def test_a_hub_whose_lowest_rows_are_removed_names_the_next_lowest_live_rows(eng, monkeypatch):
    """The case the over-ask exists for: 40 identical names, top_n 10 and 30, the 8 lowest removed.  A multiply asked for
    top_n alone would return the lowest rows, dead ones among them, and come back short after the filter."""
    monkeypatch.setattr(eng, "CORPUS_COMPACT_SHARE", 1.0)
    monkeypatch.setattr(eng, "CORPUS_MAX_DEAD", 10_000)
    rng = np.random.default_rng(2)
    base = list(base_names())
    hub = "NORTHERN LIGHTS HOLDING CO"
    for at in rng.choice(len(base), 25, replace=False):
        base[at] = hub
    x1 = list(synth_names(300, seed=71))
    for at in rng.choice(len(x1), 15, replace=False):
        x1[at] = hub
    twin = "SOUTHERN CROSS TRADING PARTNERS"
    base[100] = base[2000] = twin                                  # a pair of identical rows: one collapse group
    grown = base + x1
    hub_rows = [i for i, s in enumerate(grown) if s == hub]
    drop = sorted(hub_rows[:8] + [100])
    keep = _keep(len(grown), drop)
    left = [s for s, k in zip(grown, keep) if k]
    batch = [hub] * 50 + [hub + " inc", hub.lower(), twin, "", twin + "."] * 6 + list(synth_names(40, seed=72, perturb_of=grown, perturb_frac=0.5))
    for dtype in (np.float32, np.float64):
        (m_all, mn), _, _ = O.tfidf_sklearn(base, [grown, batch], dtype=dtype)
        mc = m_all.tocsr()[keep]
        state = eng.corpus_fit(pd.Series(base), 3, REGEX, True, True, dtype)
        try:
            eng.corpus_append(state, pd.Series(x1))
            B = eng.corpus_transform(state, pd.Series(batch))
            # with the indexes built BEFORE the remove: nothing may be rebuilt for it
            topn_host(eng, B, state.matrix, 10, 0.6).nnz
            eng.corpus_remove(state, np.array(drop))
            live_hub = [i for i, s in enumerate(left) if s == hub]
            assert len(live_hub) == 32 and state.stats["dead_rows"] == 9
            for top_n in (10, 30):
                want = P.sp_matmul_topn_port(mn, mc.T, top_n, 0.6, True, 16)
                row = want.getrow(0)
                assert row.nnz == top_n and (row.data == row.data[0]).all() and list(row.indices) == live_hub[:top_n]
                got = topn_host(eng, B, state.matrix, top_n, 0.6)
                assert got.getrow(0).nnz == top_n, "short: the multiply was not asked for top_n + dead rows"
                assert_same(got, want, f"hub, batch x corpus, top {top_n}")
                # the twin's surviving member (row 2000, now renumbered) still answers the batch's copies
                twin_live = left.index(twin)
                assert twin_live in set(got.getrow(52).indices) and left.count(twin) == 1
                want = P.sp_matmul_topn_port(mc, mn.T, top_n, 0.6, True, 16)
                assert all(want.getrow(i).nnz == top_n for i in live_hub)
                monkeypatch.setenv("SG_CORPUS_REVERSE", "1")
                assert_same(topn_host(eng, state.matrix, B, top_n, 0.6), want, f"hub, corpus x batch, reverse, top {top_n}")
                monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
                assert state.stats["compactions"] == 0 and state.stats["base_index_builds"] == 1
            monkeypatch.setenv("SG_CORPUS_REVERSE", "0")           # the forward path: compacts, same result
            for top_n in (10, 30):
                want = P.sp_matmul_topn_port(mc, mn.T, top_n, 0.6, True, 16)
                assert_same(topn_host(eng, state.matrix, B, top_n, 0.6), want, f"hub, corpus x batch, forward, top {top_n}")
            monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
            assert state.stats["compactions"] == 1 and state.stats["dead_rows"] == 0
            B.csr.free()
        finally:
            eng.corpus_free(state)


def test_crossing_the_cap_of_dead_rows_compacts_once_not_per_remove(eng):
    from tests.test_corpus_cpu import _expected
    base = pd.Series(base_names(), name="name")
    cap = eng.CORPUS_MAX_DEAD
    batch = pd.Series(synth_names(50, seed=64, perturb_of=list(base[:500]), perturb_frac=0.5))
    with sga.Corpus(base, min_similarity=0.6) as cp:
        cp.match_strings(batch, cp.master)
        left = base
        for k, (rows, compactions, dead) in enumerate([(range(10, 10 + cap - 12), 0, cap - 12), ([0, 1, -1, 5, 6, 7, 8, 9, 300, 301, 302, 303], 0, cap),
                                                       ([42], 1, 0), ([42], 1, 1), ([0, 1], 1, 3)]):
            rows = list(rows)
            cp.remove(rows)
            left = left[_keep(len(left), rows)]
            st = cp.stats
            assert (st["compactions"], st["dead_rows"], st["removals"]) == (compactions, dead, k + 1), (k, st)
            pd.testing.assert_series_equal(cp.master, left)
            pd.testing.assert_frame_equal(cp.match_strings(batch, cp.master), _expected(list(base), "match_strings", batch, left, min_similarity=0.6))
            pd.testing.assert_frame_equal(cp.match_strings(cp.master, batch[:7]), _expected(list(base), "match_strings", left, batch[:7], min_similarity=0.6))
            assert cp.stats["compactions"] == compactions        # (neither call needed the rows in one matrix)
        assert cp.stats["base_index_builds"] == 2 and cp.stats["tokenisations"] == 1
        # a top_n whose over-ask goes beyond what the pruned multiply holds a row (128): the wider form, the same answer
        assert cp.stats["dead_rows"] == 3
        pd.testing.assert_frame_equal(cp.match_strings(batch, cp.master, max_n_matches=126),
                                      _expected(list(base), "match_strings", batch, left, min_similarity=0.6, max_n_matches=126))
        assert cp.stats["compactions"] == 1 and cp.stats["dead_rows"] == 3


def test_two_hundred_steps_of_a_living_list_never_reindex_per_step(eng):
    from tests.test_corpus_cpu import _expected
    base = pd.Series(base_names(), name="name")
    rows = synth_names(200, seed=81, perturb_of=list(base[:2000]), perturb_frac=0.5)
    queries = synth_names(200, seed=82, perturb_of=rows, perturb_frac=0.5)
    queries[-1] = rows[-1]                       # the last query is answered by the row appended just before it
    rng = np.random.default_rng(9)
    left = base
    with sga.Corpus(base, min_similarity=0.5) as cp:
        for i, (r, q) in enumerate(zip(rows, queries)):
            at = int(rng.integers(0, len(left))) if i % 3 else len(left) - 1      # every third step: the row appended last
            cp.remove(at)
            left = left[_keep(len(left), [at])]
            cp.append(pd.Series([r], name="name"))
            left = pd.concat([left, pd.Series([r], name="name")])
            got = cp.match_strings(cp.master, pd.Series([q]))
        st = cp.stats
        pd.testing.assert_series_equal(cp.master, left)
        pd.testing.assert_frame_equal(got, _expected(list(base), "match_strings", left, pd.Series([queries[-1]]), min_similarity=0.5))
        assert ((got.left_name == rows[-1]) & (got.similarity > 0.999)).any()
        pd.testing.assert_frame_equal(cp.match_strings(pd.Series(queries[-20:]), cp.master),
                                      _expected(list(base), "match_strings", pd.Series(queries[-20:]), left, min_similarity=0.5))
    assert st["tokenisations"] == 1 and st["removals"] == 200 and st["rows_removed"] == 200 and st["appends"] == 200
    assert st["base_index_builds"] <= 1 + st["compactions"], st
    assert 1 <= st["compactions"] <= 200 // eng.CORPUS_MAX_DEAD + 1 and st["reverse"] == 200, st


def test_close_after_removes_appends_and_compactions_frees_what_the_corpus_held(eng, ctx):
    import torch
    names = synth_names(713_000, seed=11)
    corpus, more = pd.Series(names[:663_000]), pd.Series(names[663_000:])
    batch = pd.Series(synth_names(100, seed=12, perturb_of=names[600_000:], perturb_frac=0.5))
    ctx.trim()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    cp = sga.Corpus(corpus, min_similarity=0.8)
    cp.match_strings(corpus, batch)
    cp.remove([0, 5, 600_000])
    cp.match_strings(batch, cp.master)                        # tombstones against the index
    cp.append(more[:20_000])
    cp.remove(np.arange(662_990, 663_010))                    # rows of both segments
    cp.match_strings(cp.master, batch[:5])                    # reverse, tombstones pending
    cp.match_strings(cp.master, batch)                        # forward: compacts
    cp.append(more[20_000:])
    cp.remove(np.arange(100, 100 + eng.CORPUS_MAX_DEAD + 1))  # crosses the cap: compacts
    cp.match_strings(batch, cp.master)
    cp.remove([-1, 0])
    cp.compact()
    cp.match_strings(cp.master, batch)
    cp.remove(7)                                              # a dead list is pending when the corpus closes
    st = cp.stats
    assert st["segments"] == 1 and st["compactions"] >= 3 and st["dead_rows"] == 1
    assert len(cp.master) == 713_000 - 3 - 20 - (eng.CORPUS_MAX_DEAD + 1) - 2 - 1
    held = free0 - torch.cuda.mem_get_info(0)[0]
    cp.close()
    ctx.trim()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert held > 0
    assert abs(free1 - free0) <= 0.01 * free0, (free0, free1, held)
