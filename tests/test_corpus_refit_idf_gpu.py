"""GPU tests of Corpus.refit_idf and of the device operations under it: sg_csr_column_counts, the row norms K2 leaves and
sg_csr_concat / sg_csr_select_rows carry, and sg_vec_reweigh.  Every comparison is bit for bit: the counts against
np.bincount, the norms and the reweighed rows against the numpy restatement and sklearn fitted with the vocabulary fixed
(tests/_corpus_refit_oracle.py), the corpus against that oracle plus sparse_dot_topn's multiply (oracle/port.py)."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from oracle import oracle as O
from string_grouper_amd.synth import synth_names
from string_grouper_amd.vectorizer import HipTfidfVectorizer, idf_from_df
from tests import _corpus_refit_oracle as R

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
LDS_COLUMNS = 30 * 1024                                  # counters of one pass of the column count


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_matrix(got, want, what=""):
    assert got.shape == want.shape, what
    assert np.array_equal(np.asarray(got.indptr, np.int64), np.asarray(want.indptr, np.int64)), f"{what}: row pointers differ"
    assert np.array_equal(got.indices, want.indices), f"{what}: columns differ"
    assert got.data.dtype == want.data.dtype and np.array_equal(_bits(got.data), _bits(want.data)), f"{what}: values differ"


def _fitted(ctx, strings, dtype):
    vec = HipTfidfVectorizer(dtype=dtype, ctx=ctx)
    vec.fit_prepared([vec.prepare(pd.Series(list(strings)))])
    return vec


def _rows(vec, strings):
    return vec.transform_prepared(vec.prepare(pd.Series(list(strings))))


# ------------------------------------------------------------------------------------------ sg_csr_column_counts
def _counted(rng, n_rows, n_cols, dtype=np.float32):
    """Rows of 0 .. 40 distinct columns (every fifth row empty), column 0 in every other row: many adds to one LDS word."""
    indptr, indices = [0], []
    for r in range(n_rows):
        k = 0 if r % 5 == 4 else int(rng.integers(1, 41))
        cols = set(rng.integers(0, n_cols, k).tolist())
        if k:
            cols.add(0)
        indices += sorted(cols)
        indptr.append(len(indices))
    data = np.ones(len(indices), dtype)
    return sp.csr_matrix((data, np.array(indices, np.int32), np.array(indptr, np.int64)), shape=(n_rows, n_cols))


@pytest.mark.parametrize("n_cols", [1, LDS_COLUMNS, LDS_COLUMNS + 1])
@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, 1025])
def test_column_counts_of_caller_made_matrices_equal_bincount(ctx, n_rows, n_cols):
    rng = np.random.default_rng(n_rows * 7 + n_cols)
    m = _counted(rng, n_rows, n_cols)
    if n_cols > 1:
        m = m.tolil()
        m[0, n_cols - 1] = 1.0                               # the last counter of the last pass
        m = m.tocsr()
        m.sort_indices()
    dev = ctx.csr_from_scipy(m)
    want = np.bincount(m.indices, minlength=n_cols)
    assert want[0] >= (n_rows + 1) // 2 or n_rows < 5
    got = dev.column_counts()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # views: the first entry of the range lies at every offset of a 16-byte unit, the last one too
    for r0 in range(0, min(n_rows, 5)):
        for r1 in sorted({r0, r0 + 1, n_rows - 1, n_rows} & set(range(r0, n_rows + 1))):
            view = dev.row_block(r0, r1)
            assert np.array_equal(view.column_counts(), np.bincount(m[r0:r1].indices, minlength=n_cols)), (r0, r1)
            view.free()
    dev.free()


def test_column_counts_of_views_that_start_at_every_offset_of_a_unit(ctx):
    rng = np.random.default_rng(5)
    body = _counted(rng, 300, 700)
    head = sp.csr_matrix((np.ones(3, np.float32), np.array([5, 6, 7], np.int32), np.array([0, 1, 2, 3], np.int64)), shape=(3, 700))
    m = sp.vstack([head, body], format="csr", dtype=np.float32)
    dev = ctx.csr_from_scipy(m)
    for r0 in (1, 2, 3):                                     # the view's first entry is entry 1, 2, 3 of the parent's array
        assert m.indptr[r0] % 4 == r0
        for r1 in (r0, r0 + 1, 200, 303):
            view = dev.row_block(r0, r1)
            assert np.array_equal(view.column_counts(), np.bincount(m[r0:r1].indices, minlength=700)), (r0, r1)
            view.free()
    dev.free()


def test_column_counts_of_a_column_every_row_names(ctx):
    """No empty row, one column in all of them: every lane of every workgroup adds to the same LDS word."""
    rng = np.random.default_rng(11)
    n_rows, n_cols = 40_000, 50
    others = rng.integers(8, n_cols, (n_rows, 3))
    indices = np.sort(np.concatenate([np.full((n_rows, 1), 7), others], axis=1), axis=1)
    keep = np.concatenate([np.ones((n_rows, 1), bool), indices[:, 1:] != indices[:, :-1]], axis=1)      # a column once a row
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    m = sp.csr_matrix((np.ones(int(keep.sum()), np.float32), indices[keep].astype(np.int32), indptr), shape=(n_rows, n_cols))
    dev = ctx.csr_from_scipy(m)
    got = dev.column_counts()
    assert got[7] == n_rows and np.array_equal(got, np.bincount(m.indices, minlength=n_cols))
    dev.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_counts_of_a_transform_are_its_document_frequencies(ctx, dtype):
    original, appended, removed, live = R.bite_list()
    vec = _fitted(ctx, original, dtype)
    m = _rows(vec, original)
    _, df = ctx.vocab_to_host(vec._vocab)
    assert np.array_equal(m.column_counts(), df)
    live_rows = _rows(vec, live)
    assert np.array_equal(live_rows.column_counts(), np.bincount(live_rows.to_scipy().indices, minlength=len(df)))


# ------------------------------------------------------------------------------------------ row norms
def _restated(original, strings, dtype):
    (_,), vocab, idf = O.tfidf_sklearn(original, [original], dtype=dtype)
    _, counts = O.count_matrix(list(strings), vocab, dtype)
    counts = counts.tocsr()
    values, norms = R.k2_restated(counts, idf, dtype)
    return counts, values, norms, idf, vocab


@pytest.mark.parametrize("plain", [False, True], ids=["rows16", "plain"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_transform_leaves_the_norm_it_divided_every_row_by(ctx, dtype, plain):
    original, appended, removed, live = R.bite_list()
    if plain:
        ctx.set_option("SG_K2_PLAIN", "1")
    vec = _fitted(ctx, original, dtype)
    for strings in (original, live, ["", "!!??"], [live[0]]):
        counts, values, norms, _, _ = _restated(original, strings, dtype)
        m = _rows(vec, strings)
        got = m.row_norms()
        assert got is not None and got.dtype == np.float64 and len(got) == len(strings)
        assert np.array_equal(_bits(got), _bits(norms))
        assert (got[np.diff(counts.indptr) == 0] == 0.0).all()
        assert np.array_equal(_bits(m.to_scipy().data), _bits(values))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_norms_travel_through_concat_and_select_rows(ctx, dtype):
    original, appended, removed, live = R.bite_list()
    vec = _fitted(ctx, original, dtype)
    a, b, c = _rows(vec, original), _rows(vec, appended), _rows(vec, [live[7]])
    na, nb, nc = a.row_norms(), b.row_norms(), c.row_norms()
    view = a.row_block(3, 11)
    assert np.array_equal(_bits(view.row_norms()), _bits(na[3:11]))               # a view shares the parent's, shifted
    for what, parts, want in [("two", [a, b], [na, nb]), ("three", [a, b, c], [na, nb, nc]),
                              ("a view as a part", [b, view, a], [nb, na[3:11], na]), ("a part of one row", [c, a], [nc, na]),
                              ("one row alone", [c], [nc])]:
        cat = ctx.csr_concat(parts)
        assert np.array_equal(_bits(cat.row_norms()), _bits(np.concatenate(want))), what
        cat.free()
    n = len(original)
    for what, drop in [("first", [0]), ("last", [n - 1]), ("two adjacent", [4, 5]), ("every second", list(range(0, n, 2))),
                       ("none", []), ("all but one", [r for r in range(n) if r != 9])]:
        d = ctx.upload_sorted_ints(drop)
        sel = ctx.csr_select_rows(a, d)
        assert np.array_equal(_bits(sel.row_norms()), _bits(np.delete(na, drop))), what
        sel.free()
        d.free()
    d = ctx.upload_sorted_ints([0, 2])
    sel = ctx.csr_select_rows(view, d)                                               # a selection of a view
    assert np.array_equal(_bits(sel.row_norms()), _bits(np.delete(na[3:11], [0, 2])))
    # matrices the caller made carry none, and neither does a concatenation with one
    host = ctx.csr_from_scipy(a.to_scipy())
    assert host.row_norms() is None and host.row_block(1, 5).row_norms() is None
    assert ctx.csr_concat([a, host]).row_norms() is None and ctx.csr_concat([host, b]).row_norms() is None
    assert ctx.csr_select_rows(host, d).row_norms() is None


# ------------------------------------------------------------------------------------------ sg_vec_reweigh
def _refit(vec, m):
    """counts -> numpy's idf -> reweigh, by hand (what HipTfidfVectorizer.refit_idf_prepared does)."""
    df = m.column_counts().astype(np.int64)
    n_docs = m.dims()[0]
    idf = idf_from_df(df, n_docs, vec.dtype)
    return vec.ctx.vec_reweigh(vec._vocab, m, df, n_docs, idf), df, idf


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_identity_refit_changes_no_bit(ctx, dtype):
    original, _, _, _ = R.bite_list()
    vec = _fitted(ctx, original, dtype)
    idf0 = vec.idf_.copy()
    m = _rows(vec, original)
    out, df, idf = _refit(vec, m)
    assert np.array_equal(_bits(idf), _bits(idf0)) and np.array_equal(df, ctx.vocab_to_host(vec._vocab)[1])
    _same_matrix(out.to_scipy(), m.to_scipy(), "identity refit")
    assert np.array_equal(_bits(out.row_norms()), _bits(m.row_norms()))
    assert out.dims() == m.dims()


@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, None])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reweighed_rows_equal_sklearn_fitted_with_the_vocabulary_fixed(ctx, dtype, n_rows):
    original, appended, removed, live = R.bite_list()
    # the rows built to bite first: the long one, the counts far from one, rows of 16, 17, 32, 33 entries, an empty one
    order = sorted(range(len(live)), key=lambda i: (live[i] not in original[2:12] and live[i] != "!!??", i))
    current = [live[i] for i in order][:n_rows]
    vec = _fitted(ctx, original, dtype)
    m = _rows(vec, current)
    held, norms0 = m.to_scipy(), m.row_norms()
    out, df, idf = _refit(vec, m)
    (want,), vocab, want_idf = R.fixed_vocabulary_matrices(original, current, [current], dtype=dtype)
    assert np.array_equal(_bits(idf), _bits(want_idf))
    _same_matrix(out.to_scipy(), want, f"{len(current)} rows")
    values, norms, _, failed = R.reweigh_restated(held, norms0, vec_idf_before(original, dtype), idf)
    assert failed == 0 and np.array_equal(_bits(out.row_norms()), _bits(norms))
    # the input was only read
    _same_matrix(m.to_scipy(), held, "the input")
    assert np.array_equal(_bits(m.row_norms()), _bits(norms0))
    # the vocabulary holds the new counts and weights: what it reports, and what a batch is transformed with
    keys, got_df = ctx.vocab_to_host(vec._vocab)
    assert np.array_equal(got_df, df) and ctx.vocab_size(vec._vocab)[1] == len(current)
    batch = list(appended) + list(original[:20])
    (want_batch,), _, _ = R.fixed_vocabulary_matrices(original, current, [batch], dtype=dtype)
    _same_matrix(_rows(vec, batch).to_scipy(), want_batch, "a batch after the refit")
    # ... and a second refit starts from the norms the first one left
    again, _, idf2 = _refit(vec, out)
    assert np.array_equal(_bits(idf2), _bits(idf))
    _same_matrix(again.to_scipy(), want, "refit of the refit")


def vec_idf_before(original, dtype):
    (_,), _, idf = O.tfidf_sklearn(original, [original], dtype=dtype)
    return idf


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_words_a_reweigh_leaves_are_a_fresh_transforms(ctx, dtype):
    original, appended, removed, live = R.bite_list()
    ctx.set_option("SG_ROW_BLOCKS", "1")                     # K2 leaves its three words only for the opt-in row blocks
    vec = _fitted(ctx, original, dtype)
    m = _rows(vec, live)
    assert m.vectoriser_words() is not None
    out, _, _ = _refit(vec, m)
    fresh = _rows(vec, live)                                 # under the idf the refit installed
    _same_matrix(out.to_scipy(), fresh.to_scipy(), "reweigh against a fresh transform")
    got, want = out.vectoriser_words(), fresh.vectoriser_words()
    assert got == want and got[0] == 0 and got[2] == int(np.diff(fresh.to_scipy().indptr).max()) and 0.9999 < got[1] < 1.0001


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_refused_reweigh_installs_nothing(ctx, dtype):
    original, appended, removed, live = R.bite_list()
    vec = _fitted(ctx, original, dtype)
    m = _rows(vec, live)
    n_terms = ctx.vocab_size(vec._vocab)[0]
    df = m.column_counts().astype(np.int64)
    idf = idf_from_df(df, len(live), dtype)
    before_df, before_rows, before_docs = ctx.vocab_to_host(vec._vocab)[1].copy(), _rows(vec, appended).to_scipy(), len(original)

    def unchanged(what):
        assert np.array_equal(ctx.vocab_to_host(vec._vocab)[1], before_df), what
        assert ctx.vocab_size(vec._vocab) == (n_terms, before_docs), what
        _same_matrix(_rows(vec, appended).to_scipy(), before_rows, what)

    host = ctx.csr_from_scipy(m.to_scipy())                  # the same rows without norms
    with pytest.raises(ValueError, match="no row norms"):
        ctx.vec_reweigh(vec._vocab, host, df, len(live), idf)
    unchanged("a matrix without norms")
    other = _fitted(ctx, ["abcdefgh", "bcdefghi"], dtype)    # another vocabulary: another width
    narrow = _rows(other, ["abcdefgh"])
    assert narrow.dims()[1] != n_terms
    with pytest.raises(ValueError, match="columns are not the vocabulary's"):
        ctx.vec_reweigh(vec._vocab, narrow, df, len(live), idf)
    unchanged("a matrix of the wrong width")
    for bad in (np.inf, np.nan, 0.0, -1.0):
        worse = idf.copy()
        worse[n_terms // 2] = bad
        with pytest.raises(ValueError, match="not positive and finite"):
            ctx.vec_reweigh(vec._vocab, m, df, len(live), worse)
        unchanged(f"an idf that holds {bad}")
    with pytest.raises(ValueError):                          # the other value type
        ctx.vec_reweigh(vec._vocab, m, df, len(live), idf.astype(np.float64 if dtype == np.float32 else np.float32))
    unchanged("an idf of the other type")
    # the idf changed under the matrix: its entries are no whole counts of the idf the vocabulary holds now
    idf_fit = vec.idf_.copy()
    ctx.vocab_set_idf(vec._vocab, (idf_fit * dtype(1.5)).astype(dtype))
    before_rows = _rows(vec, appended).to_scipy()
    with pytest.raises(NotImplementedError, match="another idf"):
        ctx.vec_reweigh(vec._vocab, m, df, len(live), idf)
    unchanged("a matrix made under another idf")
    ctx.vocab_set_idf(vec._vocab, idf_fit)
    # a good call works afterwards
    out = ctx.vec_reweigh(vec._vocab, m, df, len(live), idf)
    (want,), _, _ = R.fixed_vocabulary_matrices(original, live, [live], dtype=dtype)
    _same_matrix(out.to_scipy(), want, "the good call after the refusals")
    assert np.array_equal(ctx.vocab_to_host(vec._vocab)[1], df) and ctx.vocab_size(vec._vocab)[1] == len(live)


# ------------------------------------------------------------------------------------------ Corpus, end to end
def _living_list():
    base = list(synth_names(2500, seed=21))
    more = list(synth_names(200, seed=22)) + list(synth_names(96, seed=23, perturb_of=base[:600], perturb_frac=0.5))
    more += ["", "!!??", base[3], base[2499]]
    grown = base + more
    n = len(grown)
    drop = sorted({0, 1, 2, 17, 18, 2498, 2499, 2500, 2501, n - 1, n - 2, n - 3} | set(range(300, 328)))
    assert len(more) == 300 and len(drop) == 40
    batch = list(synth_names(60, seed=24, perturb_of=grown, perturb_frac=0.5)) + ["", grown[5], grown[2600]]
    return base, more, drop, batch


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_living_corpus_after_refit_idf_equals_the_fixed_vocabulary_oracle(eng, monkeypatch, dtype):
    monkeypatch.setattr(eng, "CORPUS_COMPACT_SHARE", 1.0)     # the appended rows and the removed ones are still pending
    monkeypatch.setattr(eng, "CORPUS_MAX_DEAD", 10_000)       # when the refit comes: it compacts
    base, more, drop, batch = _living_list()
    grown = pd.concat([pd.Series(base, name="name"), pd.Series(more, name="name")])      # (labels as Corpus.append joins them)
    keep = np.ones(len(grown), bool)
    keep[drop] = False
    left = grown[keep]
    big, small = pd.Series(batch), pd.Series(batch[:9])
    kw = dict(min_similarity=0.6, tfidf_matrix_dtype=dtype)

    def want(current, method, *args, **k):
        return R.expected_after_refit(base, list(current), method, *args, **dict(kw, **k))

    def same(got, expected, what):
        (pd.testing.assert_frame_equal if isinstance(got, pd.DataFrame) else pd.testing.assert_series_equal)(got, expected)
        assert len(got) > 0, what

    with sga.Corpus(pd.Series(base, name="name"), **kw) as cp:
        cp.keep_self_join()
        cp.group_similar_strings(cp.master)
        cp.append(pd.Series(more, name="name"))
        cp.remove(drop)
        assert cp.stats["dead_rows"] == 40 and cp.stats["segments"] == 2 and cp.stats["self_join_full"] == 1
        cp.refit_idf()
        st = cp.stats
        assert st["idf_refits"] == 1 and st["dead_rows"] == 0 and st["segments"] == 1 and st["tokenisations"] == 1
        master = cp.master
        pd.testing.assert_series_equal(master, left)
        _, _, want_idf = R.fixed_vocabulary_matrices(base, list(left), [], dtype=dtype)
        assert np.array_equal(_bits(cp.vectorizer.idf_), _bits(want_idf))
        same(cp.match_strings(master), want(left, "match_strings", left), "self-join")
        st = cp.stats
        assert st["self_join_full"] == 2 and st["self_join_served"] == 2, st        # kept before, multiplied anew, served
        same(cp.group_similar_strings(master), want(left, "group_similar_strings", left), "groups")
        assert cp.stats["self_join_full"] == 2 and cp.stats["self_join_served"] == 3
        for reverse in ("1", "0"):
            monkeypatch.setenv("SG_CORPUS_REVERSE", reverse)
            same(cp.match_strings(master, small), want(left, "match_strings", left, small), f"corpus x batch, reverse={reverse}")
            same(cp.match_strings(master, big), want(left, "match_strings", left, big), f"corpus x batch, reverse={reverse}")
        monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)
        assert cp.stats["reverse"] >= 2 and cp.stats["forward"] >= 2
        same(cp.match_strings(big, master), want(left, "match_strings", big, left), "batch x corpus")
        same(cp.match_most_similar(master, big), want(left, "match_most_similar", left, big), "most similar")
        other = pd.Series(list(left)[::-1])
        same(cp.compute_pairwise_similarities(master, other), want(left, "compute_pairwise_similarities", left, other), "pairwise")
        # the list lives on under the new idf, then is refitted again
        extra = pd.Series(list(synth_names(50, seed=25)) + [base[7]], name="name")
        cp.append(extra)
        left2 = pd.concat([left, extra])
        drop2 = [0, 1, len(left2) - 1, len(left2) - 2, 1234]
        cp.remove(drop2)
        keep2 = np.ones(len(left2), bool)
        keep2[drop2] = False
        left2 = left2[keep2]
        same(cp.match_strings(cp.master, big), want(left, "match_strings", left2, big), "after the refit: append and remove")
        same(cp.match_strings(cp.master), want(left, "match_strings", left2), "the kept self-join follows")
        full = cp.stats["self_join_full"]
        cp.refit_idf()
        pd.testing.assert_series_equal(cp.master, left2)
        same(cp.match_strings(cp.master, big), want(left2, "match_strings", left2, big), "second refit, batch")
        same(cp.match_strings(cp.master), want(left2, "match_strings", left2), "second refit, self-join")
        st = cp.stats
        assert st["idf_refits"] == 2 and st["tokenisations"] == 1 and st["self_join_full"] == full + 1, st


@pytest.mark.parametrize("dtype", DTYPES)
def test_refit_idf_on_an_untouched_corpus_changes_no_bit(eng, dtype):
    base = pd.Series(synth_names(2500, seed=21), name="name")
    with sga.Corpus(base, tfidf_matrix_dtype=dtype) as cp:
        rows0, idf0 = cp._state.matrix.to_scipy(), cp.vectorizer.idf_.copy()
        _, df0 = eng.ctx.vocab_to_host(cp.vectorizer._vocab)
        cp.refit_idf()
        _same_matrix(cp._state.matrix.to_scipy(), rows0, "rows after a refit of an untouched corpus")
        assert np.array_equal(_bits(cp.vectorizer.idf_), _bits(idf0))
        assert np.array_equal(eng.ctx.vocab_to_host(cp.vectorizer._vocab)[1], df0)
        assert cp.master is base and cp.stats["idf_refits"] == 1 and cp.stats["tokenisations"] == 1
    with pytest.raises(ValueError, match="the corpus is closed"):
        cp.refit_idf()
