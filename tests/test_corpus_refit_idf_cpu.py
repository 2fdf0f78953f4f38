"""CPU tests of Corpus.refit_idf: the host logic of ``Corpus`` on the engine double that refits with sklearn
(tests/_corpus_refit_oracle.py), and the numpy restatement of what the device does instead of reading the strings again --
recover every entry's whole count from the entry, its row's norm and the old idf, verify it, weight it with the new idf,
normalise by a sum taken in column order in double -- held to sklearn bit for bit, together with the wrong turns such a
restatement could take, each of which must change the answer.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from oracle import oracle as O
from tests import _corpus_refit_oracle as R
from tests._corpus_remove_oracle import RemoveCorpusOracleEngine
from tests.test_corpus_append_cpu import X1, X2
from tests.test_corpus_cpu import CORPUS, NEW, _expected

DTYPES = [np.float32, np.float64]


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


def _same(got, want):
    (pd.testing.assert_frame_equal if isinstance(got, pd.DataFrame) else pd.testing.assert_series_equal)(got, want)
    assert len(got) > 0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _corpus(**kwargs):
    E.set_engine(R.RefitCorpusOracleEngine(use_port=True))
    return sga.Corpus(CORPUS, **kwargs)


def _lived(corpus):
    """append, remove, append: returns the list that is left (pandas alone)."""
    corpus.append(X1)
    left = pd.concat([CORPUS, X1])
    drop = [0, 2, len(CORPUS) - 1, len(CORPUS), len(left) - 1]
    corpus.remove(drop)
    keep = np.ones(len(left), bool)
    keep[drop] = False
    left = left[keep]
    corpus.append(X2)
    return pd.concat([left, X2])


# ------------------------------------------------------------------------------------------ Corpus on the double
@pytest.mark.parametrize("dtype", DTYPES)
def test_frames_of_all_four_methods_after_a_refit_equal_the_fixed_vocabulary_oracle(dtype):
    corpus = _corpus(tfidf_matrix_dtype=dtype)
    left = _lived(corpus)
    vocab0 = dict(corpus.vectorizer.vocabulary_)
    kw = dict(min_similarity=0.3)
    before = corpus.match_strings(corpus.master, NEW, **kw)
    _same(before, _expected(CORPUS, "match_strings", left, NEW, tfidf_matrix_dtype=dtype, **kw))
    corpus.refit_idf()
    master = corpus.master
    pd.testing.assert_series_equal(master, left)
    want = lambda method, *args, **k: R.expected_after_refit(CORPUS, left, method, *args, tfidf_matrix_dtype=dtype, **k)
    after = corpus.match_strings(master, NEW, **kw)
    _same(after, want("match_strings", left, NEW, **kw))
    assert not np.array_equal(after.similarity.to_numpy(), before.similarity.to_numpy()), "the refit changed no score"
    _same(corpus.match_strings(NEW, master, **kw), want("match_strings", NEW, left, **kw))
    _same(corpus.match_strings(master, **kw), want("match_strings", left, **kw))
    _same(corpus.match_most_similar(master, NEW, **kw), want("match_most_similar", left, NEW, **kw))
    _same(corpus.group_similar_strings(master, **kw), want("group_similar_strings", left, **kw))
    other = pd.Series(list(left)[::-1])
    _same(corpus.compute_pairwise_similarities(master, other), want("compute_pairwise_similarities", left, other))
    # the vocabulary is the original's, the idf the current list's
    assert corpus.vectorizer.vocabulary_ == vocab0
    _, _, idf = R.fixed_vocabulary_matrices(CORPUS, left, [], dtype=dtype)
    assert np.array_equal(_bits(corpus.vectorizer.idf_), _bits(idf))
    st = corpus.stats
    assert st["idf_refits"] == 1 and st["tokenisations"] == 1 and st["appends"] == 2 and st["removals"] == 1
    # the list lives on: a second append, remove and refit
    corpus.append(pd.Series(["Acme Corp Holdings", "Hooli Incorporated"], name="company"))
    corpus.remove([1, -2])
    left2 = pd.concat([left, pd.Series(["Acme Corp Holdings", "Hooli Incorporated"], name="company")])
    keep = np.ones(len(left2), bool)
    keep[[1, len(left2) - 2]] = False
    left2 = left2[keep]
    _same(corpus.match_strings(corpus.master, NEW, **kw),
          R.expected_after_refit(CORPUS, left, "match_strings", left2, NEW, tfidf_matrix_dtype=dtype, **kw))
    corpus.refit_idf()
    _same(corpus.match_strings(corpus.master, NEW, **kw),
          R.expected_after_refit(CORPUS, left2, "match_strings", left2, NEW, tfidf_matrix_dtype=dtype, **kw))
    assert corpus.stats["idf_refits"] == 2 and corpus.stats["tokenisations"] == 1


def test_a_refit_on_an_untouched_corpus_changes_nothing():
    corpus = _corpus()
    idf0, vocab0 = corpus.vectorizer.idf_.copy(), dict(corpus.vectorizer.vocabulary_)
    rows0 = corpus._engine.corpus_matrix(corpus._state).m.copy()
    before = corpus.match_strings(CORPUS, NEW, min_similarity=0.3)
    corpus.refit_idf()
    rows1 = corpus._engine.corpus_matrix(corpus._state).m
    assert corpus.vectorizer.vocabulary_ == vocab0 and np.array_equal(_bits(corpus.vectorizer.idf_), _bits(idf0))
    assert np.array_equal(rows1.indptr, rows0.indptr) and np.array_equal(rows1.indices, rows0.indices)
    assert np.array_equal(_bits(rows1.data), _bits(rows0.data))
    pd.testing.assert_frame_equal(corpus.match_strings(corpus.master, NEW, min_similarity=0.3), before)
    assert corpus.master is CORPUS and corpus.stats["idf_refits"] == 1


def test_a_kept_self_join_is_multiplied_anew_after_a_refit_and_served_right():
    corpus = _corpus()
    corpus.keep_self_join(min_similarity=0.3, max_n_matches=5)
    kw = dict(min_similarity=0.3, max_n_matches=5)
    corpus.group_similar_strings(corpus.master, **kw)
    left = _lived(corpus)
    _same(corpus.match_strings(corpus.master, **kw), _expected(CORPUS, "match_strings", left, **kw))
    st = corpus.stats
    assert st["self_join_full"] == 1 and st["self_join_served"] == 2 and st["self_join_append_updates"] == 2
    corpus.refit_idf()
    _same(corpus.match_strings(corpus.master, **kw), R.expected_after_refit(CORPUS, left, "match_strings", left, **kw))
    _same(corpus.group_similar_strings(corpus.master, **kw),
          R.expected_after_refit(CORPUS, left, "group_similar_strings", left, **kw))
    st = corpus.stats
    assert st["self_join_full"] == 2 and st["self_join_served"] == 4, st       # multiplied once more, its options kept
    # ... and follows the list again afterwards
    corpus.append(pd.Series(["Umbrella Corp Ltd"], name="company"))
    left = pd.concat([left, pd.Series(["Umbrella Corp Ltd"], name="company")])
    _same(corpus.match_strings(corpus.master, **kw), R.expected_after_refit(CORPUS, left[:-1], "match_strings", left, **kw))
    assert corpus.stats["self_join_full"] == 2 and corpus.stats["self_join_append_updates"] == 3


def test_refit_idf_on_a_closed_corpus_and_on_an_engine_without_it():
    corpus = _corpus()
    corpus.close()
    with pytest.raises(ValueError, match="the corpus is closed"):
        corpus.refit_idf()
    E.set_engine(RemoveCorpusOracleEngine(use_port=True))
    corpus = sga.Corpus(CORPUS)
    with pytest.raises(NotImplementedError, match="the engine 'oracle-corpus-remove' refits no idf"):
        corpus.refit_idf()
    corpus.match_strings(CORPUS, NEW)                    # nothing else is lost
    corpus = _corpus()
    E.set_engine(RemoveCorpusOracleEngine(use_port=True))
    with pytest.raises(RuntimeError, match="the engine has changed"):
        corpus.refit_idf()


# ------------------------------------------------------------------------------------------ the restatement
def _bite(dtype):
    """The corpus's rows before the refit as K2 leaves them (values and norms), the whole counts, and what sklearn gives."""
    original, appended, removed, live = R.bite_list()
    (_,), vocab, idf_old = O.tfidf_sklearn(original, [original], dtype=dtype)
    _, counts = O.count_matrix(live, vocab, dtype)
    counts = counts.tocsr()
    values, norms = R.k2_restated(counts, idf_old, dtype)
    held = counts.copy()
    held.data = values
    (want_old,), _, _ = O.tfidf_sklearn(original, [live], dtype=dtype)
    assert np.array_equal(want_old.indices, held.indices) and np.array_equal(_bits(want_old.data), _bits(held.data)), \
        "K2's restatement is not sklearn's transform"
    (want,), _, want_idf = R.fixed_vocabulary_matrices(original, live, [live], dtype=dtype)
    return held, norms, counts, idf_old, want, want_idf, vocab


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_list_holds_what_it_is_built_for(dtype):
    original, appended, removed, live = R.bite_list()
    held, norms, counts, idf_old, want, want_idf, vocab = _bite(dtype)
    lengths = set(np.diff(held.indptr).tolist())
    assert set(R.ROW_LENGTHS) <= lengths and max(lengths) > 128, sorted(lengths)
    assert counts.data.max() == 69_998 and 2_999 in counts.data
    assert any(len(set(counts.data[a:b].tolist())) > 1 for a, b in zip(counts.indptr[:-1], counts.indptr[1:]))
    empty = np.flatnonzero(np.diff(held.indptr) == 0)
    assert "!!??" in live and live.index("!!??") in empty and (norms[empty] == 0.0).all()
    df = np.bincount(held.indices, minlength=held.shape[1])
    assert df[vocab["qzx"]] == 0 and np.isfinite(want_idf[vocab["qzx"]])          # the column keeps its place
    assert len(removed) > 5 and len(live) == len(original) + len(appended) - len(removed)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_restated_reweigh_equals_sklearn_fitted_with_the_vocabulary_fixed(dtype):
    held, norms, counts, idf_old, want, want_idf, _ = _bite(dtype)
    idf_new = R.refit_idf_of(held, dtype)
    assert idf_new.dtype == dtype and np.array_equal(_bits(idf_new), _bits(want_idf))
    values, new_norms, tf, failed = R.reweigh_restated(held, norms, idf_old, idf_new)
    assert failed == 0
    assert np.array_equal(tf, counts.data.astype(np.int64)), "a count was not recovered"
    assert np.array_equal(want.indptr, held.indptr) and np.array_equal(want.indices, held.indices)
    assert np.array_equal(_bits(values), _bits(want.data))
    # the new norms are what K2 would leave on the whole counts under the new idf: a second refit starts from them
    v2, n2 = R.k2_restated(counts, idf_new, dtype)
    assert np.array_equal(_bits(v2), _bits(values)) and np.array_equal(_bits(n2), _bits(new_norms))
    # an identity refit changes no bit
    same, same_norms, _, failed = R.reweigh_restated(held, norms, idf_old, idf_old)
    assert failed == 0 and np.array_equal(_bits(same), _bits(held.data)) and np.array_equal(_bits(same_norms), _bits(norms))
    # rows made under ANOTHER idf than the one they are recovered with do not pass the verification
    _, _, _, failed = R.reweigh_restated(held, norms, idf_new, idf_new)
    assert failed > 0


# (the sum in the values' own type IS the sum in double for fp64; fp32 squares summed in double round the order away, the fp64
#  rows are the ones that depend on it)
@pytest.mark.parametrize("variant, dtype", [("tf_by_smallest_ratio", np.float32), ("tf_by_smallest_ratio", np.float64),
                                            ("sum_in_float", np.float32), ("sum_in_another_order", np.float64)])
def test_a_wrong_turn_of_the_arithmetic_changes_the_answer(variant, dtype):
    held, norms, counts, idf_old, want, _, _ = _bite(dtype)
    idf_new = R.refit_idf_of(held, dtype)
    values, _, tf, _ = R.reweigh_restated(held, norms, idf_old, idf_new, variant)
    assert not np.array_equal(_bits(values), _bits(want.data)), variant
    if variant == "tf_by_smallest_ratio":
        assert not np.array_equal(tf, counts.data.astype(np.int64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["df_over_removed_rows_too", "documents_of_the_original_list"])
def test_a_wrong_turn_of_the_counting_changes_the_answer(dtype, variant):
    original, appended, removed, live = R.bite_list()
    held, norms, counts, idf_old, want, want_idf, vocab = _bite(dtype)
    if variant == "df_over_removed_rows_too":
        _, everything = O.count_matrix(list(original) + list(appended), vocab, dtype)
        df, n_docs = np.bincount(everything.tocsr().indices, minlength=held.shape[1]), held.shape[0]
    else:
        df, n_docs = np.bincount(held.indices, minlength=held.shape[1]), len(original)
    idf = R.idf_from_df(df.astype(np.int64), n_docs, dtype)
    assert not np.array_equal(_bits(idf), _bits(want_idf))
    values, _, _, failed = R.reweigh_restated(held, norms, idf_old, idf)
    assert failed == 0 and not np.array_equal(_bits(values), _bits(want.data)), variant
