"""CPU tests of Corpus.append on the oracle engine double (tests/_corpus_append_oracle.py): after appends every frame is
what the oracle definition gives -- TfidfVectorizer(...).fit(original master), .transform(original + appended strings) as
the corpus's rows -- and the vocabulary and idf never change.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from tests._corpus_append_oracle import AppendCorpusOracleEngine
from tests._corpus_oracle import fixed_corpus_matrices
from tests.test_corpus_cpu import CORPUS, IDS_C, IDS_N, NEW, _expected

X1 = pd.Series(["Acme Corp Ltd", "Stark Industries", "Hooli"], index=[100, 101, 102], name="company")
X2 = pd.Series(["Globex", "Wayne Enterprises Inc", "zzqqxx", "Initech LLC"], index=[7, 8, 9, 10], name="company")
IDS_1 = pd.Series([f"x{i}" for i in range(len(X1))], index=X1.index, name="cid")
IDS_2 = pd.Series([f"y{i}" for i in range(len(X2))], index=X2.index, name="cid")
GROWN = pd.concat([CORPUS, X1, X2])
GROWN_IDS = pd.concat([IDS_C, IDS_1, IDS_2])


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


def _grown(with_ids=False, **kwargs):
    E.set_engine(AppendCorpusOracleEngine(use_port=True))
    corpus = sga.Corpus(CORPUS, master_id=IDS_C if with_ids else None, **kwargs)
    corpus.append(X1, IDS_1 if with_ids else None)
    corpus.append(X2, IDS_2 if with_ids else None)
    return corpus


def _same(got, want):
    if isinstance(got, pd.DataFrame):
        pd.testing.assert_frame_equal(got, want)
    else:
        pd.testing.assert_series_equal(got, want)
    assert len(got) > 0


@pytest.mark.parametrize("with_ids", [False, True])
def test_frames_of_all_four_methods_after_two_appends_equal_the_oracle(with_ids):
    corpus = _grown(with_ids)
    master = corpus.master
    pd.testing.assert_series_equal(master, GROWN)
    if with_ids:
        pd.testing.assert_series_equal(corpus.master_id, GROWN_IDS)
    else:
        assert corpus.master_id is None
    mid, nid = (corpus.master_id, IDS_N) if with_ids else (None, None)
    gid, gnid = (GROWN_IDS, IDS_N) if with_ids else (None, None)
    kw = dict(min_similarity=0.3)
    # the oracle fits on the ORIGINAL corpus and transforms the concatenation
    _same(corpus.match_strings(master, NEW, mid, nid, **kw), _expected(CORPUS, "match_strings", GROWN, NEW, gid, gnid, **kw))
    _same(corpus.match_strings(NEW, master, nid, mid, **kw), _expected(CORPUS, "match_strings", NEW, GROWN, gnid, gid, **kw))
    _same(corpus.match_strings(master, None, mid, **kw), _expected(CORPUS, "match_strings", GROWN, None, gid, **kw))
    _same(corpus.match_most_similar(master, NEW, mid, nid, **kw),
          _expected(CORPUS, "match_most_similar", GROWN, NEW, gid, gnid, **kw))
    _same(corpus.group_similar_strings(master, mid, **kw), _expected(CORPUS, "group_similar_strings", GROWN, gid, **kw))
    other = pd.Series(list(GROWN)[::-1])
    _same(corpus.compute_pairwise_similarities(master, other),
          _expected(CORPUS, "compute_pairwise_similarities", GROWN, other))
    # an appended row is found like any other: "Globex" (appended second) by the batch's copy of it
    frame = corpus.match_strings(master, NEW, mid, nid, min_similarity=0.99)
    assert "Globex" in set(frame.left_company)


def test_the_idf_is_the_original_corpus_s_not_a_refit():
    corpus = _grown()
    fixed = corpus.match_strings(corpus.master, NEW, min_similarity=0.3)
    E.set_engine(AppendCorpusOracleEngine(use_port=True))
    refit = sga.Corpus(GROWN).match_strings(GROWN, NEW, min_similarity=0.3)
    assert not (len(fixed) == len(refit) and np.array_equal(fixed.similarity.to_numpy(), refit.similarity.to_numpy()))


def test_ten_appends_leave_vocabulary_and_idf_bit_identical_and_count():
    E.set_engine(AppendCorpusOracleEngine(use_port=True))
    corpus = sga.Corpus(CORPUS)
    vocab0, idf0 = dict(corpus.vectorizer.vocabulary_), corpus.vectorizer.idf_.copy()
    rows = 0
    for i in range(10):
        batch = pd.Series([f"Brand New Name {i}", "Acme Corp", "Qwertz Übung"][: 1 + i % 3])
        corpus.append(batch)
        rows += len(batch)
        corpus.match_strings(corpus.master, NEW, min_similarity=0.2)
    assert corpus.vectorizer.vocabulary_ == vocab0
    assert np.array_equal(corpus.vectorizer.idf_.view(np.uint64), idf0.view(np.uint64))
    st = corpus.stats
    assert st["tokenisations"] == 1 and st["appends"] == 10 and st["rows_appended"] == rows
    assert len(corpus.master) == len(CORPUS) + rows
    corpus.compact()
    assert corpus.stats["compactions"] == 1
    _same(corpus.match_strings(corpus.master, NEW, min_similarity=0.2),
          _expected(CORPUS, "match_strings", corpus.master, NEW, min_similarity=0.2))


def test_an_appended_string_of_unseen_ngrams_is_an_empty_row_that_matches_itself():
    corpus = _grown()
    (m,), _, _ = fixed_corpus_matrices(CORPUS, [GROWN])
    row = len(CORPUS) + len(X1) + 2                      # "zzqqxx"
    assert GROWN.iloc[row] == "zzqqxx" and m[row].nnz == 0
    got = corpus.match_strings(corpus.master, min_similarity=0.5)
    _same(got, _expected(CORPUS, "match_strings", GROWN, min_similarity=0.5))
    label = GROWN.index[row]
    own = got[(got.left_index == label) & (got.right_index == label) & (got.left_company == "zzqqxx")]
    assert len(own) == 1 and own.similarity.iloc[0] == 1.0


def test_append_validates_its_input():
    E.set_engine(AppendCorpusOracleEngine(use_port=True))
    plain, with_ids = sga.Corpus(CORPUS), sga.Corpus(CORPUS, master_id=IDS_C)
    with pytest.raises(ValueError, match="new_ids"):
        plain.append(X1, IDS_1)                          # superfluous
    with pytest.raises(ValueError, match="new_ids"):
        with_ids.append(X1)                              # missing
    with pytest.raises(Exception, match="same length"):
        with_ids.append(X1, IDS_2)
    for bad in (pd.Series([1, 2, 3]), pd.Series(["a", None]), ["Acme"], pd.Series(["a", 2.5])):
        with pytest.raises(TypeError):
            plain.append(bad)
    for c in (plain, with_ids):
        assert c.stats["appends"] == 0 and len(c.master) == len(CORPUS)
    before = plain.master
    plain.append(pd.Series([], dtype=object))            # an empty Series: nothing happens
    assert plain.master is before and plain.stats["appends"] == 0
    plain.close()
    with pytest.raises(ValueError, match="closed"):
        plain.append(X1)
    with pytest.raises(ValueError, match="closed"):
        plain.compact()
    E.set_engine(AppendCorpusOracleEngine())
    with pytest.raises(RuntimeError, match="engine has changed"):
        with_ids.append(X1, IDS_1)


def test_an_old_master_object_after_an_append_is_transformed_like_any_series():
    E.set_engine(AppendCorpusOracleEngine(use_port=True))
    corpus = sga.Corpus(CORPUS)
    corpus.append(X1)
    old = corpus.master
    corpus.append(X2)
    assert corpus.master is not old
    before = corpus.stats["transforms"]
    kw = dict(min_similarity=0.3)
    _same(corpus.match_strings(old, NEW, **kw), _expected(CORPUS, "match_strings", old, NEW, **kw))
    _same(corpus.match_strings(CORPUS, NEW, **kw), _expected(CORPUS, "match_strings", CORPUS, NEW, **kw))
    assert corpus.stats["transforms"] == before + 4      # neither is the corpus's current Series: both sides transformed
    _same(corpus.match_strings(corpus.master, NEW, **kw), _expected(CORPUS, "match_strings", GROWN, NEW, **kw))
    assert corpus.stats["transforms"] == before + 5


@pytest.mark.parametrize("labels", ["range", "integers", "strings", "named", "string_dtype"])
def test_master_is_the_concatenation_of_the_parts_whatever_their_labels(labels):
    def series(values, start):
        index = {"range": None, "integers": [start * 3 + 7 * i for i in range(len(values))],
                 "strings": [f"r{start}_{i}" for i in range(len(values))],
                 "named": pd.Index(range(start, start + len(values)), name="key"),
                 "string_dtype": None}[labels]
        return pd.Series(values, index=index, name="company", dtype="string" if labels == "string_dtype" else object)
    E.set_engine(AppendCorpusOracleEngine(use_port=True))
    parts = [series(list(CORPUS), 0), series(list(X1), 100), series(list(X2), 200), series(["Hooli Inc"], 300)]
    corpus = sga.Corpus(parts[0], master_id=IDS_C)
    seen = []
    for k, (part, ids) in enumerate(zip(parts[1:], (IDS_1, IDS_2, pd.Series(["z0"], name="other")))):
        corpus.append(part, ids)
        if k != 1:                               # (two appends between two looks at the Series: joined in one go)
            seen.append((corpus.master, pd.concat(parts[:k + 2])))
    seen.append((corpus.master_id, pd.concat([IDS_C, IDS_1, IDS_2, pd.Series(["z0"], name="other")])))
    for got, want in seen:                       # the earlier objects are still what they were
        pd.testing.assert_series_equal(got, want)
        assert got.index.name == want.index.name
    kw = dict(min_similarity=0.3)
    _same(corpus.match_strings(corpus.master, NEW, corpus.master_id, IDS_N, **kw),
          _expected(CORPUS, "match_strings", seen[-2][1], NEW, seen[-1][1], IDS_N, **kw))
