"""CPU tests of string_grouper_amd.Corpus on the oracle engine double (tests/_corpus_oracle.py): the fixed-corpus
semantics -- vocabulary and idf of TfidfVectorizer(...).fit(corpus), every Series .transform()ed with them -- and the
mirror's frames on top.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from string_grouper_amd.string_grouper import StringGrouper
from tests._corpus_oracle import CorpusOracleEngine, fixed_corpus_matrices
from tests._oracle_engine import HostMatrix, OracleEngine

CORPUS = pd.Series(["Acme Corporation", "Acme Corp", "Globex Inc", "Globex Incorporated", "Initech LLC", "Initech",
                    "Umbrella Corp", "Umbrella Corporation", "Hooli", "Hooli Inc", "Vehement Capital", "Massive Dynamic"],
                   name="company")
NEW = pd.Series(["ACME Corp.", "Globex", "Initech L.L.C.", "Stark Industries", "Umbrella Corp", "hooli inc",
                 "Wayne Enterprises"], name="incoming")


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


class _FixedGrouper(StringGrouper):
    """The oracle definition of a call: the mirror's fit() and frames over sklearn's fit(corpus) + transform matrices."""

    def __init__(self, corpus, *args, **kwargs):
        self._fit_on = corpus
        super().__init__(*args, **kwargs)

    def _tfidf_on_engine(self):
        cfg = self._config
        kw = dict(ngram_size=cfg.ngram_size, regex=cfg.regex, ignore_case=cfg.ignore_case,
                  normalize_to_ascii=cfg.normalize_to_ascii)
        sets = [self._master] + ([] if self._duplicates is None else [self._duplicates])
        mats, _, _ = fixed_corpus_matrices(self._fit_on, sets, dtype=cfg.tfidf_matrix_dtype, **kw)
        A = HostMatrix(mats[0])
        return A, (A if self._duplicates is None else HostMatrix(mats[1]))


def _expected(corpus, method, *args, **kwargs):
    before = E._engine
    E.set_engine(OracleEngine(use_port=True))
    try:
        if method == "match_strings":
            master, dupes, mid, did = (list(args) + [None] * 4)[:4]
            return _FixedGrouper(corpus, master, dupes, mid, did, **kwargs).fit().get_matches()
        if method == "match_most_similar":
            master, dupes, mid, did = (list(args) + [None] * 4)[:4]
            kwargs["max_n_matches"] = 1
            return _FixedGrouper(corpus, master, dupes, mid, did, **kwargs).fit().get_groups()
        if method == "group_similar_strings":
            strings, ids = (list(args) + [None] * 2)[:2]
            return _FixedGrouper(corpus, strings, master_id=ids, **kwargs).fit().get_groups()
        s1, s2 = args
        return _FixedGrouper(corpus, s1, s2, **kwargs).dot()
    finally:
        E.set_engine(before)


def _corpus(**kwargs):
    E.set_engine(CorpusOracleEngine(use_port=True))
    return sga.Corpus(CORPUS, **kwargs)


IDS_C = pd.Series([f"c{i}" for i in range(len(CORPUS))], name="cid")
IDS_N = pd.Series([f"n{i}" for i in range(len(NEW))], name="nid")


@pytest.mark.parametrize("case", ["self_join", "corpus_x_new", "new_x_corpus", "new_self_join", "ids", "ignore_index",
                                  "low_threshold", "fp32"])
def test_match_strings_frames_equal_the_oracle(case):
    args, kw = {
        "self_join": ((CORPUS,), dict(min_similarity=0.5)),
        "corpus_x_new": ((CORPUS, NEW), dict(min_similarity=0.3)),
        "new_x_corpus": ((NEW, CORPUS), dict(min_similarity=0.3)),
        "new_self_join": ((NEW,), dict(min_similarity=0.1)),
        "ids": ((CORPUS, NEW, IDS_C, IDS_N), dict(min_similarity=0.3)),
        "ignore_index": ((CORPUS, NEW), dict(min_similarity=0.3, ignore_index=True)),
        "low_threshold": ((CORPUS, NEW), dict(min_similarity=0.05, max_n_matches=2)),
        "fp32": ((CORPUS, NEW), dict(min_similarity=0.3)),
    }[case]
    ckw = dict(tfidf_matrix_dtype=np.float32) if case == "fp32" else {}
    corpus = _corpus(**ckw)
    got = corpus.match_strings(*args, **kw)
    want = _expected(CORPUS, "match_strings", *args, **kw, **ckw)
    pd.testing.assert_frame_equal(got, want)
    assert len(got) > 0


def test_match_most_similar_group_similar_and_pairwise_equal_the_oracle():
    corpus = _corpus()
    for args, kw in [((CORPUS, NEW), dict(min_similarity=0.3)), ((CORPUS, NEW, IDS_C, IDS_N), dict(min_similarity=0.3)),
                     ((CORPUS, NEW), dict(min_similarity=0.3, ignore_index=True))]:
        got = corpus.match_most_similar(*args, **kw)
        want = _expected(CORPUS, "match_most_similar", *args, **kw)
        pd.testing.assert_frame_equal(got, want) if isinstance(got, pd.DataFrame) else pd.testing.assert_series_equal(got, want)
    for args, kw in [((NEW,), dict(min_similarity=0.2)), ((CORPUS, IDS_C), dict(min_similarity=0.5, group_rep="first"))]:
        got = corpus.group_similar_strings(*args, **kw)
        want = _expected(CORPUS, "group_similar_strings", *args, **kw)
        pd.testing.assert_frame_equal(got, want) if isinstance(got, pd.DataFrame) else pd.testing.assert_series_equal(got, want)
    s1 = CORPUS[:len(NEW)].reset_index(drop=True)
    got = corpus.compute_pairwise_similarities(s1, NEW)
    pd.testing.assert_series_equal(got, _expected(CORPUS, "compute_pairwise_similarities", s1, NEW))


def test_the_corpus_does_not_refit_on_the_new_strings():
    # the new strings repeat one trigram-rich word many times: a refit on corpus + new would lower its idf
    new = pd.Series(["Acme Corp"] * 20 + ["Acme Corporation"] * 20)
    corpus = _corpus()
    fixed = corpus.match_strings(CORPUS, new, min_similarity=0.3)
    E.set_engine(OracleEngine(use_port=True))
    refit = sga.match_strings(CORPUS, new, min_similarity=0.3)
    E.set_engine(corpus._engine)
    assert list(fixed.columns) == list(refit.columns)
    assert not np.array_equal(fixed.similarity.to_numpy(), refit.similarity.to_numpy())
    pd.testing.assert_frame_equal(fixed, _expected(CORPUS, "match_strings", CORPUS, new, min_similarity=0.3))


def test_ten_calls_leave_vocabulary_and_idf_bit_identical():
    corpus = _corpus()
    vocab0, idf0 = dict(corpus.vectorizer.vocabulary_), corpus.vectorizer.idf_.copy()
    for i in range(10):
        corpus.match_strings(CORPUS, pd.Series([f"Brand New Name {i}", "Acme Corp"]), min_similarity=0.2)
        corpus.group_similar_strings(NEW)
    assert corpus.vectorizer.vocabulary_ == vocab0
    assert np.array_equal(corpus.vectorizer.idf_.view(np.uint64), idf0.view(np.uint64))
    st = corpus.stats
    assert st["tokenisations"] == 1 and st["transforms"] == 20


def test_the_corpus_index_is_built_once():
    corpus = _corpus()
    for _ in range(5):
        corpus.match_strings(NEW, CORPUS, min_similarity=0.3)
    assert corpus.stats["index_builds"] == 1 and corpus.stats["resident_index"] == 5


@pytest.mark.parametrize("name,value", [("ngram_size", 2), ("regex", r"\s"), ("ignore_case", False),
                                        ("normalize_to_ascii", False), ("tfidf_matrix_dtype", np.float32)])
def test_vectoriser_options_that_differ_raise(name, value):
    corpus = _corpus()
    with pytest.raises(ValueError, match=name):
        corpus.match_strings(CORPUS, NEW, **{name: value})
    corpus.match_strings(CORPUS, NEW, **{name: getattr(corpus._config, name)})       # the same value is accepted


def test_per_call_options_and_unknown_options():
    corpus = _corpus(min_similarity=0.9)
    assert len(corpus.match_strings(CORPUS, NEW)) < len(corpus.match_strings(CORPUS, NEW, min_similarity=0.2))
    with pytest.raises(TypeError):
        corpus.match_strings(CORPUS, NEW, no_such_option=1)


def test_strings_of_unseen_ngrams_are_empty_rows_and_still_match_themselves():
    unseen = pd.Series(["zzqqxx", "qqzzxxjj", "Acme Corp"])
    corpus = _corpus()
    (m,), _, _ = fixed_corpus_matrices(CORPUS, [unseen])
    assert m[0].nnz == 0 and m[1].nnz == 0
    got = corpus.match_strings(unseen, min_similarity=0.5)
    pd.testing.assert_frame_equal(got, _expected(CORPUS, "match_strings", unseen, min_similarity=0.5))
    self_rows = got[got.left_index == got.right_index]
    assert sorted(self_rows.left_index) == [0, 1, 2] and (self_rows.similarity == 1.0).all()
    vs = corpus.match_strings(CORPUS, unseen, min_similarity=0.1)
    assert set(vs.right_index) == {2}


def test_closed_corpus_and_distributed_engine_refuse():
    corpus = _corpus()
    with corpus as c:
        c.match_strings(NEW, min_similarity=0.5)
    with pytest.raises(ValueError, match="closed"):
        corpus.match_strings(NEW)
    E.set_engine(E.DistributedHipEngine(ctx=None, group=None))
    with pytest.raises(NotImplementedError, match="single-GPU"):
        sga.Corpus(CORPUS)
    other = _corpus()
    E.set_engine(OracleEngine())
    with pytest.raises(RuntimeError, match="engine has changed"):
        other.match_strings(NEW)



def test_the_alias_package_keeps_the_reference_surface():
    import string_grouper
    assert not hasattr(string_grouper, "Corpus")
