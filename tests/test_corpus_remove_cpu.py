"""CPU tests of Corpus.remove on the oracle engine double (tests/_corpus_remove_oracle.py): after removes (and appends in
between) every frame is what the oracle definition gives -- TfidfVectorizer(...).fit(ORIGINAL master), .transform(remaining
strings) as the corpus's rows -- the vocabulary and idf never change, and ``corpus.master`` is ``master[keep]``.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from tests._corpus_remove_oracle import RemoveCorpusOracleEngine
from tests.test_corpus_append_cpu import IDS_1, IDS_2, X1, X2
from tests.test_corpus_cpu import CORPUS, IDS_C, IDS_N, NEW, _expected


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


def _same(got, want):
    if isinstance(got, pd.DataFrame):
        pd.testing.assert_frame_equal(got, want)
    else:
        pd.testing.assert_series_equal(got, want)
    assert len(got) > 0


def _corpus(with_ids=False, master=CORPUS, **kwargs):
    E.set_engine(RemoveCorpusOracleEngine(use_port=True))
    return sga.Corpus(master, master_id=IDS_C if with_ids else None, **kwargs)


def _lived(with_ids):
    """append -> remove -> append -> remove: rows go from the original list, from a joined append and from a pending one.
    Returns the corpus and the list (and ids) that must be left, built with pandas alone."""
    corpus = _corpus(with_ids)
    want, want_ids = CORPUS, IDS_C
    corpus.append(X1, IDS_1 if with_ids else None)
    want, want_ids = pd.concat([want, X1]), pd.concat([want_ids, IDS_1])
    assert len(corpus.master) == len(want)               # (joined)
    drop = [2, len(CORPUS) + 1]                          # "Globex Inc" of the original list, "Stark Industries" of X1
    corpus.remove(drop)
    keep = np.ones(len(want), bool)
    keep[drop] = False
    want, want_ids = want[keep], want_ids[keep]
    corpus.append(X2, IDS_2 if with_ids else None)       # pending on the host: master is not asked for before the remove
    want, want_ids = pd.concat([want, X2]), pd.concat([want_ids, IDS_2])
    drop = [0, len(want) - 2]                            # "Acme Corporation", and "zzqqxx" of the pending X2
    assert want.iloc[drop[1]] == "zzqqxx"
    corpus.remove(np.array(drop))
    keep = np.ones(len(want), bool)
    keep[drop] = False
    return corpus, want[keep], want_ids[keep]


@pytest.mark.parametrize("with_ids", [False, True])
def test_frames_of_all_four_methods_after_appends_and_removes_equal_the_oracle(with_ids):
    corpus, left, left_ids = _lived(with_ids)
    master = corpus.master
    pd.testing.assert_series_equal(master, left)
    if with_ids:
        pd.testing.assert_series_equal(corpus.master_id, left_ids)
    else:
        assert corpus.master_id is None
    mid, nid = (corpus.master_id, IDS_N) if with_ids else (None, None)
    gid, gnid = (left_ids, IDS_N) if with_ids else (None, None)
    kw = dict(min_similarity=0.3)
    # the oracle fits on the ORIGINAL corpus and transforms what is left
    _same(corpus.match_strings(master, NEW, mid, nid, **kw), _expected(CORPUS, "match_strings", left, NEW, gid, gnid, **kw))
    _same(corpus.match_strings(NEW, master, nid, mid, **kw), _expected(CORPUS, "match_strings", NEW, left, gnid, gid, **kw))
    _same(corpus.match_strings(master, None, mid, **kw), _expected(CORPUS, "match_strings", left, None, gid, **kw))
    _same(corpus.match_most_similar(master, NEW, mid, nid, **kw),
          _expected(CORPUS, "match_most_similar", left, NEW, gid, gnid, **kw))
    _same(corpus.group_similar_strings(master, mid, **kw), _expected(CORPUS, "group_similar_strings", left, gid, **kw))
    other = pd.Series(list(left)[::-1])
    _same(corpus.compute_pairwise_similarities(master, other), _expected(CORPUS, "compute_pairwise_similarities", left, other))
    # a removed row is not found any more, its neighbour is: "Globex Inc" went, "Globex Incorporated" stayed
    frame = corpus.match_strings(master, NEW, mid, nid, min_similarity=0.3)
    assert "Globex Inc" not in set(frame.left_company) and "Globex Incorporated" in set(frame.left_company)
    st = corpus.stats
    assert st["removals"] == 2 and st["rows_removed"] == 4 and st["appends"] == 2 and st["tokenisations"] == 1
    assert st["dead_rows"] == 0                           # (the double keeps no tombstones)


def test_vocabulary_and_idf_stay_bit_identical_even_when_an_ngram_loses_its_only_row():
    corpus = _corpus()
    vocab0, idf0 = dict(corpus.vectorizer.vocabulary_), corpus.vectorizer.idf_.copy()
    row = list(CORPUS).index("Vehement Capital")         # nobody else has "veh"
    assert sum("veh" in s.lower() for s in CORPUS) == 1 and "veh" in vocab0
    corpus.remove(row)
    corpus.append(pd.Series(["Brand New Name"], name="company"))
    corpus.remove([0, -1])
    corpus.compact()
    assert corpus.vectorizer.vocabulary_ == vocab0
    assert np.array_equal(corpus.vectorizer.idf_.view(np.uint64), idf0.view(np.uint64))
    left = CORPUS.drop(index=[row])[1:]
    pd.testing.assert_series_equal(corpus.master, left)
    kw = dict(min_similarity=0.2)
    _same(corpus.match_strings(corpus.master, NEW, **kw), _expected(CORPUS, "match_strings", left, NEW, **kw))
    # the refit is a different thing: its idf counts the remaining documents
    E.set_engine(RemoveCorpusOracleEngine(use_port=True))
    refit = sga.Corpus(left)
    assert "veh" not in refit.vectorizer.vocabulary_


@pytest.mark.parametrize("labels", ["range", "integers", "strings", "duplicates", "named", "string_dtype"])
@pytest.mark.parametrize("how", ["int", "list", "negative", "mask", "array", "series_mask"])
def test_master_is_master_keep_whatever_the_labels_and_the_argument(labels, how):
    n = len(CORPUS)
    index = {"range": None, "integers": [7 * i + 3 for i in range(n)], "strings": [f"r{i}" for i in range(n)],
             "duplicates": [i // 2 for i in range(n)], "named": pd.Index(range(100, 100 + n), name="key"),
             "string_dtype": None}[labels]
    master = pd.Series(list(CORPUS), index=index, name="company", dtype="string" if labels == "string_dtype" else object)
    ids = pd.Series(np.arange(n) * 10, index=index, name="cid")            # an int64 id column: joined by pandas
    E.set_engine(RemoveCorpusOracleEngine(use_port=True))
    corpus = sga.Corpus(master, master_id=ids)
    keep = np.ones(n, bool)
    if how == "int":
        rows = 3
        keep[3] = False
    elif how == "list":
        rows = [5, 1, 5, 9]                              # out of order, one position twice
        keep[[1, 5, 9]] = False
    elif how == "negative":
        rows = [-1, 0, -n + 2, n - 1]                    # the last row twice under two names
        keep[[0, 2, n - 1]] = False
    elif how == "array":
        rows = np.array([4, 6], dtype=np.uint8)
        keep[[4, 6]] = False
    else:
        keep[[2, 3, 10]] = False
        rows = ~keep if how == "mask" else pd.Series(~keep)
    before = corpus.master
    corpus.remove(rows)
    got = corpus.master
    assert got is not before
    pd.testing.assert_series_equal(got, master[keep])
    assert got.index.name == master.index.name and got.name == "company"
    pd.testing.assert_series_equal(corpus.master_id, ids[keep])
    assert corpus.stats["rows_removed"] == int((~keep).sum()) and corpus.stats["removals"] == 1
    kw = dict(min_similarity=0.3)
    _same(corpus.match_strings(got, NEW, corpus.master_id, IDS_N, **kw),
          _expected(CORPUS, "match_strings", master[keep], NEW, ids[keep], IDS_N, **kw))


def test_a_master_taken_before_a_remove_still_reads_its_old_values():
    """The Series a corpus hands out are views of buffers that grow at the end: a remove must not move rows inside them."""
    corpus = _corpus(with_ids=True)
    corpus.append(X1, IDS_1)
    old, old_ids = corpus.master, corpus.master_id       # views of the growing buffers
    snapshot, snapshot_ids = old.copy(deep=True), old_ids.copy(deep=True)
    corpus.remove([1, 4, len(CORPUS)])
    middle = corpus.master
    middle_snapshot = middle.copy(deep=True)
    corpus.append(X2, IDS_2)                             # written behind the NEW buffers' rows
    corpus.remove(0)
    corpus.append(pd.Series(["Soylent Corp"]), pd.Series(["s0"]))
    now = corpus.master
    pd.testing.assert_series_equal(old, snapshot)
    pd.testing.assert_series_equal(old_ids, snapshot_ids)
    pd.testing.assert_series_equal(middle, middle_snapshot)
    keep = np.ones(len(snapshot), bool)
    keep[[1, 4, len(CORPUS)]] = False
    pd.testing.assert_series_equal(now, pd.concat([snapshot[keep], X2])[1:].pipe(lambda s: pd.concat([s, pd.Series(["Soylent Corp"])])))
    # an old object in a call is a Series like any other: transformed, same result as the list it holds
    before = corpus.stats["transforms"]
    kw = dict(min_similarity=0.3)
    _same(corpus.match_strings(old, NEW, **kw), _expected(CORPUS, "match_strings", snapshot, NEW, **kw))
    assert corpus.stats["transforms"] == before + 2
    _same(corpus.match_strings(now, NEW, **kw), _expected(CORPUS, "match_strings", now.copy(), NEW, **kw))
    assert corpus.stats["transforms"] == before + 3      # the current object stands for the resident rows


def test_remove_validates_its_input_and_the_no_op_cases_change_nothing():
    corpus = _corpus(with_ids=True)
    n = len(CORPUS)
    for bad in (1.5, "3", [1.0, 2.0], ["a"], None, True, np.array([[1, 2]]), [1, None]):
        with pytest.raises(TypeError):
            corpus.remove(bad)
    for bad in (np.ones(n - 1, bool), [True, False], n, -n - 1, [0, n], np.array([-n - 1, 2])):
        with pytest.raises(IndexError):
            corpus.remove(bad)
    with pytest.raises(ValueError, match="every row"):
        corpus.remove(np.ones(n, bool))
    with pytest.raises(ValueError, match="every row"):
        corpus.remove(list(range(n)) + [-1])
    stats, master, ids = corpus.stats, corpus.master, corpus.master_id
    for nothing in ([], np.zeros(n, bool), np.zeros(0, np.int64), ()):
        corpus.remove(nothing)
    assert corpus.stats == stats and corpus.master is master and corpus.master_id is ids
    pd.testing.assert_series_equal(master, CORPUS)
    corpus.remove(-n)                                    # the lowest position by its negative name
    pd.testing.assert_series_equal(corpus.master, CORPUS[1:])
    corpus.close()
    with pytest.raises(ValueError, match="closed"):
        corpus.remove(0)
    other = _corpus()
    E.set_engine(RemoveCorpusOracleEngine())
    with pytest.raises(RuntimeError, match="engine has changed"):
        other.remove(0)


def test_an_engine_that_removes_nothing_says_so():
    from tests._corpus_append_oracle import AppendCorpusOracleEngine
    E.set_engine(AppendCorpusOracleEngine(use_port=True))
    corpus = sga.Corpus(CORPUS)
    with pytest.raises(NotImplementedError, match="removes no rows"):
        corpus.remove(0)


def test_the_engine_s_bookkeeping_of_dead_rows_maps_live_to_physical_rows():
    """CorpusState.physical_rows (no device needed): live position -> position in the segments, dead rows skipped."""
    state = E.CorpusState.__new__(E.CorpusState)
    state.dead = np.array([0, 1, 5, 9], dtype=np.int64)              # of 12 physical rows
    live = np.array([r for r in range(12) if r not in (0, 1, 5, 9)])
    assert np.array_equal(state.physical_rows(np.arange(8)), live)
    state.dead = np.zeros(0, np.int64)
    assert np.array_equal(state.physical_rows(np.array([0, 3, 7])), [0, 3, 7])
