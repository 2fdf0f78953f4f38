"""CPU tests of record matching on the engine double of tests/_record_oracle.py: every argument check of
``Corpus.match_records`` / ``group_similar_records`` / ``string_grouper_amd.match_records``, the frame against the composed route
(match_strings at the candidate options, pair_similarities a further corpus, the numpy chain, the filter, the order and the cut
in pandas), the counters, and the reference's surface.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import string_grouper
import string_grouper_amd as sga
import string_grouper_amd.engine as E
from tests._pair_oracle import PairCorpusOracleEngine
from tests._record_oracle import RecordOracleEngine, composed_groups, composed_route
from tests.test_corpus_cpu import CORPUS, NEW

DTYPES = [np.float32, np.float64]
ADDRESS = pd.Series([f"{i % 4} Main Street {'North' if i % 2 else 'Nrth'}" for i in range(len(CORPUS))], name="address")
CITY = pd.Series(["Springfield", "Springfeld", "Shelbyville", "Shelbyvile"] * 3, name="city")
NEW_ADDRESS = pd.Series([f"{i % 3} Main Street North" for i in range(len(NEW))], name="address")
NEW_CITY = pd.Series(["Springfield", "Shelbyville", "Springfeld", "Gotham", "Shelbyvile", "Springfield", "Gotham"], name="city")
W = [0.5, 0.25, 0.25]
CAND = dict(min_similarity=0.1, max_n_matches=8)


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


def _corpora(**kwargs):
    eng = RecordOracleEngine(use_port=True)
    E.set_engine(eng)
    return sga.Corpus(CORPUS, **kwargs), sga.Corpus(ADDRESS, **kwargs), sga.Corpus(CITY, **kwargs), eng


# ------------------------------------------------------------------------------------------ the frame
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_frame_is_the_composed_route_s(dtype):
    names, addresses, cities, eng = _corpora(tfidf_matrix_dtype=dtype)
    for thr, top_n in ((0.3, 3), (0.45, 1), (0.15, 20)):
        got = names.match_records([addresses, cities], weights=W, candidates=CAND, min_similarity=thr, max_n_matches=top_n,
                                  force_symmetries=False)
        want = composed_route(names, [addresses, cities], W, CAND, thr, top_n)
        pd.testing.assert_frame_equal(got, want)
        assert 0 < len(got) <= len(names.match_strings(names.master, force_symmetries=False, **CAND)) and (thr < 0.3 or len(got) < 38)
    dupes = [NEW, NEW_ADDRESS, NEW_CITY]
    got = names.match_records([addresses, cities], duplicates=dupes, weights=W, candidates=CAND, min_similarity=0.3, max_n_matches=2)
    want = composed_route(names, [addresses, cities], W, CAND, 0.3, 2, duplicates=dupes)
    pd.testing.assert_frame_equal(got, want)
    assert len(got) > 3 and list(got.columns) == list(names.match_strings(names.master, NEW).columns)
    one = names.match_records([cities], weights=[0.75, 0.25], candidates=CAND, min_similarity=0.3, force_symmetries=False)
    pd.testing.assert_frame_equal(one, composed_route(names, [cities], [0.75, 0.25], CAND, 0.3, 20))
    assert eng.record_calls == [(12, 2)] * 4 + [(12, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_defaults_equal_shares_self_matches_and_symmetry(dtype):
    names, addresses, cities, _ = _corpora(tfidf_matrix_dtype=dtype, min_similarity=0.3)
    got = names.match_records([addresses, cities])
    third = [1 / 3] * 3
    own = dict(min_similarity=0.3, max_n_matches=20)                                # the corpus's own options find the candidates
    unsym = composed_route(names, [addresses, cities], third, own, 0.3, 20)
    diag = got[got.left_index == got.right_index]
    assert len(diag) == len(CORPUS) and (diag.similarity == 1.0).all()              # a record always matches itself with 1
    pairs = set(zip(got.left_index, got.right_index))
    assert pairs == {(b, a) for a, b in pairs} and pairs >= set(zip(unsym.left_index, unsym.right_index))
    off = got[got.left_index != got.right_index].set_index(["left_index", "right_index"]).similarity
    for (a, b), s in unsym[unsym.left_index != unsym.right_index].set_index(["left_index", "right_index"]).similarity.items():
        assert off[(a, b)] == s
    groups = names.group_similar_records([addresses, cities], weights=W, candidates=CAND, min_similarity=0.3)
    pd.testing.assert_frame_equal(groups, composed_groups(names, [addresses, cities], W, CAND, 0.3, 20))
    ids = pd.Series([f"id{i}" for i in range(len(CORPUS))], name="id")
    with_ids = sga.Corpus(CORPUS, master_id=ids, tfidf_matrix_dtype=dtype)
    got = with_ids.match_records([addresses, cities], weights=W, candidates=CAND, min_similarity=0.3, force_symmetries=False)
    pd.testing.assert_frame_equal(got, composed_route(with_ids, [addresses, cities], W, CAND, 0.3, 20))
    assert "left_id" in got.columns
    assert list(with_ids.group_similar_records([addresses, cities]).columns) == list(with_ids.group_similar_strings(CORPUS, ids).columns)


def test_the_module_level_function_builds_calls_and_closes():
    eng = RecordOracleEngine(use_port=True)
    E.set_engine(eng)
    got = sga.match_records([CORPUS, ADDRESS, CITY], weights=W, candidates=CAND, min_similarity=0.3, max_n_matches=3,
                            force_symmetries=False)
    names, addresses, cities, _ = _corpora()
    pd.testing.assert_frame_equal(got, composed_route(names, [addresses, cities], W, CAND, 0.3, 3))
    got = sga.match_records([CORPUS, ADDRESS, CITY], duplicates=[NEW, NEW_ADDRESS, NEW_CITY], weights=W, candidates=CAND, min_similarity=0.3)
    pd.testing.assert_frame_equal(got, composed_route(names, [addresses, cities], W, CAND, 0.3, 20, duplicates=[NEW, NEW_ADDRESS, NEW_CITY]))
    with pytest.raises(TypeError):
        sga.match_records(CORPUS)
    with pytest.raises(TypeError):
        sga.match_records([CORPUS])
    with pytest.raises(ValueError, match="differ in length"):
        sga.match_records([CORPUS, ADDRESS[:-1]])


# ------------------------------------------------------------------------------------------ counters
def test_record_calls_move_and_nothing_is_tokenised_or_compacted():
    names, addresses, cities, _ = _corpora()
    corpora = (names, addresses, cities)
    before = [c.stats for c in corpora]
    names.match_records([addresses, cities], weights=W, candidates=CAND, min_similarity=0.3)
    names.group_similar_records([addresses, cities])
    addresses.match_records([names], min_similarity=0.3)
    for c, b, calls in zip(corpora, before, (3, 3, 2)):
        st = c.stats
        assert st["record_calls"] == b["record_calls"] + calls
        assert st["compactions"] == b["compactions"] and st["tokenisations"] == b["tokenisations"] == 1
        assert st["pair_calls"] == 0 and st["transforms"] == 0
    names.match_records([addresses, cities], duplicates=[NEW, NEW_ADDRESS, NEW_CITY])
    assert [c.stats["transforms"] for c in corpora] == [1, 1, 1]                     # one transform a field


# ------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    names, addresses, cities, eng = _corpora()
    both = [addresses, cities]
    for bad in (addresses, [], [addresses, "x"], None, [CITY]):
        with pytest.raises((TypeError, ValueError)):
            names.match_records(bad)
    with pytest.raises(TypeError):
        names.match_records(addresses)                                               # a corpus, not a list of them
    with pytest.raises(ValueError, match="between 1 and 7"):
        names.match_records([])
    with pytest.raises(ValueError, match="between 1 and 7"):
        names.match_records([addresses] * 8)
    names.match_records([addresses] * 7)                                             # seven further fields are served
    # weights
    for bad in ([0.5, 0.5], [0.25] * 4):
        with pytest.raises(ValueError, match="one a field"):
            names.match_records(both, weights=bad)
    for bad in ([0.5, 0.5, 0.0], [0.5, -0.25, 0.75], [0.5, np.nan, 0.5], [np.inf, 0.5, 0.5]):
        with pytest.raises(ValueError, match="finite and greater than 0"):
            names.match_records(both, weights=bad)
    with pytest.raises(TypeError):
        names.match_records(both, weights=["a", "b", "c"])
    # candidates
    with pytest.raises(TypeError):
        names.match_records(both, candidates=dict(min_similarity=0.5, ngram_size=2))
    with pytest.raises(TypeError):
        names.match_records(both, candidates=[0.5, 20])
    with pytest.raises(ValueError, match="2048"):
        names.match_records(both, candidates=dict(max_n_matches=2049))
    with pytest.raises(ValueError, match="whole number"):
        names.match_records(both, candidates=dict(max_n_matches=0))
    names.match_records(both, candidates=dict(max_n_matches=2048))
    names.match_records(both, candidates=dict(max_n_matches=None))                   # 12 records: all of them are candidates
    with pytest.raises(ValueError, match="one a field"):                              # a first field alone is no set of duplicates
        names.match_records(both, duplicates=[NEW])
    # duplicates
    with pytest.raises(TypeError):
        names.match_records(both, duplicates=NEW)
    with pytest.raises(ValueError, match="one a field"):
        names.match_records(both, duplicates=[NEW, NEW_ADDRESS])
    with pytest.raises(ValueError, match="differ in length"):
        names.match_records(both, duplicates=[NEW, NEW_ADDRESS, NEW_CITY[:-1]])
    with pytest.raises(TypeError):
        names.match_records(both, duplicates=[NEW, NEW_ADDRESS, pd.Series(range(len(NEW)))])
    with pytest.raises(ValueError, match="duplicates_id without duplicates"):
        names.match_records(both, duplicates_id=pd.Series(range(len(NEW))))
    # options
    with pytest.raises(TypeError):
        names.match_records(both, no_such_option=1)
    with pytest.raises(ValueError, match="ngram_size"):
        names.match_records(both, ngram_size=2)
    with pytest.raises(NotImplementedError, match="n_blocks"):
        names.match_records(both, n_blocks=(1, 1))
    with pytest.raises(NotImplementedError, match="n_blocks"):
        names.group_similar_records(both, n_blocks=(2, 1))
    assert eng.record_calls == [(12, 7), (12, 2), (12, 2)], "a refused call reached the engine"
    # corpora that do not go together
    other_ngrams = sga.Corpus(CITY, ngram_size=2)
    with pytest.raises(ValueError, match="ngram_size"):
        names.match_records([other_ngrams], ngram_size=3)
    other_dtype = sga.Corpus(CITY, tfidf_matrix_dtype=np.float32)
    with pytest.raises(ValueError, match="tfidf_matrix_dtype"):
        names.match_records([addresses, other_dtype])
    shorter = sga.Corpus(CITY[:-1])
    with pytest.raises(ValueError, match="differ in length"):
        names.match_records([addresses, shorter])
    cities.append(pd.Series(["Gotham"]))                                             # (rows waiting to be joined count)
    with pytest.raises(ValueError, match="differ in length"):
        names.match_records(both)
    cities.remove([-1])
    names.match_records(both)
    cities.close()
    with pytest.raises(ValueError, match="closed"):
        names.match_records(both)
    names.close()
    with pytest.raises(ValueError, match="closed"):
        names.match_records([addresses])


def test_all_candidates_of_a_list_longer_than_the_cap_are_refused():
    E.set_engine(RecordOracleEngine(use_port=True))
    n = sga.Corpus.MAX_RECORD_CANDIDATES + 1
    long_a = pd.Series([f"a{i:04d}" for i in range(n)])
    long_b = pd.Series([f"b{i:04d}" for i in range(n)])
    a, b = sga.Corpus(long_a), sga.Corpus(long_b)
    with pytest.raises(ValueError, match="2048"):
        a.match_records([b], candidates=dict(max_n_matches=None))
    with pytest.raises(ValueError, match="2048"):                                     # ... and when None is the corpus's own option
        sga.Corpus(long_a, max_n_matches=None).match_records([b])
    short_a, short_b = sga.Corpus(long_a[:12]), sga.Corpus(long_b[:12])               # None counts the RIGHT side's rows
    with pytest.raises(ValueError, match="2048"):
        short_a.match_records([short_b], duplicates=[long_a, long_b], candidates=dict(max_n_matches=None))
    assert E.get_engine().record_calls == [] and a.stats["record_calls"] == 0


class _OverflowingEngine(RecordOracleEngine):
    def corpus_records(self, *args, **kwargs):
        self.record_calls.append("overflow")
        raise OverflowError("rows x candidates exceed the result index")


def test_an_overflow_is_refused_and_never_answered_with_the_one_field_match():
    """fit() answers an OverflowError of the engine with the block-wise multiply of ONE field; a record call must not."""
    eng = _OverflowingEngine(use_port=True)
    E.set_engine(eng)
    names, addresses, cities = sga.Corpus(CORPUS), sga.Corpus(ADDRESS), sga.Corpus(CITY)
    multiplies = len(eng.calls)
    for call in (lambda: names.match_records([addresses, cities], weights=W, candidates=CAND, min_similarity=0.3),
                 lambda: names.group_similar_records([addresses, cities]),
                 lambda: names.match_records([addresses, cities], duplicates=[NEW, NEW_ADDRESS, NEW_CITY])):
        with pytest.raises(ValueError, match=r"candidates\['max_n_matches'\]"):
            call()
    assert eng.record_calls == ["overflow"] * 3
    assert len(eng.calls) == multiplies, "the one-field multiply ran after the overflow"
    names.match_strings(names.master)                                                # the corpus still answers
    assert len(eng.calls) == multiplies + 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_whose_first_series_is_the_master_are_still_duplicates(dtype):
    names, addresses, cities, eng = _corpora(tfidf_matrix_dtype=dtype)
    other_address, other_city = ADDRESS[::-1].reset_index(drop=True), CITY[::-1].reset_index(drop=True)
    dupes = [names.master, other_address, other_city]
    got = names.match_records([addresses, cities], duplicates=dupes, weights=W, candidates=CAND, min_similarity=0.3)
    want = composed_route(names, [addresses, cities], W, CAND, 0.3, 20, duplicates=dupes)
    pd.testing.assert_frame_equal(got, want)
    own = names.match_records([addresses, cities], weights=W, candidates=CAND, min_similarity=0.3, force_symmetries=False)
    assert not got.similarity.equals(own.similarity)                                 # the fields given were the ones scored
    assert addresses.stats["transforms"] >= 1 and cities.stats["transforms"] >= 1


def test_engines_that_match_no_records_and_engines_that_changed():
    E.set_engine(PairCorpusOracleEngine(use_port=True))
    names, addresses = sga.Corpus(CORPUS), sga.Corpus(ADDRESS)
    with pytest.raises(NotImplementedError, match="matches no records"):
        names.match_records([addresses])
    E.set_engine(RecordOracleEngine(use_port=True))
    with pytest.raises(RuntimeError, match="engine has changed"):
        names.match_records([addresses])
    mine = sga.Corpus(CORPUS)
    with pytest.raises(RuntimeError, match="engine"):
        mine.match_records([addresses])
    from string_grouper_amd.engine import DistributedHipEngine
    with pytest.raises(NotImplementedError, match="single-GPU"):
        DistributedHipEngine.corpus_records(None)


def test_the_surface():
    assert "match_records" in sga.__all__ and callable(sga.match_records)
    assert hasattr(sga.Corpus, "match_records") and hasattr(sga.Corpus, "group_similar_records")
    assert not hasattr(string_grouper, "match_records") and not hasattr(string_grouper, "Corpus")
    # nothing changes for a grouper that does not use the hook: the engine's match_list is what fit() calls
    from string_grouper_amd.string_grouper import StringGrouper
    seen = []

    class Eng:
        def match_list(self, A, B, top_n, thr, fix, keep_on_device=False):
            seen.append((top_n, thr, fix, keep_on_device))
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), 0

    g = StringGrouper(CORPUS, max_n_matches=7, min_similarity=0.6)
    g._engine_match_list(Eng(), None, None, True)
    assert seen == [(7, 0.6, True, True)]
