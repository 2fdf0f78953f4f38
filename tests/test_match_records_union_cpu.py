"""CPU tests of ``candidate_fields`` -- record matching with candidates from several fields -- on the engine double of
tests/_record_oracle.py: every new argument check, the default's route, the frame against the composed union route
(match_strings a candidate field, the union in pandas, pair_similarities on every field, the numpy chain), the counters, and the
pair that only an address finds.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from tests._record_oracle import ALL_OPTIONS, RecordOracleEngine, composed_route
from tests._record_union_oracle import composed_union_groups, composed_union_route
from tests.test_corpus_cpu import CORPUS, NEW
from tests.test_match_records_cpu import ADDRESS, CAND, CITY, NEW_ADDRESS, NEW_CITY, W

DTYPES = [np.float32, np.float64]
# two records that share address and city exactly and whose names share no n-gram, among records that share nothing
ONLY_NAMES = pd.Series(["Zyxwv Qrstu Limited", "Bcdfg Hjklm GmbH", "Mnopq Aeiou Inc", "Jjjkk Lllmm Co"], name="name")
ONLY_ADDRESS = pd.Series(["12 Harbour Road", "12 Harbour Road", "7 Hill Lane", "301 Ocean Drive"], name="address")
ONLY_CITY = pd.Series(["Portsmouth", "Portsmouth", "Leeds", "Miami"], name="city")


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


def _corpora(series=(CORPUS, ADDRESS, CITY), **kwargs):
    eng = RecordOracleEngine(use_port=True)
    E.set_engine(eng)
    return [sga.Corpus(s, **kwargs) for s in series] + [eng]


# ------------------------------------------------------------------------------------------ the frame
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_frame_is_the_composed_union_route_s(dtype):
    names, addresses, cities, eng = _corpora(tfidf_matrix_dtype=dtype)
    both = [addresses, cities]
    narrow = dict(min_similarity=0.6, max_n_matches=3)
    for fields, cand, thr, top_n in (((0, 1), narrow, 0.3, 3), ((0, 1, 2), narrow, 0.45, 1), ((0, 2), CAND, 0.15, 20),
                                     ((0, 1), [narrow, dict(min_similarity=0.2, max_n_matches=5)], 0.3, 4)):
        got = names.match_records(both, weights=W, candidates=cand, candidate_fields=fields, min_similarity=thr,
                                  max_n_matches=top_n, force_symmetries=False)
        want = composed_union_route(names, both, W, cand, fields, thr, top_n)
        pd.testing.assert_frame_equal(got, want)
        assert len(got) > 0
    assert [c[0] for c in eng.union_calls] == [(0, 1), (0, 1, 2), (0, 2), (0, 1)]
    assert all(before > after > 0 for _, before, after in eng.union_calls)           # the fields' candidates overlap, and unite
    # more pairs than the names alone find at the same options
    one = names.match_records(both, weights=W, candidates=narrow, min_similarity=0.3, max_n_matches=20, force_symmetries=False)
    two = names.match_records(both, weights=W, candidates=narrow, candidate_fields=(0, 1), min_similarity=0.3, max_n_matches=20,
                              force_symmetries=False)
    assert set(zip(one.left_index, one.right_index)) < set(zip(two.left_index, two.right_index))
    dupes = [NEW, NEW_ADDRESS, NEW_CITY]
    got = names.match_records(both, duplicates=dupes, weights=W, candidates=narrow, candidate_fields=(0, 1, 2), min_similarity=0.3,
                              max_n_matches=2)
    pd.testing.assert_frame_equal(got, composed_union_route(names, both, W, narrow, (0, 1, 2), 0.3, 2, duplicates=dupes))
    assert len(got) > 3 and list(got.columns) == list(names.match_strings(names.master, NEW).columns)
    # max_n_matches=None: every candidate of the union
    got = names.match_records(both, weights=W, candidates=narrow, candidate_fields=(0, 1), min_similarity=0.05, max_n_matches=None,
                              force_symmetries=False)
    pd.testing.assert_frame_equal(got, composed_union_route(names, both, W, narrow, (0, 1), 0.05, 6))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ids_groups_symmetry_and_the_module_level_function(dtype):
    names, addresses, cities, _ = _corpora(tfidf_matrix_dtype=dtype)
    both = [addresses, cities]
    groups = names.group_similar_records(both, weights=W, candidates=CAND, candidate_fields=(0, 1), min_similarity=0.3)
    pd.testing.assert_frame_equal(groups, composed_union_groups(names, both, W, CAND, (0, 1), 0.3, 20))
    ids = pd.Series([f"id{i}" for i in range(len(CORPUS))], name="id")
    with_ids = sga.Corpus(CORPUS, master_id=ids, tfidf_matrix_dtype=dtype)
    got = with_ids.match_records(both, weights=W, candidates=CAND, candidate_fields=(0, 2), min_similarity=0.3, force_symmetries=False)
    pd.testing.assert_frame_equal(got, composed_union_route(with_ids, both, W, CAND, (0, 2), 0.3, 20))
    assert "left_id" in got.columns
    sym = names.match_records(both, weights=W, candidates=CAND, candidate_fields=(0, 1), min_similarity=0.3)
    pairs = set(zip(sym.left_index, sym.right_index))
    diag = sym[sym.left_index == sym.right_index]
    assert pairs == {(b, a) for a, b in pairs} and len(diag) == len(CORPUS) and (diag.similarity == 1.0).all()
    got = sga.match_records([CORPUS, ADDRESS, CITY], weights=W, candidates=CAND, candidate_fields=(0, 1), min_similarity=0.3,
                            max_n_matches=3, force_symmetries=False, tfidf_matrix_dtype=dtype)
    pd.testing.assert_frame_equal(got, composed_union_route(names, both, W, CAND, (0, 1), 0.3, 3))


# ------------------------------------------------------------------------------------------ the pair only an address finds
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_pair_that_agrees_on_address_and_city_alone_is_found_with_candidate_fields(dtype):
    names, addresses, cities, eng = _corpora((ONLY_NAMES, ONLY_ADDRESS, ONLY_CITY), tfidf_matrix_dtype=dtype)
    assert names.pair_similarities([0], [1])[0] == 0                                  # no n-gram in common
    assert addresses.pair_similarities([0], [1])[0] > 0.99 and cities.pair_similarities([0], [1])[0] > 0.99
    kw = dict(weights=W, candidates=dict(min_similarity=0.5, max_n_matches=4), min_similarity=0.3, force_symmetries=False)
    default = names.match_records([addresses, cities], **kw)
    assert (0, 1) not in set(zip(default.left_index, default.right_index))            # the names never compared them
    for fields in ((0, 1), (0, 2), (0, 1, 2)):
        got = names.match_records([addresses, cities], candidate_fields=fields, **kw)
        at = got[(got.left_index == 0) & (got.right_index == 1)]
        assert len(at) == 1 and (1, 0) in set(zip(got.left_index, got.right_index))
        acc = np.zeros(1, dtype)                                                     # the names' score of the pair is the fill's: 0
        for w, c in zip(W, (names, addresses, cities)):
            acc = acc + np.dtype(dtype).type(w) * c.pair_similarities([0], [1])
        assert acc.dtype == dtype and at.similarity.iloc[0] == np.float64(acc[0]) > 0.49
    got = sga.match_records([ONLY_NAMES, ONLY_ADDRESS, ONLY_CITY], candidate_fields=(0, 1), tfidf_matrix_dtype=dtype, **kw)
    assert (0, 1) in set(zip(got.left_index, got.right_index))


# ------------------------------------------------------------------------------------------ the default's route, counters
def test_the_default_takes_the_route_it_took_and_counts_as_it_did():
    names, addresses, cities, eng = _corpora()
    both = [addresses, cities]
    before = [c.stats for c in (names, addresses, cities)]
    for kw in ({}, dict(candidate_fields=(0,)), dict(candidate_fields=[0])):
        got = names.match_records(both, weights=W, candidates=CAND, min_similarity=0.3, force_symmetries=False, **kw)
        pd.testing.assert_frame_equal(got, composed_route(names, both, W, CAND, 0.3, 20))
    names.group_similar_records(both, candidate_fields=(0,))
    assert eng.record_calls == [(12, 2)] * 4 and eng.union_calls == []
    for c, b in zip((names, addresses, cities), before):
        assert c.stats["record_calls"] == b["record_calls"] + 4 and c.stats["record_union_calls"] == 0
    names.match_records(both, candidate_fields=(0, 2))
    assert eng.record_calls == [(12, 2)] * 4 and [c[0] for c in eng.union_calls] == [(0, 2)]
    assert [c.stats["record_union_calls"] for c in (names, addresses, cities)] == [1, 0, 1]
    assert [c.stats["record_calls"] - b["record_calls"] for c, b in zip((names, addresses, cities), before)] == [5, 5, 5]
    for c in (names, addresses, cities):
        assert c.stats["compactions"] == 0 and c.stats["tokenisations"] == 1 and c.stats["transforms"] == 0


def test_an_engine_without_the_union_refuses_it_and_serves_the_default():
    E.set_engine(RecordOracleEngine(use_port=True, options=ALL_OPTIONS - {"union"}))
    names, addresses = sga.Corpus(CORPUS), sga.Corpus(ADDRESS)
    names.match_records([addresses], candidate_fields=(0,))
    with pytest.raises(NotImplementedError, match="unites no candidates"):
        names.match_records([addresses], candidate_fields=(0, 1))
    with pytest.raises(NotImplementedError, match="unites no candidates"):
        names.group_similar_records([addresses], candidate_fields=(0, 1))
    from string_grouper_amd.engine import DistributedHipEngine
    with pytest.raises(NotImplementedError, match="single-GPU"):
        DistributedHipEngine.corpus_records(None)


class _OverflowingEngine(RecordOracleEngine):
    def corpus_records(self, *args, **kwargs):
        self.union_calls.append("overflow")
        raise OverflowError("rows x candidates exceed the result index")


def test_an_overflow_of_the_union_is_refused_like_the_records():
    eng = _OverflowingEngine(use_port=True)
    E.set_engine(eng)
    names, addresses, cities = sga.Corpus(CORPUS), sga.Corpus(ADDRESS), sga.Corpus(CITY)
    multiplies = len(eng.calls)
    with pytest.raises(ValueError, match=r"candidates\['max_n_matches'\]"):
        names.match_records([addresses, cities], candidate_fields=(0, 1))
    assert eng.union_calls == ["overflow"] and len(eng.calls) == multiplies


# ------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    names, addresses, cities, eng = _corpora()
    both = [addresses, cities]
    for bad in (1, None, "01", 0.5):
        with pytest.raises(TypeError, match="candidate_fields"):
            names.match_records(both, candidate_fields=bad)
    for bad in ((0, "1"), (0, 1.0), (0, True), (None,)):
        with pytest.raises(TypeError, match="candidate_fields"):
            names.match_records(both, candidate_fields=bad)
    for bad in ((0, 3), (-1, 0), (0, 1, 2, 3)):
        with pytest.raises(ValueError, match="between 0 and 2"):
            names.match_records(both, candidate_fields=bad)
    for bad in ((), (1,), (1, 2), (1, 0), (0, 1, 1), (0, 0), (0, 2, 1)):
        with pytest.raises(ValueError, match="ascending"):
            names.match_records(both, candidate_fields=bad)
    with pytest.raises(ValueError, match="ascending"):
        names.group_similar_records(both, candidate_fields=(1,))
    with pytest.raises(ValueError, match="ascending"):
        sga.match_records([CORPUS, ADDRESS, CITY], candidate_fields=(2, 0))
    # candidates: one dict for all, or one a candidate field
    with pytest.raises(ValueError, match="one a candidate field"):
        names.match_records(both, candidate_fields=(0, 1), candidates=[CAND])
    with pytest.raises(ValueError, match="one a candidate field"):
        names.match_records(both, candidate_fields=(0, 1), candidates=[CAND] * 3)
    with pytest.raises(ValueError, match="one a candidate field"):
        names.match_records(both, candidates=[CAND, CAND])
    with pytest.raises(TypeError):
        names.match_records(both, candidate_fields=(0, 1), candidates=[CAND, dict(ngram_size=2)])
    with pytest.raises(TypeError):
        names.match_records(both, candidate_fields=(0, 1), candidates=[CAND, 5])
    with pytest.raises(ValueError, match="whole number"):
        names.match_records(both, candidate_fields=(0, 1), candidates=[CAND, dict(max_n_matches=0)])
    with pytest.raises(ValueError, match="2048"):
        names.match_records(both, candidate_fields=(0, 1), candidates=[CAND, dict(max_n_matches=2049)])
    # the candidate fields' max_n_matches together
    with pytest.raises(ValueError, match=r"fields \[0, 2\] \(1024 \+ 1025\) exceed together the 2048"):
        names.match_records(both, candidate_fields=(0, 2), candidates=[dict(max_n_matches=1024), dict(max_n_matches=1025)])
    with pytest.raises(ValueError, match="exceed together the 2048"):
        names.match_records(both, candidate_fields=(0, 1, 2), candidates=dict(max_n_matches=683))
    assert eng.record_calls == [] and eng.union_calls == [], "a refused call reached the engine"
    names.match_records(both, candidate_fields=(0, 2), candidates=[dict(max_n_matches=1024), dict(max_n_matches=1024)])
    names.match_records(both, candidate_fields=[0, 1], candidates=[CAND, dict(max_n_matches=None)])   # 12 records: all of them
    names.match_records(both, candidate_fields=np.array([0, 1]))
    names.match_records(both, candidates=[CAND])                                      # one dict for the one candidate field
    assert len(eng.union_calls) == 3 and len(eng.record_calls) == 1
    # a field's own corpus options fill what the dict leaves out
    own = sga.Corpus(ADDRESS, min_similarity=0.55, max_n_matches=2)
    got = names.match_records([own, cities], weights=W, candidate_fields=(0, 1), candidates=dict(max_n_matches=7), min_similarity=0.3,
                              force_symmetries=False)
    want = composed_union_route(names, [own, cities], W, [dict(max_n_matches=7, min_similarity=names._config.min_similarity),
                                                          dict(max_n_matches=7, min_similarity=0.55)], (0, 1), 0.3, 14)
    pd.testing.assert_frame_equal(got, want)
    # everything else is refused as before
    with pytest.raises(NotImplementedError, match="n_blocks"):
        names.match_records(both, candidate_fields=(0, 1), n_blocks=(1, 1))
    with pytest.raises(ValueError, match="ngram_size"):
        names.match_records(both, candidate_fields=(0, 1), ngram_size=2)
    with pytest.raises(ValueError, match="one a field"):
        names.match_records(both, candidate_fields=(0, 1), weights=[0.5, 0.5])
