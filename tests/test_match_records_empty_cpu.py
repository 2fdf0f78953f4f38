"""CPU tests of ``empty_fields`` on the engine double of tests/_record_oracle.py: the argument checks, the default route
(``"zero"`` asks the engine for no skip), the frame with ``"skip"`` against the composed route -- with floors, with duplicates,
through the module-level function --, self matches, symmetry and groups, records without blanks, the counter, and the refusal
of an engine without the capability.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from tests._record_empty_oracle import composed_groups_skip, composed_route_skip, skip_pairs
from tests._record_oracle import ALL_OPTIONS, RecordOracleEngine, composed_route
from tests.test_corpus_cpu import CORPUS, NEW
from tests.test_match_records_cpu import ADDRESS, CAND, CITY, NEW_ADDRESS, NEW_CITY, W

DTYPES = [np.float32, np.float64]


def _blanked(series, blanks):
    out = series.copy()
    for at, value in blanks.items():
        out.iloc[at] = value
    return out


# a quarter of the addresses and two cities are blank: "", a string shorter than an n-gram, one that the regex empties
ADDRESS_B = _blanked(ADDRESS, {1: "", 5: "", 6: "ab", 9: "., "})
CITY_B = _blanked(CITY, {5: "", 10: ""})
# in duplicates also a string made only of n-grams the corpus has never seen
NEW_ADDRESS_B = _blanked(NEW_ADDRESS, {0: "", 3: "QQQQQQ"})
NEW_CITY_B = _blanked(NEW_CITY, {3: "Xyzzyx", 4: ""})


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


def _corpora(options=ALL_OPTIONS, address=ADDRESS_B, city=CITY_B, **kwargs):
    eng = RecordOracleEngine(use_port=True, options=options)
    E.set_engine(eng)
    return sga.Corpus(CORPUS, **kwargs), sga.Corpus(address, **kwargs), sga.Corpus(city, **kwargs), eng


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_frame_with_skip_is_the_composed_route_s(dtype):
    names, addresses, cities, eng = _corpora(tfidf_matrix_dtype=dtype)
    others = [addresses, cities]
    _, _, _, _, empty = skip_pairs(names, others, W, CAND, -1.0, 100)
    assert empty[1].any() and empty[2].any() and (empty[1] & empty[2]).any() and not empty[0].any()
    for floors in (None, [None, 0.3, None], [0.2, None, 0.5]):
        for thr, top_n in ((0.15, 20), (0.3, 2), (0.45, 1)):
            got = names.match_records(others, weights=W, candidates=CAND, min_similarity=thr, max_n_matches=top_n,
                                      field_min_similarity=floors, empty_fields="skip", force_symmetries=False)
            want = composed_route_skip(names, others, W, CAND, thr, top_n, floors)
            pd.testing.assert_frame_equal(got, want)
            assert len(got)
    seen = eng.calls_seen
    assert [c.skip_empty for c in seen] == [True] * 9 and seen[0].floors is None and seen[-1].floors == (0.2, None, 0.5)
    # the option decides: a pair with a blank address stays that the blank took under the threshold, and a floor on the
    # address is not held against it
    zero = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.45, force_symmetries=False)
    skip = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.45, empty_fields="skip", force_symmetries=False)
    pd.testing.assert_frame_equal(zero, composed_route(names, others, W, CAND, 0.45, 20))
    assert len(skip) > len(zero)
    held = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.15, field_min_similarity=[None, 0.3, None],
                               force_symmetries=False)
    not_held = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.15, field_min_similarity=[None, 0.3, None],
                                   empty_fields="skip", force_symmetries=False)
    blank = set(np.flatnonzero(ADDRESS_B.isin(["", "ab", "., "])))
    assert not any(a in blank or b in blank for a, b in zip(held.left_index, held.right_index))
    assert any(a in blank or b in blank for a, b in zip(not_held.left_index, not_held.right_index))
    # duplicates
    dupes = [NEW, NEW_ADDRESS_B, NEW_CITY_B]
    _, _, _, _, empty = skip_pairs(names, others, W, CAND, -1.0, 100, duplicates=dupes)
    assert empty[1].any() and empty[2].any()
    for floors in (None, [None, 0.5, None]):
        got = names.match_records(others, duplicates=dupes, weights=W, candidates=CAND, min_similarity=0.3, max_n_matches=2,
                                  field_min_similarity=floors, empty_fields="skip")
        pd.testing.assert_frame_equal(got, composed_route_skip(names, others, W, CAND, 0.3, 2, floors, duplicates=dupes))
    # field_similarities: the columns are unchanged, an empty field shows 0.0
    got = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3, max_n_matches=3, empty_fields="skip",
                              field_similarities=True, force_symmetries=False)
    want = composed_route_skip(names, others, W, CAND, 0.3, 3, field_similarities=True)
    pd.testing.assert_frame_equal(got, want)
    assert (got.similarity_1[got.left_index.isin(blank) | got.right_index.isin(blank)] == 0.0).all()
    # the module-level function
    got = sga.match_records([CORPUS, ADDRESS_B, CITY_B], weights=W, candidates=CAND, min_similarity=0.3, max_n_matches=3,
                            force_symmetries=False, tfidf_matrix_dtype=dtype, empty_fields="skip")
    pd.testing.assert_frame_equal(got, composed_route_skip(names, others, W, CAND, 0.3, 3))


@pytest.mark.parametrize("dtype", DTYPES)
def test_self_matches_symmetry_and_groups_with_skip(dtype):
    names, addresses, cities, _ = _corpora(tfidf_matrix_dtype=dtype)
    others = [addresses, cities]
    got = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3, empty_fields="skip")
    unsym = composed_route_skip(names, others, W, CAND, 0.3, 20)
    diag = got[got.left_index == got.right_index]
    assert len(diag) == len(CORPUS) and (diag.similarity == 1.0).all()              # also the record whose further fields are blank
    pairs = set(zip(got.left_index, got.right_index))
    assert pairs == {(b, a) for a, b in pairs} and pairs >= set(zip(unsym.left_index, unsym.right_index))
    groups = names.group_similar_records(others, weights=W, candidates=CAND, min_similarity=0.45, empty_fields="skip")
    pd.testing.assert_frame_equal(groups, composed_groups_skip(names, others, W, CAND, 0.45, 20))
    assert not groups.equals(names.group_similar_records(others, weights=W, candidates=CAND, min_similarity=0.45))


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_records_without_blanks_the_option_changes_no_bit(dtype):
    names, addresses, cities, _ = _corpora(address=ADDRESS, city=CITY, tfidf_matrix_dtype=dtype)
    others = [addresses, cities]
    for weights in (W, None, [0.1, 0.2, 0.3]):                                      # (equal shares and 0.6: wt != 1)
        kw = dict(weights=weights, candidates=CAND, min_similarity=0.2, max_n_matches=4, force_symmetries=False)
        pd.testing.assert_frame_equal(names.match_records(others, empty_fields="skip", **kw), names.match_records(others, **kw))


def test_zero_is_the_call_as_it_was_and_the_counter():
    names, addresses, cities, eng = _corpora()
    others = [addresses, cities]
    names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3)
    names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3, empty_fields="zero")
    names.group_similar_records(others, empty_fields="zero")
    sga.match_records([CORPUS, ADDRESS_B, CITY_B], empty_fields="zero")
    assert [c.skip_empty for c in eng.calls_seen] == [False] * 4                     # the descriptions do not ask to skip
    assert all(c.stats["record_skip_empty_calls"] == 0 and c.stats["record_calls"] == 3 for c in (names, addresses, cities))
    names.match_records(others, empty_fields="skip")
    names.group_similar_records(others, empty_fields="skip", field_min_similarity=[None, 0.5, None])
    assert [c.skip_empty for c in eng.calls_seen[4:]] == [True, True]
    assert all(c.stats["record_skip_empty_calls"] == 2 and c.stats["record_calls"] == 5 and c.stats["record_floor_calls"] == 1
               for c in (names, addresses, cities))


def test_an_engine_double_without_the_keyword_still_serves_zero_and_refuses_skip():
    names, addresses, cities, eng = _corpora(options=ALL_OPTIONS - {"skip_empty"})
    others = [addresses, cities]
    got = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3, force_symmetries=False, empty_fields="zero")
    pd.testing.assert_frame_equal(got, composed_route(names, others, W, CAND, 0.3, 20))
    calls = list(eng.record_calls)
    for call in (names.match_records, names.group_similar_records):
        with pytest.raises(NotImplementedError, match="empty_fields"):
            call(others, empty_fields="skip")
    assert eng.record_calls == calls                                                 # nothing reached the engine
    with pytest.raises(NotImplementedError, match="single-GPU"):
        E.DistributedHipEngine.corpus_records(None)


def test_argument_checks():
    names, addresses, cities, eng = _corpora()
    others = [addresses, cities]
    for call in (names.match_records, names.group_similar_records):
        for bad in (None, 0, 1, True, False, b"skip", ["skip"], object()):
            with pytest.raises(TypeError, match="empty_fields"):
                call(others, empty_fields=bad)
        for bad in ("", "Skip", "SKIP", "zeros", "drop", "skip "):
            with pytest.raises(ValueError, match="empty_fields"):
                call(others, empty_fields=bad)
    with pytest.raises(TypeError, match="empty_fields"):
        sga.match_records([CORPUS, ADDRESS_B, CITY_B], empty_fields=None)
    with pytest.raises(ValueError, match="empty_fields"):
        sga.match_records([CORPUS, ADDRESS_B, CITY_B], empty_fields="none")
    assert eng.calls_seen == []
