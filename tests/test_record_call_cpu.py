"""CPU tests of the description of a record call (string_grouper_amd/record_call.py): ``checked_record_call`` called directly,
``RecordCall``'s invariants, and -- on the one engine double of tests/_record_oracle.py -- the combinations of
``candidate_fields`` with ``field_min_similarity``, ``empty_fields="skip"`` and ``field_similarities`` against their composed
routes.  No GPU."""
import glob
import os

import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from string_grouper_amd.record_call import MAX_RECORD_CANDIDATES, RecordCall, checked_record_call
from string_grouper_amd.string_grouper import StringGrouperConfig
from tests._record_empty_oracle import composed_route_skip
from tests._record_floor_oracle import composed_union_route_floors
from tests._record_oracle import RecordOracleEngine
from tests._record_union_oracle import composed_union_route
from tests.test_corpus_cpu import CORPUS, NEW
from tests.test_match_records_cpu import ADDRESS, CAND, CITY, NEW_ADDRESS, NEW_CITY, W
from tests.test_match_records_empty_cpu import ADDRESS_B, CITY_B, NEW_ADDRESS_B, NEW_CITY_B
from tests.test_match_records_fields_cpu import _columns_equal_pair_similarities

DTYPES = [np.float32, np.float64]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [StringGrouperConfig(), StringGrouperConfig(min_similarity=0.55, max_n_matches=7), StringGrouperConfig()]


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


# ------------------------------------------------------------------------------------------ checked_record_call
def test_a_valid_call_is_the_normalised_description():
    call = checked_record_call(CONFIGS, 12, None, None)
    assert call == RecordCall((1 / 3,) * 3, (0,), ((20, 0.8),))
    assert call.weights == (1 / 3, 1 / 3, 1 / 3) and all(type(w) is float for w in call.weights)
    assert call.floors is None and call.field_scores is False and call.skip_empty is False
    assert (call.n_fields, call.union, call.all_candidates, call.needs) == (3, False, 20, frozenset())
    call = checked_record_call(CONFIGS, 12, [1, np.float32(0.5), 2], dict(max_n_matches=None), (0, 1))
    assert call.weights == (1.0, 0.5, 2.0) and all(type(w) is float for w in call.weights)
    assert call.candidates == ((12, 0.8), (12, 0.55))            # one dict for every candidate field; None: the right rows
    assert all(type(k) is int and type(m) is float for k, m in call.candidates)
    assert call.candidate_fields == (0, 1) and call.all_candidates == 24
    call = checked_record_call(CONFIGS, 12, None, [dict(max_n_matches=3), {}], np.array([0, 1]))
    assert call.candidates == ((3, 0.8), (7, 0.55))              # a field's own corpus fills what its dict leaves out
    assert type(call.candidates) is tuple and type(call.candidate_fields) is tuple
    assert checked_record_call(CONFIGS, 12, None, None, field_min_similarity=[None, None, None]).floors is None
    assert checked_record_call(CONFIGS, 12, None, None, field_min_similarity=[0, None, np.float32(0.5)]).floors == (0.0, None, 0.5)


def test_needs_names_every_option_alone_and_all_four_together():
    def needs(**kw):
        return checked_record_call(CONFIGS, 12, None, None, **kw).needs
    assert needs(candidate_fields=(0, 2)) == {"union"}
    assert needs(field_min_similarity=[None, 0.5, None]) == {"floors"}
    assert needs(field_similarities=True) == {"field_scores"}
    assert needs(empty_fields="skip") == {"skip_empty"}
    assert needs(candidate_fields=(0,), field_min_similarity=None, field_similarities=False, empty_fields="zero") == set()
    assert needs(candidate_fields=(0, 1, 2), field_min_similarity=[0.1, None, None], field_similarities=True,
                 empty_fields="skip") == {"union", "floors", "field_scores", "skip_empty"}
    assert needs(candidate_fields=(0, 1, 2), field_min_similarity=[0.1, None, None], field_similarities=True,
                 empty_fields="skip") == E.HipEngine.RECORD_OPTIONS


def test_a_description_made_by_hand_is_checked():
    RecordCall((0.5, 0.5), (0, 1), ((3, 0.5), (4, 0.5)))
    for fields, cands in (((1, 0), ((3, 0.5), (4, 0.5))),        # descending
                          ((0, 0), ((3, 0.5), (4, 0.5))),        # not distinct
                          ((1,), ((3, 0.5),)),                   # no 0
                          ((), ()),
                          ((0, 2), ((3, 0.5), (4, 0.5))),        # beyond the fields
                          ((0, 1), ((3, 0.5),)),                 # a candidates pair short
                          ((0,), ((3, 0.5), (4, 0.5))),          # one too many
                          ((0, 1), ((3, 0.5), (0, 0.5))),
                          ((0, 1), ((MAX_RECORD_CANDIDATES, 0.5), (1, 0.5)))):
        with pytest.raises(ValueError):
            RecordCall((0.5, 0.5), fields, cands)
    for weights in ((1.0,), (0.125,) * 9, (0.5, np.nan), (np.inf, 0.5)):
        with pytest.raises(ValueError):
            RecordCall(weights, (0,), ((3, 0.5),))
    for floors in ((None, None), (0.5,), (0.5, np.inf), (np.nan, None)):
        with pytest.raises(ValueError):
            RecordCall((0.5, 0.5), (0,), ((3, 0.5),), floors=floors)


# ------------------------------------------------------------------------------------------ the combinations
def _pairs(frame):
    return set(zip(frame.left_index, frame.right_index))


def _records(dtype, duplicates, blanks=False):
    E.set_engine(RecordOracleEngine(use_port=True))
    fields = (CORPUS, ADDRESS_B, CITY_B) if blanks else (CORPUS, ADDRESS, CITY)
    names, addresses, cities = (sga.Corpus(s, tfidf_matrix_dtype=dtype) for s in fields)
    dupes = None
    if duplicates:
        dupes = [NEW, NEW_ADDRESS_B, NEW_CITY_B] if blanks else [NEW, NEW_ADDRESS, NEW_CITY]
    return names, [addresses, cities], dupes


@pytest.mark.parametrize("duplicates", [False, True], ids=["self_join", "duplicates"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_candidate_fields_with_floors(dtype, duplicates):
    names, others, dupes = _records(dtype, duplicates)
    floors = [None, 0.5, None]
    want = composed_union_route_floors(names, others, W, CAND, (0, 1), 0.2, 20, floors, duplicates=dupes)
    plain = composed_union_route(names, others, W, CAND, (0, 1), 0.2, 20, duplicates=dupes)
    assert len(want) > 0 and _pairs(plain) - _pairs(want)                 # the floor keeps some and drops some
    got = names.match_records(others, duplicates=dupes, weights=W, candidates=CAND, candidate_fields=(0, 1), min_similarity=0.2,
                              max_n_matches=20, field_min_similarity=floors, force_symmetries=False)
    pd.testing.assert_frame_equal(got, want)
    assert [c.stats["record_floor_calls"] for c in [names] + others] == [1, 1, 1]
    assert [c.stats["record_union_calls"] for c in [names] + others] == [1, 1, 0]


@pytest.mark.parametrize("duplicates", [False, True], ids=["self_join", "duplicates"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_candidate_fields_with_skip(dtype, duplicates):
    names, others, dupes = _records(dtype, duplicates, blanks=True)
    want = composed_route_skip(names, others, W, CAND, 0.2, 3, duplicates=dupes, candidate_fields=(0, 1))
    plain = composed_union_route(names, others, W, CAND, (0, 1), 0.2, 3, duplicates=dupes)
    assert len(want) > 0 and _pairs(plain) - _pairs(want)                 # a pair the skip pushes out of the cut
    got = names.match_records(others, duplicates=dupes, weights=W, candidates=CAND, candidate_fields=(0, 1), min_similarity=0.2,
                              max_n_matches=3, empty_fields="skip", force_symmetries=False)
    pd.testing.assert_frame_equal(got, want)
    assert [c.stats["record_skip_empty_calls"] for c in [names] + others] == [1, 1, 1]
    assert [c.stats["record_union_calls"] for c in [names] + others] == [1, 1, 0]


@pytest.mark.parametrize("duplicates", [False, True], ids=["self_join", "duplicates"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_candidate_fields_with_field_similarities(dtype, duplicates):
    """The union's own filter keeps some pairs and drops some (against every candidate of the union, min_similarity -1); the
    field columns of every row are the fields' ``pair_similarities`` of its positions, to the bit."""
    names, others, dupes = _records(dtype, duplicates)
    want = composed_union_route(names, others, W, CAND, (0, 1), 0.3, 20, duplicates=dupes)
    every = composed_union_route(names, others, W, CAND, (0, 1), -1.0, MAX_RECORD_CANDIDATES, duplicates=dupes)
    assert len(want) > 0 and _pairs(every) - _pairs(want)
    got = names.match_records(others, duplicates=dupes, weights=W, candidates=CAND, candidate_fields=(0, 1), min_similarity=0.3,
                              max_n_matches=20, field_similarities=True, force_symmetries=False)
    pd.testing.assert_frame_equal(got.drop(columns=["similarity_0", "similarity_1", "similarity_2"]), want)
    _columns_equal_pair_similarities(got, [names] + others, dtype, dupes)
    assert [c.stats["record_field_score_calls"] for c in [names] + others] == [1, 1, 1]


# ------------------------------------------------------------------------------------------ what went
def test_no_reflection_sentinel_or_patch_in_the_record_path():
    files = [os.path.join(ROOT, "string_grouper_amd", "corpus.py")] + sorted(glob.glob(os.path.join(ROOT, "tests", "_record*_oracle.py")))
    assert len(files) == 5
    for path in files:
        with open(path) as f:
            text = f.read()
        for word in ("inspect.signature", "NOT_GIVEN", "mock.patch"):
            assert word not in text, (path, word)
