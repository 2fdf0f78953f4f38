"""CPU tests of ``field_min_similarity`` and ``field_similarities`` on the engine double of tests/_record_oracle.py:
every argument check, the default route (the descriptions that reach the engine ask for no new option), the frame with
floors against the composed route with floors, the groups, the field columns against ``pair_similarities`` on the double, the
counters, and the refusal of an engine without the capability.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from tests._record_floor_oracle import combined_pairs_floors, composed_groups_floors, composed_route_floors
from tests._record_oracle import ALL_OPTIONS, RecordOracleEngine, composed_route
from tests.test_corpus_cpu import CORPUS, NEW
from tests.test_match_records_cpu import ADDRESS, CAND, CITY, NEW_ADDRESS, NEW_CITY, W

DTYPES = [np.float32, np.float64]


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


def _corpora(options=ALL_OPTIONS, **kwargs):
    eng = RecordOracleEngine(use_port=True, options=options)
    E.set_engine(eng)
    return sga.Corpus(CORPUS, **kwargs), sga.Corpus(ADDRESS, **kwargs), sga.Corpus(CITY, **kwargs), eng


def _present_floors(names, others, dtype):
    """A floor a field that is PRESENT among the candidates' scores of that field (the median): the strict comparison bites."""
    _, _, _, lp, rp, scores = combined_pairs_floors(names, others, W, CAND, -1.0, 100, None)
    off = lp != rp
    return [float(np.sort(s[off])[len(s[off]) // 2]) for s in scores]


# ------------------------------------------------------------------------------------------ the frame
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_frame_with_floors_is_the_composed_route_s(dtype):
    names, addresses, cities, eng = _corpora(tfidf_matrix_dtype=dtype)
    others = [addresses, cities]
    m = _present_floors(names, others, dtype)
    plain = composed_route(names, others, W, CAND, 0.15, 20)
    for floors in ([m[0], None, None], [None, m[1], None], [None, None, m[2]], m, [None, None, None], [None, 0, None]):
        for thr, top_n in ((0.15, 20), (0.3, 2), (0.45, 1)):
            got = names.match_records(others, weights=W, candidates=CAND, min_similarity=thr, max_n_matches=top_n,
                                      field_min_similarity=floors, force_symmetries=False)
            want = composed_route_floors(names, others, W, CAND, thr, top_n, floors)
            pd.testing.assert_frame_equal(got, want)
        if any(x for x in floors):
            assert 0 < len(want) and len(composed_route_floors(names, others, W, CAND, 0.15, 20, floors)) < len(plain)
    assert eng.calls_seen[-1].floors == (None, 0.0, None) and all(isinstance(x, float) for x in eng.calls_seen[0].floors if x is not None)
    # the floors act BEFORE the cut: a pair the floor lets through takes the place of one it refused
    moved = 0
    for top_n in (2, 3):                                                             # (the first place is the record itself)
        cut = composed_route(names, others, W, CAND, 0.15, top_n)
        for floors in ([m[0], None, None], [None, m[1], None], [None, None, m[2]]):
            cut_floors = composed_route_floors(names, others, W, CAND, 0.15, top_n, floors)
            moved += len(cut_floors) - len(cut.merge(cut_floors, on=["left_index", "right_index"]))
    assert moved > 0
    # duplicates
    dupes = [NEW, NEW_ADDRESS, NEW_CITY]
    for floors in ([None, 0.5, None], [0.3, None, 0.2]):
        got = names.match_records(others, duplicates=dupes, weights=W, candidates=CAND, min_similarity=0.3, max_n_matches=2,
                                  field_min_similarity=floors)
        pd.testing.assert_frame_equal(got, composed_route_floors(names, others, W, CAND, 0.3, 2, floors, duplicates=dupes))
    # the module-level function
    got = sga.match_records([CORPUS, ADDRESS, CITY], weights=W, candidates=CAND, min_similarity=0.3, max_n_matches=3,
                            force_symmetries=False, tfidf_matrix_dtype=dtype, field_min_similarity=m)
    pd.testing.assert_frame_equal(got, composed_route_floors(names, others, W, CAND, 0.3, 3, m))


@pytest.mark.parametrize("dtype", DTYPES)
def test_self_matches_symmetry_and_groups_with_floors(dtype):
    names, addresses, cities, _ = _corpora(tfidf_matrix_dtype=dtype)
    others = [addresses, cities]
    floors = [None, None, _present_floors(names, others, dtype)[2]]
    got = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3, field_min_similarity=[2.0, 2.0, 2.0])
    assert len(got) == len(CORPUS) and (got.left_index == got.right_index).all() and (got.similarity == 1.0).all()
    got = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3, field_min_similarity=floors)
    unsym = composed_route_floors(names, others, W, CAND, 0.3, 20, floors)
    diag = got[got.left_index == got.right_index]
    assert len(diag) == len(CORPUS) and (diag.similarity == 1.0).all()              # whatever the floors say
    pairs = set(zip(got.left_index, got.right_index))
    assert pairs == {(b, a) for a, b in pairs} and pairs >= set(zip(unsym.left_index, unsym.right_index))
    groups = names.group_similar_records(others, weights=W, candidates=CAND, min_similarity=0.3, field_min_similarity=floors)
    pd.testing.assert_frame_equal(groups, composed_groups_floors(names, others, W, CAND, 0.3, 20, floors))
    assert not groups.equals(names.group_similar_records(others, weights=W, candidates=CAND, min_similarity=0.3))


# ------------------------------------------------------------------------------------------ the default route, the counters
def test_without_the_option_the_engine_is_called_as_before():
    names, addresses, cities, eng = _corpora()
    others = [addresses, cities]
    names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3)
    names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3, field_min_similarity=None)
    names.group_similar_records(others)
    assert [c.floors for c in eng.calls_seen] == [None] * 3                          # the descriptions carry no floors
    assert all(c.stats["record_floor_calls"] == 0 and c.stats["record_calls"] == 3 for c in (names, addresses, cities))
    names.match_records(others, field_min_similarity=[None, 0.5, None])
    names.group_similar_records(others, field_min_similarity=(0.1, None, None))
    assert [c.floors for c in eng.calls_seen[3:]] == [(None, 0.5, None), (0.1, None, None)]
    assert all(c.stats["record_floor_calls"] == 2 and c.stats["record_calls"] == 5 for c in (names, addresses, cities))
    assert all(c.stats["pair_calls"] == 0 and c.stats["compactions"] == 0 for c in (names, addresses, cities))


def test_an_engine_double_without_the_keyword_still_serves_the_old_call_and_refuses_the_new():
    names, addresses, cities, eng = _corpora(options=ALL_OPTIONS - {"floors"})
    others = [addresses, cities]
    got = names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3, force_symmetries=False)
    pd.testing.assert_frame_equal(got, composed_route(names, others, W, CAND, 0.3, 20))
    calls = list(eng.record_calls)
    for call in (names.match_records, names.group_similar_records):
        with pytest.raises(NotImplementedError, match="field_min_similarity"):
            call(others, field_min_similarity=[None, 0.5, None])
    assert eng.record_calls == calls                                                 # nothing reached the engine
    with pytest.raises(NotImplementedError, match="single-GPU"):
        E.DistributedHipEngine.corpus_records(None)


# ------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    names, addresses, cities, eng = _corpora()
    others = [addresses, cities]
    for call in (names.match_records, names.group_similar_records):
        for bad in ([0.5], [0.5, 0.5], [None] * 4, [], ()):
            with pytest.raises(ValueError, match="one a field"):
                call(others, field_min_similarity=bad)
        for bad in (np.nan, np.inf, -np.inf, float("nan"), np.float32("inf"), "0.5", 1j, [0.5], object()):
            with pytest.raises(ValueError, match="finite real number or None"):
                call(others, field_min_similarity=[None, bad, None])
        for bad in (True, False, np.bool_(True)):
            with pytest.raises(TypeError, match="bool"):
                call(others, field_min_similarity=[bad, None, None])
        for bad in (0.5, "abc", 3):
            with pytest.raises(TypeError, match="sequence"):
                call(others, field_min_similarity=bad)
    assert eng.calls_seen == []
    for good in ([0, None, 1], (np.float32(0.5), np.int64(0), -1.5), np.array([0.25, 0.5, 0.75]), [None, None, None]):
        names.match_records(others, field_min_similarity=good)
    assert len(eng.calls_seen) == 4
    assert eng.calls_seen[-1].floors is None and names.stats["record_floor_calls"] == 3   # nothing but None: the call it always was
    with pytest.raises(ValueError, match="one a field"):
        sga.match_records([CORPUS, ADDRESS, CITY], field_min_similarity=[0.5])
    with pytest.raises(TypeError, match="bool"):
        sga.match_records([CORPUS, ADDRESS, CITY], field_min_similarity=[None, None, True])


# ------------------------------------------------------------------------------------------ field_similarities
def _columns_equal_pair_similarities(frame, corpora, dtype, duplicates=None):
    """Every ``similarity_k``, cast back to the dtype, against ``corpus_k.pair_similarities`` on the row's positions: bits."""
    T = np.dtype(dtype).type
    lp = pd.Index(corpora[0].master.index).get_indexer(frame.left_index)
    rp = pd.Index((corpora[0].master if duplicates is None else duplicates[0]).index).get_indexer(frame.right_index)
    assert (lp >= 0).all() and (rp >= 0).all()
    at = list(frame.columns).index("similarity")
    assert list(frame.columns[at + 1:at + 1 + len(corpora)]) == [f"similarity_{k}" for k in range(len(corpora))]
    for k, c in enumerate(corpora):
        col = frame[f"similarity_{k}"]
        assert col.dtype == np.float64
        want = c.pair_similarities(lp, rp) if duplicates is None else c.pair_similarities(lp, rp, duplicates=duplicates[k])
        assert want.dtype == T and np.array_equal(col.to_numpy().astype(T).view(np.uint8), want.view(np.uint8)), k
        assert np.array_equal(col.to_numpy(), want.astype(np.float64))               # widened, nothing else
    return lp, rp


def _recombines(frame, lp, rp, dtype, self_join):
    """Off the diagonal, acc = acc + W[f] * similarity_f in the dtype gives ``similarity`` to the bit."""
    T = np.dtype(dtype).type
    off = lp != rp if self_join else np.ones(len(frame), bool)
    acc = np.zeros(int(off.sum()), T)
    for f, w in enumerate(W):
        acc = acc + T(w) * frame[f"similarity_{f}"].to_numpy()[off].astype(T)
    assert acc.dtype == T and np.array_equal(acc.astype(np.float64), frame.similarity.to_numpy()[off])
    return int(off.sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_field_columns_are_pair_similarities(dtype):
    names, addresses, cities, eng = _corpora(tfidf_matrix_dtype=dtype)
    corpora, others = [names, addresses, cities], [addresses, cities]
    kw = dict(weights=W, candidates=CAND, min_similarity=0.3)
    plain = names.match_records(others, **kw)
    got = names.match_records(others, field_similarities=True, **kw)             # the defaults: diagonal and mirror
    pd.testing.assert_frame_equal(got.drop(columns=["similarity_0", "similarity_1", "similarity_2"]), plain)
    lp, rp = _columns_equal_pair_similarities(got, corpora, dtype)
    assert _recombines(got, lp, rp, dtype, True) > 0
    diag = got[lp == rp]
    assert len(diag) == len(CORPUS) and (diag.similarity == 1.0).all()
    got = names.match_records(others, field_similarities=True, force_symmetries=False, **kw)
    pd.testing.assert_frame_equal(got.drop(columns=["similarity_0", "similarity_1", "similarity_2"]),
                                  composed_route(names, others, W, CAND, 0.3, 20))
    _recombines(got, *_columns_equal_pair_similarities(got, corpora, dtype), dtype, True)
    # duplicates, and both options in one call
    dupes = [NEW, NEW_ADDRESS, NEW_CITY]
    got = names.match_records(others, duplicates=dupes, field_similarities=True, **kw)
    assert len(got) > 0
    _recombines(got, *_columns_equal_pair_similarities(got, corpora, dtype, dupes), dtype, False)
    floors = [None, None, _present_floors(names, others, dtype)[2]]
    got = names.match_records(others, field_similarities=True, field_min_similarity=floors, force_symmetries=False, **kw)
    pd.testing.assert_frame_equal(got.drop(columns=["similarity_0", "similarity_1", "similarity_2"]),
                                  composed_route_floors(names, others, W, CAND, 0.3, 20, floors))
    lp, rp = _columns_equal_pair_similarities(got, corpora, dtype)
    assert (got.similarity_2.to_numpy()[lp != rp] > floors[2]).all() and (lp != rp).any()
    # ids and ignore_index
    ids = pd.Series([f"id{k}" for k in range(len(CORPUS))], index=CORPUS.index)
    with_ids = sga.Corpus(CORPUS, master_id=ids, tfidf_matrix_dtype=dtype)
    got = with_ids.match_records(others, field_similarities=True, **kw)
    assert "left_id" in got.columns and "right_id" in got.columns
    _columns_equal_pair_similarities(got, [with_ids, addresses, cities], dtype)
    ignored = with_ids.match_records(others, field_similarities=True, ignore_index=True, **kw)
    assert "left_index" not in ignored.columns
    for k in range(3):
        assert np.array_equal(ignored[f"similarity_{k}"].to_numpy(), got[f"similarity_{k}"].to_numpy())
    # include_zeroes adds rows only at min_similarity <= 0: they carry 0.0 in every field column
    zeroes = names.match_records(others, weights=W, candidates=dict(min_similarity=0.0, max_n_matches=len(CORPUS)), min_similarity=0.0,
                                 max_n_matches=len(CORPUS), field_similarities=True)
    assert len(zeroes) == len(CORPUS) ** 2
    added = zeroes[zeroes.similarity == 0]
    assert len(added) > 0 and all((added[f"similarity_{k}"] == 0.0).all() for k in range(3))
    listed = zeroes[zeroes.similarity != 0]
    _columns_equal_pair_similarities(listed, corpora, dtype)
    # the module-level function
    got = sga.match_records([CORPUS, ADDRESS, CITY], weights=W, candidates=CAND, min_similarity=0.3, tfidf_matrix_dtype=dtype,
                            field_similarities=True)
    _columns_equal_pair_similarities(got, corpora, dtype)
    assert all(c.stats["record_field_score_calls"] == 7 for c in others)             # (the module-level call has corpora of its own)


def test_without_field_similarities_the_engine_is_called_as_before_and_the_checks():
    names, addresses, cities, eng = _corpora()
    others = [addresses, cities]
    names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3)
    names.match_records(others, weights=W, candidates=CAND, min_similarity=0.3, field_similarities=False)
    names.group_similar_records(others)
    assert [(c.field_scores, c.floors) for c in eng.calls_seen] == [(False, None)] * 3    # neither option is asked for
    assert all(c.stats["record_field_score_calls"] == 0 for c in (names, addresses, cities))
    frame = names.match_records(others, field_similarities=True)
    assert [(c.field_scores, c.floors) for c in eng.calls_seen[3:]] == [(True, None)]
    assert all(c.stats["record_field_score_calls"] == 1 and c.stats["pair_calls"] == 0 for c in (names, addresses, cities))
    assert {"similarity_0", "similarity_1", "similarity_2"} <= set(frame.columns)
    for bad in (1, 0, None, "yes", [True]):
        with pytest.raises(TypeError, match="field_similarities"):
            names.match_records(others, field_similarities=bad)
    with pytest.raises(TypeError):                                                   # there is no frame of pairs
        names.group_similar_records(others, field_similarities=True)
    assert len(eng.calls_seen) == 4


def test_an_engine_double_without_field_scores_refuses_field_similarities():
    names, addresses, cities, eng = _corpora(options=ALL_OPTIONS - {"field_scores"})
    others = [addresses, cities]
    calls = list(eng.record_calls)
    with pytest.raises(NotImplementedError, match="field_similarities"):
        names.match_records(others, field_similarities=True)
    assert eng.record_calls == calls                                                 # nothing reached the engine
    names.match_records(others, field_similarities=False)
    with pytest.raises(NotImplementedError, match="single-GPU"):
        E.DistributedHipEngine.corpus_records(None)
