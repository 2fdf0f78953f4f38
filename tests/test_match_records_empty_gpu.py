"""GPU tests of ``match_records(empty_fields="skip")``: the 2 000 synthetic records of tests/test_match_records_gpu.py with about
a fifth of the addresses and a tenth of the cities blank -- ``""``, a few strings shorter than an n-gram, a few records all of
whose further fields are blank, a few without a name -- against the COMPOSED ROUTE of tests/_record_empty_oracle.py under
``assert_frame_equal``: the self-join, the forward and the reverse path, after an append and a remove, candidates from two
fields, a floor on the city, the field columns, the groups; the same records WITHOUT blanks, where the option changes no bit;
and the counter.  No tolerance anywhere."""
import functools

import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
from tests._record_empty_oracle import composed_groups_skip, composed_route_skip, skip_pairs
from tests.test_match_records_gpu import CAND, FINAL, N_BATCH, N_EXTRA, N_RECORDS, W, _corpora, eng, records  # noqa: F401

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
N_NAMELESS = 12


@functools.lru_cache(maxsize=None)
def blanked():
    """(master, batch) of ``records()`` with blanks, seeded.  Needs the engine: call it inside a test."""
    master, batch, _ = records()
    rng = np.random.default_rng(78)
    out = []
    for frame in (master, batch):
        frame = frame.copy()
        n = len(frame)
        address = np.where(rng.random(n) < 0.2, "", frame.address.to_numpy(object))
        city = np.where(rng.random(n) < 0.1, "", frame.city.to_numpy(object))
        address[rng.choice(n, 8, replace=False)] = "ab"                           # shorter than ngram_size = 3
        city[rng.choice(n, 4, replace=False)] = "x"
        both = rng.choice(n, 10, replace=False)                                  # every further field blank
        address[both], city[both] = "", ""
        frame["address"], frame["city"] = address, city
        out.append(frame)
    master, batch = out
    known = np.flatnonzero((master.address.str.len() > 3).to_numpy())            # records without a name, with an address
    name = master.name.to_numpy(object).copy()
    name[rng.choice(known, N_NAMELESS, replace=False)] = ""
    master["name"] = name
    return master, batch


def _held(names, others, duplicates=None, duplicates_id=None, min_rows=20, **kw):
    """match_records with "skip" against the composed route, exactly; returns the frame."""
    floors = kw.get("field_min_similarity")
    got = names.match_records(others, duplicates=duplicates, duplicates_id=duplicates_id, weights=W, candidates=CAND,
                              force_symmetries=False, empty_fields="skip", **FINAL, **kw)
    want = composed_route_skip(names, others, W, CAND, FINAL["min_similarity"], FINAL["max_n_matches"], floors, duplicates,
                               duplicates_id, kw.get("candidate_fields", (0,)), kw.get("field_similarities", False))
    pd.testing.assert_frame_equal(got, want)
    assert len(got) >= min_rows
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_skip_equals_the_composed_route_as_the_corpora_live(eng, dtype):
    master, batch = blanked()
    assert 0.15 < (master.address == "").mean() < 0.25 and 0.07 < (master.city == "").mean() < 0.14
    names, addresses, cities = _corpora(master, dtype)
    others = [addresses, cities]
    try:
        before = [c.stats for c in (names, addresses, cities)]
        self_join = _held(names, others, min_rows=N_RECORDS - N_NAMELESS)                       # the self-join
        zero = names.match_records(others, weights=W, candidates=CAND, force_symmetries=False, **FINAL)
        assert len(self_join) > len(zero)             # (leaving a field out never lowers a pair: non-negative scores, wp <= wt)
        first = batch.iloc[:N_BATCH].reset_index(drop=True)
        forward = names.stats["forward"]
        _held(names, others, [first.name, first.address, first.city], first.id)                # corpus x 500: forward path
        assert names.stats["forward"] > forward
        few = batch.iloc[:20].reset_index(drop=True)
        reverse = names.stats["reverse"]
        _held(names, others, [few.name, few.address, few.city], few.id, min_rows=3)            # corpus x 20: reverse path
        assert names.stats["reverse"] > reverse
        for c, b in zip((names, addresses, cities), before):                                   # the counter, on every corpus
            assert c.stats["record_skip_empty_calls"] == b["record_skip_empty_calls"] + 3
            assert c.stats["record_calls"] == b["record_calls"] + 4
        # after an append on all three: the delta segment waits
        extra = batch.iloc[N_BATCH:].set_axis(range(N_RECORDS, N_RECORDS + N_EXTRA))
        names.append(extra.name, extra.id)
        addresses.append(extra.address)
        cities.append(extra.city)
        grown = _held(names, others, min_rows=N_RECORDS)
        assert grown.left_index.max() >= N_RECORDS
        _held(names, others, [few.name, few.address, few.city], few.id, min_rows=3)
        # after a remove on all three, compact() on one of them only: dead rows lie next to blank ones
        n = len(names.master)
        blank = np.flatnonzero((addresses.master == "").to_numpy())
        drop = sorted({0, 5, 6, 700, n - N_EXTRA - 1, n - 3, int(blank[3]) - 1, int(blank[7]) + 1, int(blank[9])})
        for c in (names, addresses, cities):
            c.remove(drop)
        cities.compact()
        assert addresses.stats["dead_rows"] == len(drop) and cities.stats["dead_rows"] == 0
        _held(names, others, [few.name, few.address, few.city], few.id, min_rows=3)
        _held(names, others, min_rows=n - len(drop) - N_NAMELESS)
        assert addresses.stats["dead_rows"] == len(drop) and addresses.stats["compactions"] == 0
    finally:
        for c in (names, addresses, cities):
            c.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_skip_with_the_other_options_and_the_groups(eng, dtype):
    master, batch = blanked()
    names, addresses, cities = _corpora(master, dtype)
    others = [addresses, cities]
    try:
        # candidates from the names and the addresses: a record without a name is found by its address, field 0 is empty for it
        union = _held(names, others, candidate_fields=(0, 1), min_rows=N_RECORDS)
        nameless = set(np.flatnonzero((master.name == "").to_numpy()))
        off = union[union.left_index != union.right_index]
        assert any(a in nameless or b in nameless for a, b in zip(off.left_index, off.right_index))
        _, _, _, _, empty = skip_pairs(names, others, W, CAND, FINAL["min_similarity"], FINAL["max_n_matches"], None, None, (0, 1))
        assert empty[0].any() and empty[1].any() and empty[2].any()
        few = batch.iloc[:20].reset_index(drop=True)
        _held(names, others, [few.name, few.address, few.city], few.id, min_rows=3, candidate_fields=(0, 1))
        # a floor on the city: not held against a pair whose city is unknown
        floors = [None, None, 0.9]
        with_floor = _held(names, others, field_min_similarity=floors)
        plain = _held(names, others)
        assert 100 < len(with_floor) < len(plain)
        cityless = set(np.flatnonzero((master.city.str.len() < 3).to_numpy()))
        off = with_floor[with_floor.left_index != with_floor.right_index]
        assert any(a in cityless or b in cityless for a, b in zip(off.left_index, off.right_index))
        _held(names, others, field_min_similarity=floors, candidate_fields=(0, 1))
        # the field columns: unchanged, an empty field shows 0.0
        columns = _held(names, others, field_similarities=True)
        assert (columns.similarity_2[columns.left_index.isin(cityless) | columns.right_index.isin(cityless)] == 0.0).all()
        # the defaults: a record matches itself with 1 -- one all of whose fields are blank too -- and the list is symmetric
        got = names.match_records(others, weights=W, candidates=CAND, empty_fields="skip", **FINAL)
        diag = got[got.left_index == got.right_index]
        assert len(diag) == N_RECORDS and (diag.similarity == 1.0).all()
        pairs = set(zip(got.left_index, got.right_index))
        assert pairs == {(b, a) for a, b in pairs} and pairs >= set(zip(plain.left_index, plain.right_index))
        groups = names.group_similar_records(others, weights=W, candidates=CAND, empty_fields="skip", **FINAL)
        want = composed_groups_skip(names, others, W, CAND, FINAL["min_similarity"], FINAL["max_n_matches"])
        pd.testing.assert_frame_equal(groups, want)
        # the module-level function fits the same corpora, calls and closes them
        frame = sga.match_records([master.name, master.address, master.city], master_id=master.id, weights=W, candidates=CAND,
                                  tfidf_matrix_dtype=dtype, empty_fields="skip", **FINAL)
        pd.testing.assert_frame_equal(frame, got)
    finally:
        for c in (names, addresses, cities):
            c.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_records_without_blanks_skip_and_zero_give_equal_frames(eng, dtype):
    master, batch, _ = records()
    names, addresses, cities = _corpora(master, dtype)
    others = [addresses, cities]
    try:
        few = batch.iloc[:20].reset_index(drop=True)
        for kw in (dict(), dict(duplicates=[few.name, few.address, few.city], duplicates_id=few.id), dict(candidate_fields=(0, 1)),
                   dict(field_min_similarity=[None, None, 0.5]), dict(weights=None)):
            kw = {**dict(weights=W, candidates=CAND, force_symmetries=False), **FINAL, **kw}
            skip = names.match_records(others, empty_fields="skip", **kw)
            pd.testing.assert_frame_equal(skip, names.match_records(others, **kw))
            assert len(skip)
        assert names.stats["record_skip_empty_calls"] == 5 == cities.stats["record_skip_empty_calls"]
    finally:
        for c in (names, addresses, cities):
            c.close()
