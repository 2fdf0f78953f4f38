"""GPU tests of ``field_min_similarity`` and ``field_similarities`` (the columns ``similarity_k`` against ``pair_similarities``
bit for bit on a default index, with ``ignore_index``, on a shuffled string index with ids; their recombination into
``similarity``; both options in one call): ``Corpus.match_records`` on the 2 000 three-field records of
tests/test_match_records_gpu.py against the COMPOSED ROUTE WITH FLOORS (tests/_record_floor_oracle.py: match_strings at the
candidate options, pair_similarities a further corpus, the numpy chain, the floor mask, ``>``, the order and the cut in pandas)
under ``assert_frame_equal`` -- the self-join, the forward and the reverse path, after an append and a remove, with candidates
from two fields --, the further corpora left where they lie, the defaults, and ``group_similar_records``.  A floor is a value
that is PRESENT: the median of its field's score over the off-diagonal rows of the frame without floors.  No tolerance."""
import numpy as np
import pandas as pd
import pytest

import string_grouper_amd.engine as E
from tests._record_floor_oracle import composed_groups_floors, composed_route_floors, composed_union_route_floors
from tests.test_match_records_gpu import CAND, FINAL, N_BATCH, N_EXTRA, N_RECORDS, W, _corpora, records

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
THR, TOP = FINAL["min_similarity"], FINAL["max_n_matches"]
LEFT_ALONE = ("compactions", "index_builds", "segments", "dead_rows")


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


# a batch's frame at FINAL is too short for 20 pairs to leave and 20 to stay: the 500 records are cut lower, and the 32 of the
# reverse path -- about one pair a record at CAND -- also take their candidates lower and are floored on the name, whose
# scores are all distinct: the median halves them
BATCH_FINAL = dict(min_similarity=0.3, max_n_matches=20)
FEW_CAND, FEW_FINAL = dict(min_similarity=0.3, max_n_matches=50), dict(min_similarity=0.1, max_n_matches=20)


def _median_floors(names, others, duplicates=None, duplicates_id=None, final=FINAL, cand=CAND):
    """One floor a field and the frame without floors they are taken from."""
    plain = names.match_records(others, duplicates=duplicates, duplicates_id=duplicates_id, weights=W, candidates=cand, force_symmetries=False, **final)
    off = plain[plain.left_index != plain.right_index] if duplicates is None else plain
    lp = pd.Index(names.master.index).get_indexer(off.left_index)
    rp = pd.Index((names.master if duplicates is None else duplicates[0]).index).get_indexer(off.right_index)
    floors = []
    for k, c in enumerate([names] + list(others)):
        s = np.sort(c.pair_similarities(lp, rp) if duplicates is None else c.pair_similarities(lp, rp, duplicates=duplicates[k]))
        floors.append(float(s[len(s) // 2]))
    return floors, plain


def _held(names, others, floors, plain, duplicates=None, duplicates_id=None, final=FINAL, cand=CAND):
    """match_records with floors against the composed route with floors, exactly: at least 20 pairs leave and 20 stay."""
    got = names.match_records(others, duplicates=duplicates, duplicates_id=duplicates_id, weights=W, candidates=cand,
                              field_min_similarity=floors, force_symmetries=False, **final)
    want = composed_route_floors(names, others, W, cand, final["min_similarity"], final["max_n_matches"], floors, duplicates,
                                 duplicates_id)
    pd.testing.assert_frame_equal(got, want)
    stay = len(got) if duplicates is not None else int((got.left_index != got.right_index).sum())
    assert stay >= 20 and len(plain) - len(got) >= 20, f"floors {floors}: {len(plain)} pairs without, {len(got)} with, {stay} stay"
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_floors_equal_the_composed_route_as_the_corpora_live(eng, dtype):
    master, batch, _ = records()
    names, addresses, cities = _corpora(master, dtype)
    others = [addresses, cities]
    try:
        before = [{k: c.stats[k] for k in LEFT_ALONE} for c in others]
        calls = names.stats["record_floor_calls"]
        m, plain = _median_floors(names, others)
        assert names.stats["record_floor_calls"] == calls                                      # (no floors so far)
        for floors in ([None, m[1], None], [None, None, m[2]], [m[0], None, None], m):           # the self-join
            _held(names, others, floors, plain)
        assert [c.stats["record_floor_calls"] for c in (names, addresses, cities)] == [calls + 4] * 3
        first = batch.iloc[:N_BATCH].reset_index(drop=True)
        dupes = [first.name, first.address, first.city]
        mb, plain_b = _median_floors(names, others, dupes, first.id, BATCH_FINAL)
        forward = names.stats["forward"]
        _held(names, others, [None, mb[1], None], plain_b, dupes, first.id, BATCH_FINAL)                # corpus x 500: forward path
        assert names.stats["forward"] > forward
        few = batch.iloc[:32].reset_index(drop=True)
        dupes = [few.name, few.address, few.city]
        mf, plain_f = _median_floors(names, others, dupes, few.id, FEW_FINAL, FEW_CAND)
        reverse = names.stats["reverse"]
        _held(names, others, [mf[0], None, None], plain_f, dupes, few.id, FEW_FINAL, FEW_CAND)          # corpus x 32: reverse path
        assert names.stats["reverse"] > reverse
        assert [{k: c.stats[k] for k in LEFT_ALONE} for c in others] == before                 # read where they lie
        # after an append on all three: the delta segment waits
        extra = batch.iloc[N_BATCH:].set_axis(range(N_RECORDS, N_RECORDS + N_EXTRA))
        names.append(extra.name, extra.id)
        addresses.append(extra.address)
        cities.append(extra.city)
        m, plain = _median_floors(names, others)
        _held(names, others, [None, m[1], m[2]], plain)
        assert len(names.master) == N_RECORDS + N_EXTRA
        assert [c.stats["segments"] for c in others] == [2, 2] and [c.stats["compactions"] for c in others] == [0, 0]
        # after a remove on all three, compact() on one of them only
        n = len(names.master)
        drop = [0, 5, 6, 700, n - N_EXTRA - 1, n - N_EXTRA, n - 3]
        for c in (names, addresses, cities):
            c.remove(drop)
        cities.compact()
        m, plain = _median_floors(names, others)
        shorter = _held(names, others, [None, m[1], m[2]], plain)
        assert set(shorter.left_id) <= set(names.master_id)
        assert addresses.stats["dead_rows"] == len(drop) and addresses.stats["compactions"] == 0 and addresses.stats["segments"] == 2
        assert addresses.stats["index_builds"] == 0 and cities.stats["index_builds"] == 0
    finally:
        for c in (names, addresses, cities):
            c.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_floors_with_candidates_from_two_fields(eng, dtype):
    master, _, _ = records()
    names, addresses, cities = _corpora(master, dtype)
    others = [addresses, cities]
    try:
        kw = dict(weights=W, candidates=CAND, candidate_fields=(0, 1), force_symmetries=False, **FINAL)
        plain = names.match_records(others, **kw)
        m, _ = _median_floors(names, others)
        before = {k: cities.stats[k] for k in LEFT_ALONE}
        for floors in ([m[0], None, None], [None, None, m[2]], m):                             # the primary's floor meets scores the union filled in
            got = names.match_records(others, field_min_similarity=floors, **kw)
            want = composed_union_route_floors(names, others, W, CAND, (0, 1), THR, TOP, floors)
            pd.testing.assert_frame_equal(got, want)
            assert (got.left_index != got.right_index).sum() >= 20 and len(plain) - len(got) >= 20
        assert {k: cities.stats[k] for k in LEFT_ALONE} == before                              # (addresses finds candidates: it is indexed)
        assert names.stats["record_floor_calls"] == 3 == names.stats["record_union_calls"] - 1
    finally:
        for c in (names, addresses, cities):
            c.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_defaults_self_matches_symmetry_and_groups_with_floors(eng, dtype):
    master, _, _ = records()
    names, addresses, cities = _corpora(master, dtype)
    others = [addresses, cities]
    try:
        m, _ = _median_floors(names, others)
        floors = [None, m[1], None]
        got = names.match_records(others, weights=W, candidates=CAND, field_min_similarity=floors, **FINAL)
        diag = got[got.left_index == got.right_index]
        assert len(diag) == N_RECORDS and (diag.similarity == 1.0).all()                       # whatever the floors say
        pairs = set(zip(got.left_index, got.right_index))
        assert pairs == {(b, a) for a, b in pairs} and len(pairs) == len(got) > N_RECORDS + 20
        unsym = composed_route_floors(names, others, W, CAND, THR, TOP, floors)
        assert pairs >= set(zip(unsym.left_index, unsym.right_index))
        none_passes = names.match_records(others, weights=W, candidates=CAND, field_min_similarity=[None, 2.0, None], **FINAL)
        assert len(none_passes) == N_RECORDS and (none_passes.left_index == none_passes.right_index).all()
        without = names.group_similar_records(others, weights=W, candidates=CAND, **FINAL)
        for rep in ("centroid", "first"):
            groups = names.group_similar_records(others, weights=W, candidates=CAND, group_rep=rep, field_min_similarity=floors, **FINAL)
            want = composed_groups_floors(names, others, W, CAND, THR, TOP, floors, group_rep=rep)
            pd.testing.assert_frame_equal(groups, want)
        assert groups.iloc[:, 0].nunique() > without.iloc[:, 0].nunique()                      # fewer pairs: more groups
    finally:
        for c in (names, addresses, cities):
            c.close()


# ------------------------------------------------------------------------------------------ field_similarities
FIELD_COLUMNS = ["similarity_0", "similarity_1", "similarity_2"]


def _columns_equal_pair_similarities(frame, lp, rp, corpora, dtype, duplicates=None):
    """Every column cast back to the dtype against ``pair_similarities`` of the rows' POSITIONS, bit for bit."""
    T = np.dtype(dtype).type
    at = list(frame.columns).index("similarity")
    assert list(frame.columns[at + 1:at + 4]) == FIELD_COLUMNS
    for k, c in enumerate(corpora):
        col = frame[f"similarity_{k}"]
        assert col.dtype == np.float64 and len(col) == len(lp)
        want = c.pair_similarities(lp, rp) if duplicates is None else c.pair_similarities(lp, rp, duplicates=duplicates[k])
        got = col.to_numpy().astype(T)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), k
        assert np.array_equal(col.to_numpy(), want.astype(np.float64)), k                       # widened, nothing else


def _recombines(frame, off, dtype):
    """For the rows ``off`` (off the diagonal), acc = acc + W[f] * similarity_f in the dtype gives ``similarity`` to the bit."""
    T = np.dtype(dtype).type
    acc = np.zeros(int(off.sum()), T)
    for f, w in enumerate(W):
        acc = acc + T(w) * frame[f"similarity_{f}"].to_numpy()[off].astype(T)
    assert acc.dtype == T and off.sum() >= 20
    assert np.array_equal(acc.astype(np.float64), frame.similarity.to_numpy()[off])


@pytest.mark.parametrize("dtype", DTYPES)
def test_field_columns_are_pair_similarities_whatever_the_index(eng, dtype):
    master, batch, _ = records()
    names, addresses, cities = _corpora(master, dtype)
    corpora, others = [names, addresses, cities], [addresses, cities]
    try:
        kw = dict(weights=W, candidates=CAND, **FINAL)
        before = [{k: c.stats[k] for k in LEFT_ALONE} for c in others]
        plain = names.match_records(others, **kw)
        got = names.match_records(others, field_similarities=True, **kw)                       # a default index; diagonal, mirror
        pd.testing.assert_frame_equal(got.drop(columns=FIELD_COLUMNS), plain)
        lp, rp = got.left_index.to_numpy(), got.right_index.to_numpy()
        _columns_equal_pair_similarities(got, lp, rp, corpora, dtype)
        _recombines(got, lp != rp, dtype)
        assert (got.similarity[lp == rp] == 1.0).all() and (lp == rp).sum() == N_RECORDS
        ignored = names.match_records(others, field_similarities=True, ignore_index=True, **kw)
        assert "left_index" not in ignored.columns and "right_index" not in ignored.columns
        pd.testing.assert_frame_equal(ignored[FIELD_COLUMNS + ["similarity"]], got[FIELD_COLUMNS + ["similarity"]])
        first = batch.iloc[:N_BATCH].reset_index(drop=True)                                    # duplicates: the forward path
        dupes = [first.name, first.address, first.city]
        pairs = names.match_records(others, duplicates=dupes, duplicates_id=first.id, field_similarities=True, weights=W,
                                    candidates=CAND, **BATCH_FINAL)
        lp, rp = pairs.left_index.to_numpy(), pairs.right_index.to_numpy()
        _columns_equal_pair_similarities(pairs, lp, rp, corpora, dtype, dupes)
        _recombines(pairs, np.ones(len(pairs), bool), dtype)
        assert [c.stats["record_field_score_calls"] for c in corpora] == [3, 3, 3]
        assert [{k: c.stats[k] for k in LEFT_ALONE} for c in others] == before                 # read where they lie
        # both options in one call, with candidates from two fields
        m, _ = _median_floors(names, others)
        floors = [None, m[1], None]
        both = names.match_records(others, field_similarities=True, field_min_similarity=floors, candidate_fields=(0, 1),
                                   force_symmetries=False, **kw)
        want = composed_union_route_floors(names, others, W, CAND, (0, 1), THR, TOP, floors)
        pd.testing.assert_frame_equal(both.drop(columns=FIELD_COLUMNS), want)
        lp, rp = both.left_index.to_numpy(), both.right_index.to_numpy()
        _columns_equal_pair_similarities(both, lp, rp, corpora, dtype)
        _recombines(both, lp != rp, dtype)
        assert (both.similarity_1.to_numpy()[lp != rp] > m[1]).all()
    finally:
        for c in corpora:
            c.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_field_columns_on_a_shuffled_string_index_with_ids_after_a_remove(eng, dtype):
    master, _, _ = records()
    order = np.random.default_rng(3).permutation(N_RECORDS)
    labels = pd.Index([f"r{k:05d}" for k in order])                                            # labels that are no positions
    master = master.set_axis(labels)
    names, addresses, cities = _corpora(master, dtype)
    corpora, others = [names, addresses, cities], [addresses, cities]
    try:
        for c in corpora:
            c.remove([1, 40, 41, N_RECORDS - 2])                                               # dead rows pending on every field
        got = names.match_records(others, field_similarities=True, weights=W, candidates=CAND, **FINAL)
        assert {"left_id", "right_id"} <= set(got.columns) and not pd.api.types.is_integer_dtype(got.left_index)
        index = pd.Index(names.master.index)
        lp, rp = index.get_indexer(got.left_index), index.get_indexer(got.right_index)
        assert (lp >= 0).all() and (rp >= 0).all() and len(index) == N_RECORDS - 4
        _columns_equal_pair_similarities(got, lp, rp, corpora, dtype)
        _recombines(got, lp != rp, dtype)
        assert [c.stats["compactions"] for c in others] == [0, 0] and [c.stats["dead_rows"] for c in others] == [4, 4]
    finally:
        for c in corpora:
            c.close()
