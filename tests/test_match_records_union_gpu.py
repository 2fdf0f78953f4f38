"""GPU tests of ``candidate_fields``: ``Corpus.match_records`` with candidates from two and three fields on the 2 000 synthetic
records of tests/test_match_records_gpu.py against the COMPOSED UNION ROUTE (tests/_record_union_oracle.py: match_strings a
candidate field, the union of the position pairs in pandas, pair_similarities on every field, the numpy chain, ``>``, the order,
the cut) under ``assert_frame_equal`` -- as the corpora are fitted, meet batches on the forward and the reverse path, grow,
forget and keep a self-join --, ``group_similar_records`` against the composed groups, the counters of a corpus that is no
candidate field, and the pair that only an address finds.  No tolerance anywhere."""
import pandas as pd
import pytest

import string_grouper_amd as sga
from tests._record_union_oracle import composed_union_groups, composed_union_route
from tests.test_match_records_gpu import CAND, DTYPES, FINAL, N_BATCH, N_EXTRA, N_RECORDS, W, _corpora, eng, records  # noqa: F401
from tests.test_match_records_union_cpu import ONLY_ADDRESS, ONLY_CITY, ONLY_NAMES

pytestmark = pytest.mark.gpu
UNTOUCHED = ("dead_rows", "segments", "compactions", "index_builds")


def _held(names, others, fields, duplicates=None, duplicates_id=None, min_rows=20, watch=None):
    """match_records against the composed union route, exactly; returns the frame.  ``watch``: a corpus that is no candidate
    field -- the call leaves it where it lies."""
    before = None if watch is None else watch.stats
    calls = [c.stats["record_union_calls"] for c in [names] + list(others)]
    got = names.match_records(others, duplicates=duplicates, duplicates_id=duplicates_id, weights=W, candidates=CAND,
                              candidate_fields=fields, force_symmetries=False, **FINAL)
    if watch is not None:
        assert [watch.stats[k] for k in UNTOUCHED] == [before[k] for k in UNTOUCHED]
    assert [c.stats["record_union_calls"] - b for c, b in zip([names] + list(others), calls)] == [int(f in fields) for f in range(3)]
    want = composed_union_route(names, others, W, CAND, fields, FINAL["min_similarity"], FINAL["max_n_matches"], duplicates,
                                duplicates_id)
    pd.testing.assert_frame_equal(got, want)
    assert len(got) >= min_rows
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_match_records_equals_the_composed_union_route_as_the_corpora_live(eng, dtype):  # noqa: F811
    master, batch, _ = records()
    names, addresses, cities = _corpora(master, dtype)
    others = [addresses, cities]
    try:
        two = _held(names, others, (0, 1), min_rows=N_RECORDS, watch=cities)                   # the self-join
        assert cities.stats["index_builds"] == 0 and addresses.stats["index_builds"] >= 1       # a candidate field has its index
        _held(names, others, (0, 1, 2), min_rows=len(two))
        first = batch.iloc[:N_BATCH].reset_index(drop=True)
        forward = [c.stats["forward"] for c in (names, addresses)]
        _held(names, others, (0, 1), [first.name, first.address, first.city], first.id)        # corpus x 500: forward path
        assert [c.stats["forward"] for c in (names, addresses)] == [f + 2 for f in forward]    # (the call and the composed route's)
        few = batch.iloc[:20].reset_index(drop=True)
        reverse = [c.stats["reverse"] for c in (names, addresses, cities)]
        _held(names, others, (0, 1, 2), [few.name, few.address, few.city], few.id, min_rows=3)  # corpus x 20: reverse path
        assert [c.stats["reverse"] for c in (names, addresses, cities)] == [r + 2 for r in reverse]
        # after append on all three: the delta segment waits
        extra = batch.iloc[N_BATCH:].set_axis(range(N_RECORDS, N_RECORDS + N_EXTRA))
        names.append(extra.name, extra.id)
        addresses.append(extra.address)
        cities.append(extra.city)
        grown = _held(names, others, (0, 1), min_rows=N_RECORDS + N_EXTRA, watch=cities)
        assert grown.left_index.max() >= N_RECORDS and cities.stats["segments"] == 2
        _held(names, others, (0, 1), [few.name, few.address, few.city], few.id, min_rows=3, watch=cities)
        # after remove on all three: the corpus that is no candidate field keeps its dead rows, the candidate fields' self-joins
        # compact their own
        n = len(names.master)
        drop = [0, 5, 6, 700, n - N_EXTRA - 1, n - N_EXTRA, n - 3]
        for c in (names, addresses, cities):
            c.remove(drop)
        _held(names, others, (0, 1), [few.name, few.address, few.city], few.id, min_rows=3, watch=cities)   # dead rows on the left
        assert [c.stats["dead_rows"] for c in (names, addresses, cities)] == [len(drop)] * 3
        shorter = _held(names, others, (0, 1), min_rows=n - len(drop), watch=cities)
        assert cities.stats["dead_rows"] == len(drop) and cities.stats["segments"] == 2 and cities.stats["compactions"] == 0
        assert names.stats["dead_rows"] == 0 and addresses.stats["dead_rows"] == 0 and set(shorter.left_id) == set(names.master_id)
        # with a kept self-join on the primary at the candidate options
        names.keep_self_join(**CAND)
        served = names.stats["self_join_served"]
        kept = _held(names, others, (0, 1), min_rows=n - len(drop), watch=cities)
        assert names.stats["self_join_served"] == served + 2 and names.stats["self_join_full"] == 1
        pd.testing.assert_frame_equal(kept, shorter)
    finally:
        for c in (names, addresses, cities):
            c.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_groups_and_the_pair_that_only_an_address_finds(eng, dtype):  # noqa: F811
    master, _, _ = records()
    names, addresses, cities = _corpora(master, dtype)
    try:
        groups = names.group_similar_records([addresses, cities], weights=W, candidates=CAND, candidate_fields=(0, 1), **FINAL)
        want = composed_union_groups(names, [addresses, cities], W, CAND, (0, 1), FINAL["min_similarity"], FINAL["max_n_matches"])
        pd.testing.assert_frame_equal(groups, want)
        assert 100 < groups.iloc[:, 0].nunique() < N_RECORDS
    finally:
        for c in (names, addresses, cities):
            c.close()
    kw = dict(weights=[0.5, 0.25, 0.25], candidates=dict(min_similarity=0.5, max_n_matches=4), min_similarity=0.3,
              force_symmetries=False, tfidf_matrix_dtype=dtype)
    default = sga.match_records([ONLY_NAMES, ONLY_ADDRESS, ONLY_CITY], **kw)
    assert (0, 1) not in set(zip(default.left_index, default.right_index))
    for fields in ((0, 1), (0, 1, 2)):
        got = sga.match_records([ONLY_NAMES, ONLY_ADDRESS, ONLY_CITY], candidate_fields=fields, **kw)
        pairs = set(zip(got.left_index, got.right_index))
        assert (0, 1) in pairs and (1, 0) in pairs and len(got) == len(default) + 2
        assert got[(got.left_index == 0) & (got.right_index == 1)].similarity.iloc[0] > 0.49
