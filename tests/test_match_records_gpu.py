"""GPU tests of record matching: ``Corpus.match_records`` on 2 000 synthetic records of three fields against the COMPOSED ROUTE
(tests/_record_oracle.py: match_strings at the candidate options, pair_similarities a further corpus with the primary's
similarity cast back to the corpus dtype, the numpy chain, ``>``, the order by combined similarity then right position, the cut)
under ``assert_frame_equal`` -- as the corpora are fitted, meet batches on the forward and the reverse path, grow, forget and
keep a self-join --, the defaults (a record matches itself with 1, the list is symmetric), ``group_similar_records`` against
``group_similar_strings`` over the combined list, and the counters.  No tolerance anywhere."""
import functools

import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from string_grouper_amd.synth import synth_names
from tests._record_oracle import composed_groups, composed_route

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
N_RECORDS, N_BATCH, N_EXTRA = 2000, 500, 30
W = [0.5, 0.3, 0.2]
CAND = dict(min_similarity=0.6, max_n_matches=50)
FINAL = dict(min_similarity=0.8, max_n_matches=20)


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


@functools.lru_cache(maxsize=None)
def records():
    """(master frame, batch frame, agreement counts).  Names, addresses and cities are SynthNames lists of three seeds; then
    the second and third field are ARRANGED: the records are grouped by the name candidates (connected components of the
    float64 self-join at the candidate options), and a seeded coin per group and field decides whether the group's members
    share the field (the first member's value, every other member's with a number behind it) or keep their own.  A batch
    record is arranged against its best name candidate in the same way.  Needs the engine: call it inside a test."""
    rng = np.random.default_rng(77)
    name = pd.Series(synth_names(N_RECORDS, seed=51), name="name")
    fields = {"address": synth_names(N_RECORDS, seed=52, perturb_frac=0.0), "city": synth_names(N_RECORDS, seed=53, perturb_frac=0.0)}
    pairs = sga.match_strings(name, tfidf_matrix_dtype=np.float64, force_symmetries=False, **CAND)
    pairs = pairs[pairs.left_index != pairs.right_index]
    root = np.arange(N_RECORDS)

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    for a, b in zip(pairs.left_index.to_numpy(), pairs.right_index.to_numpy()):
        ra, rb = find(int(a)), find(int(b))
        root[max(ra, rb)] = min(ra, rb)
    group = np.array([find(i) for i in range(N_RECORDS)])
    agree = {}
    for f, values in fields.items():
        shared = rng.random(N_RECORDS) < 0.5                                   # the coin of the group whose first member is i
        for i in range(N_RECORDS):
            if group[i] != i and shared[group[i]]:
                values[i] = f"{values[group[i]]} {1 + i % 9}"
        li, ri = pairs.left_index.to_numpy(), pairs.right_index.to_numpy()
        agree[f] = (int(np.count_nonzero(shared[group[li]])), len(pairs))
    master = pd.DataFrame({"name": name, "address": fields["address"], "city": fields["city"],
                           "id": [f"R{i:05d}" for i in range(N_RECORDS)]})
    # the batch: perturbed names of the master list; a record shares a field with the master record its name is drawn near
    n_batch = N_BATCH + N_EXTRA
    b_name = pd.Series(synth_names(n_batch, seed=54, perturb_of=list(name), perturb_frac=0.6), name="name")
    b_fields = {"address": synth_names(n_batch, seed=55, perturb_frac=0.0), "city": synth_names(n_batch, seed=56, perturb_frac=0.0)}
    near = sga.match_strings(name, b_name, tfidf_matrix_dtype=np.float64, **CAND)
    best = near.sort_values(["right_index", "similarity", "left_index"], ascending=[True, False, True]).drop_duplicates("right_index")
    for f, values in b_fields.items():
        coin = rng.random(n_batch) < 0.5
        for d, m in zip(best.right_index.to_numpy(), best.left_index.to_numpy()):
            if coin[d]:
                values[d] = f"{master[f][m]} {1 + d % 9}"
    batch = pd.DataFrame({"name": b_name, "address": b_fields["address"], "city": b_fields["city"],
                          "id": [f"B{i:05d}" for i in range(n_batch)]})
    return master, batch, agree


def _corpora(master, dtype):
    kw = dict(tfidf_matrix_dtype=dtype)
    return (sga.Corpus(master.name, master_id=master.id, **kw), sga.Corpus(master.address, **kw), sga.Corpus(master.city, **kw))


def _held(names, others, duplicates=None, duplicates_id=None, min_rows=20):
    """match_records against the composed route, exactly; returns the frame."""
    got = names.match_records(others, duplicates=duplicates, duplicates_id=duplicates_id, weights=W, candidates=CAND,
                              force_symmetries=False, **FINAL)
    want = composed_route(names, others, W, CAND, FINAL["min_similarity"], FINAL["max_n_matches"], duplicates, duplicates_id)
    pd.testing.assert_frame_equal(got, want)
    assert len(got) >= min_rows
    return got


def test_about_half_of_the_name_candidates_agree_on_the_further_fields(eng):
    master, batch, agree = records()
    for f, (shared, n_pairs) in agree.items():
        assert n_pairs > 1000 and 0.3 * n_pairs < shared < 0.7 * n_pairs, (f, shared, n_pairs)
    assert len(master) == N_RECORDS and len(batch) == N_BATCH + N_EXTRA


@pytest.mark.parametrize("dtype", DTYPES)
def test_match_records_equals_the_composed_route_as_the_corpora_live(eng, dtype):
    master, batch, _ = records()
    names, addresses, cities = _corpora(master, dtype)
    others = [addresses, cities]
    try:
        before = [c.stats for c in (names, addresses, cities)]
        self_join = _held(names, others, min_rows=N_RECORDS)                                   # the self-join
        cand = names.match_strings(names.master, master_id=names.master_id, force_symmetries=False, **CAND)
        off = self_join[self_join.left_index != self_join.right_index]
        assert 100 < len(off) < 0.8 * np.count_nonzero(cand.left_index != cand.right_index)     # the fields decided
        first = batch.iloc[:N_BATCH].reset_index(drop=True)
        forward = names.stats["forward"]
        _held(names, others, [first.name, first.address, first.city], first.id)                # corpus x 500: forward path
        assert names.stats["forward"] == forward + 2                                           # (the call and the composed route's)
        few = batch.iloc[:20].reset_index(drop=True)
        reverse = names.stats["reverse"]
        _held(names, others, [few.name, few.address, few.city], few.id, min_rows=3)            # corpus x 20: reverse path
        assert names.stats["reverse"] == reverse + 2
        # counters: the further corpora are read where they lie
        for c, b in zip((names, addresses, cities), before):
            st = c.stats
            assert st["record_calls"] == b["record_calls"] + 3
            assert st["compactions"] == b["compactions"] == 0 and st["tokenisations"] == 1
        assert addresses.stats["index_builds"] == 0 and cities.stats["index_builds"] == 0       # no index of a further field
        assert addresses.stats["transforms"] == 2 + 2 and names.stats["transforms"] == 2 + 2    # one a field and call (+ composed)
        # after append on all three: the delta segment waits
        extra = batch.iloc[N_BATCH:].set_axis(range(N_RECORDS, N_RECORDS + N_EXTRA))          # (labels stay unique: the frames name rows by label)
        names.append(extra.name, extra.id)
        addresses.append(extra.address)
        cities.append(extra.city)
        assert [c.stats["segments"] for c in (names, addresses, cities)] == [2, 2, 2]
        grown = _held(names, others, min_rows=N_RECORDS + N_EXTRA)
        assert grown.left_index.max() >= N_RECORDS
        _held(names, others, [few.name, few.address, few.city], few.id, min_rows=3)
        assert [c.stats["segments"] for c in (addresses, cities)] == [2, 2] and addresses.stats["compactions"] == 0
        # after remove on all three, compact() on one of them only
        n = len(names.master)
        drop = [0, 5, 6, 700, n - N_EXTRA - 1, n - N_EXTRA, n - 3]
        for c in (names, addresses, cities):
            c.remove(drop)
        cities.compact()
        assert addresses.stats["dead_rows"] == len(drop) and cities.stats["dead_rows"] == 0
        _held(names, others, [few.name, few.address, few.city], few.id, min_rows=3)            # (dead rows on the left side only)
        assert names.stats["dead_rows"] == len(drop)
        shorter = _held(names, others, min_rows=n - len(drop))                                 # (a self-join compacts ITS corpus)
        assert addresses.stats["dead_rows"] == len(drop) and addresses.stats["compactions"] == 0 and addresses.stats["segments"] == 2
        assert set(shorter.left_id) == set(names.master_id)
        # with a kept self-join at the candidate options
        names.keep_self_join(**CAND)
        served = names.stats["self_join_served"]
        kept = _held(names, others, min_rows=n - len(drop))
        assert names.stats["self_join_served"] == served + 2 and names.stats["self_join_full"] == 1
        pd.testing.assert_frame_equal(kept, shorter)
    finally:
        for c in (names, addresses, cities):
            c.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_defaults_a_record_matches_itself_with_1_and_the_list_is_symmetric(eng, dtype):
    master, _, _ = records()
    names, addresses, cities = _corpora(master, dtype)
    try:
        got = names.match_records([addresses, cities], weights=W, candidates=CAND, **FINAL)
        diag = got[got.left_index == got.right_index]
        assert len(diag) == N_RECORDS and (diag.similarity == 1.0).all()
        pairs = set(zip(got.left_index, got.right_index))
        assert pairs == {(b, a) for a, b in pairs} and len(pairs) == len(got) > N_RECORDS + 100
        unsym = composed_route(names, [addresses, cities], W, CAND, FINAL["min_similarity"], FINAL["max_n_matches"])
        assert pairs >= set(zip(unsym.left_index, unsym.right_index))
        # duplicates whose first Series is corpus.master itself are still duplicates: the fields GIVEN are the ones scored
        turned = [names.master, master.address[::-1].reset_index(drop=True), master.city[::-1].reset_index(drop=True)]
        other = _held(names, [addresses, cities], turned, names.master_id, min_rows=0)
        assert len(other) < len(unsym) and addresses.stats["transforms"] == 2            # (the call and the composed route's)
        # group_similar_records: group_similar_strings fed with the combined list
        for rep in ("centroid", "first"):
            groups = names.group_similar_records([addresses, cities], weights=W, candidates=CAND, group_rep=rep, **FINAL)
            want = composed_groups(names, [addresses, cities], W, CAND, FINAL["min_similarity"], FINAL["max_n_matches"], group_rep=rep)
            pd.testing.assert_frame_equal(groups, want)
            assert 100 < groups.iloc[:, 0].nunique() < N_RECORDS
        # the module-level function fits the same corpora, calls and closes them
        live = N_live_handles()
        frame = sga.match_records([master.name, master.address, master.city], master_id=master.id, weights=W, candidates=CAND,
                                  tfidf_matrix_dtype=dtype, **FINAL)
        pd.testing.assert_frame_equal(frame, got)
        assert N_live_handles() == live
    finally:
        for c in (names, addresses, cities):
            c.close()


def N_live_handles():
    from string_grouper_amd import _native as N
    return N.live_handles()


def test_the_multi_gpu_engine_refuses():
    with pytest.raises(NotImplementedError, match="single-GPU"):
        E.DistributedHipEngine.corpus_records(None)
