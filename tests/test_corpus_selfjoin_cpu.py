"""CPU tests of a self-join that a corpus keeps (Corpus.keep_self_join): the numpy / scipy restatement of the two updates
(tests/_corpus_selfjoin_cases.py) against the port's whole self-join after every step, on random inputs and on inputs built
to bite; and the host logic of ``Corpus`` on the engine double that keeps one.  Every comparison is exact.  No GPU."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from tests import _corpus_selfjoin_cases as K
from tests._corpus_remove_oracle import RemoveCorpusOracleEngine
from tests.test_corpus_cpu import CORPUS, NEW, _expected

DTYPES = [np.float32, np.float64]


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


def _same(got, want):
    (pd.testing.assert_frame_equal if isinstance(got, pd.DataFrame) else pd.testing.assert_series_equal)(got, want)
    assert len(got) > 0


def _assert_current(kept, what):
    want = kept.whole()
    bad = K.differing_rows(kept.rows, want)
    assert not bad, f"{what}: rows {sorted(bad)[:10]} differ from the whole self-join"
    assert K.same_rows(kept.rows, want), what


# ------------------------------------------------------------------------------------------ the restatement, random inputs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("top_n, threshold", [(1, 0.5), (3, 0.3), (5, 0.0), (10, 0.7), (200, 0.2)])
def test_random_appends_and_removes_keep_the_restatement_equal_to_the_port(dtype, top_n, threshold):
    rng = np.random.default_rng(1000 * top_n + int(10 * threshold))
    m, pool = K.random_rows(rng, 60, 40, dtype)
    kept = K.KeptSelfJoin(m, top_n, threshold)
    _assert_current(kept, "first multiply")
    refilled = 0
    for step in range(14):
        n = kept.M.shape[0]
        if step % 3 == 2 or n < 8:
            new, _ = K.random_rows(rng, int(rng.integers(1, 12)), 40, dtype, pool)
            if step % 2:
                new = sp.vstack([new, sp.csr_matrix((1, 40), dtype=dtype)], format="csr", dtype=dtype)   # a row without entries
            kept.append(new)
            _assert_current(kept, f"step {step}: append {new.shape[0]}")
        else:
            dead = rng.choice(n, int(rng.integers(1, max(n // 4, 2))), replace=False)
            refilled += len(kept.remove(dead))
            _assert_current(kept, f"step {step}: remove {sorted(dead.tolist())}")
    if top_n <= 5:
        assert refilled > 0, "no remove of this run cut a full row: the run shows nothing about the refill"


# ------------------------------------------------------------------------------------------ the restatement, built inputs
def _members(groups, g):
    return np.flatnonzero(groups == g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_built_corpus_holds_what_it_is_built_for(dtype):
    m, groups = K.built_corpus(dtype)
    rows = K.product(m, m, K.BUILT_TOP_N, 0.8)
    hub = _members(groups, K.HUB)
    assert len(hub) == 40
    for i in hub:                                                     # every hub row names the ten lowest members, all ties
        assert list(rows[i][0]) == list(hub[:10]) and len(set(rows[i][1].tolist())) == 1
    assert all(len(rows[i][0]) == K.BUILT_TOP_N for i in _members(groups, K.FULL))          # exactly full: nothing was cut
    assert all(len(rows[i][0]) == K.BUILT_TOP_N - 1 for i in _members(groups, K.ONE_SHORT))  # one short
    assert len(rows[-1][0]) == 0                                      # the row without entries matches nothing


@pytest.mark.parametrize("dtype", DTYPES)
def test_removing_the_lowest_hub_members_refills_the_hub_and_nothing_else(dtype):
    m, groups = K.built_corpus(dtype)
    hub = _members(groups, K.HUB)
    dead = hub[:8]
    kept = K.KeptSelfJoin(m, K.BUILT_TOP_N, 0.8)
    before = kept.rows
    which = kept.remove(dead)
    _assert_current(kept, "hub: the eight lowest removed")
    live_hub = np.flatnonzero(np.delete(groups, dead) == K.HUB)
    assert sorted(which.tolist()) == sorted(live_hub.tolist()) and len(which) == 32
    # the inputs bite: without the refill the hub's rows come back short
    mutant = K.KeptSelfJoin(m, K.BUILT_TOP_N, 0.8, refill="none")
    mutant.remove(dead)
    assert K.differing_rows(mutant.rows, kept.whole()) == set(live_hub.tolist())
    assert all(len(mutant.rows[i][0]) == 2 for i in live_hub)         # the two survivors of the ten lowest
    # the refill set is the rows that changed beyond deletion, plus the full rows that named a removed column
    deleted_only, _ = K.forget(before, dead, K.BUILT_TOP_N)
    changed = K.differing_rows(deleted_only, kept.whole())
    keep = np.setdiff1d(np.arange(m.shape[0]), dead)
    full_and_named = {k for k, i in enumerate(keep) if len(before[i][0]) == K.BUILT_TOP_N and np.isin(before[i][0], dead).any()}
    assert set(which.tolist()) == changed | full_and_named and changed


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("group, n_refilled", [(K.FULL, 9), (K.ONE_SHORT, 0)])
def test_a_row_that_was_exactly_full_is_refilled_and_one_that_was_short_is_not(dtype, group, n_refilled):
    """A full row that loses an entry may hide a candidate, so it is multiplied again (here it hides none: the result does
    not change beyond the deletion); a row one short held every pair above the threshold and is left alone."""
    m, groups = K.built_corpus(dtype)
    dead = _members(groups, group)[:1]
    kept = K.KeptSelfJoin(m, K.BUILT_TOP_N, 0.8)
    before = kept.rows
    which = kept.remove(dead)
    _assert_current(kept, f"group {group}")
    assert len(which) == n_refilled
    deleted_only, short = K.forget(before, dead, K.BUILT_TOP_N)
    assert K.same_rows(deleted_only, kept.whole()) and len(short) == n_refilled
    # refilling every row that lost an entry is right as well, and never less work
    losers = K.KeptSelfJoin(m, K.BUILT_TOP_N, 0.8, refill="losers")
    more = losers.remove(dead)
    _assert_current(losers, f"group {group}, every loser")
    assert set(which.tolist()) <= set(more.tolist()) and len(more) == len(_members(groups, group)) - 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_scores_across_the_boundary_of_old_and_new_rows(dtype):
    """Copies of a group's row are appended: their scores tie with the old members', and the new columns, which carry the
    highest numbers, come last among equals -- in the hub they are cut, in the group that was one short one of them fills the
    row and the next is cut, and every NEW row names the lowest old members."""
    m, groups = K.built_corpus(dtype)
    kept = K.KeptSelfJoin(m, K.BUILT_TOP_N, 0.8)
    n_old = m.shape[0]
    new = K.unit_rows([K.HUB, K.ONE_SHORT, K.ONE_SHORT, 9, K.FULL], K.BUILT_COLS, dtype)
    kept.append(new)
    _assert_current(kept, "copies appended")
    hub, short = _members(groups, K.HUB), _members(groups, K.ONE_SHORT)
    assert list(kept.rows[hub[5]][0]) == list(hub[:10])               # the new copy is cut
    assert list(kept.rows[short[0]][0]) == list(short) + [n_old + 1]  # the first new copy fills the row, the second is cut
    assert list(kept.rows[n_old][0]) == list(hub[:10])                # a new row names old columns only
    assert list(kept.rows[n_old + 3][0]) == [n_old + 3]               # a new row that matches itself alone
    # a score between the ties: rows near the hub's, below its members and above the threshold
    kept.append(K.near_rows([K.HUB, K.HUB], K.BUILT_COLS, dtype, tilt=1.0))
    _assert_current(kept, "near rows appended")
    # ... and the remove that makes the boundary matter: the hub's ten lowest go, new copies move up
    which = kept.remove(hub[:33])
    _assert_current(kept, "most of the hub removed")
    assert len(which) > 0
    mutant = K.KeptSelfJoin(m, K.BUILT_TOP_N, 0.8, refill="none")
    mutant.append(new)
    mutant.remove(hub[:8])
    assert K.differing_rows(mutant.rows, mutant.whole())


@pytest.mark.parametrize("dtype", DTYPES)
def test_remove_append_remove_and_corner_sizes(dtype):
    m, groups = K.built_corpus(dtype)
    hub = _members(groups, K.HUB)
    for top_n in (1, 10, 100):                                        # 100: more than the corpus has rows
        kept = K.KeptSelfJoin(m, top_n, 0.8)
        kept.remove(hub[:3])
        _assert_current(kept, f"top {top_n}: remove")
        kept.append(K.unit_rows([K.HUB] * 5 + [11], K.BUILT_COLS, dtype))
        _assert_current(kept, f"top {top_n}: append")
        kept.remove([0, 1, kept.M.shape[0] - 1, kept.M.shape[0] - 3])
        _assert_current(kept, f"top {top_n}: remove old and new rows")
        kept.remove(np.arange(1, kept.M.shape[0]))                   # all but one row
        _assert_current(kept, f"top {top_n}: one row left")
        assert len(kept.rows) == 1
    assert sum(len(w) for w in K.KeptSelfJoin(m, 100, 0.8).refilled) == 0


def test_the_restated_operations_on_small_hand_made_rows():
    f = np.float32
    a = [(np.array([3, 1], np.int32), np.array([0.9, 0.5], f)), (np.array([], np.int32), np.array([], f))]
    b = [(np.array([0], np.int32), np.array([0.9], f)), (np.array([1, 0], np.int32), np.array([0.7, 0.7], f))]
    z = K.zip_rows([a, b], [0, 4], 3)
    assert list(z[0][0]) == [3, 4, 1] and list(z[0][1]) == [f(0.9), f(0.9), f(0.5)]      # equal scores: the lower column first
    assert list(z[1][0]) == [4, 5]
    assert list(K.zip_rows([a, b], [0, 4], 1)[0][0]) == [3]
    rows = K.concat_rows([a, [], b])
    assert len(rows) == 4 and rows[2] is b[0]
    square = [(np.array([0, 2, 3], np.int32), np.array([1, .9, .8], f)), (np.array([1], np.int32), np.array([1], f)),
              (np.array([2, 0], np.int32), np.array([1, .9], f)), (np.array([3, 1, 0], np.int32), np.array([1, .9, .8], f))]
    left, short = K.forget(square, [1], 3)
    assert [list(c) for c, _ in left] == [[0, 1, 2], [1, 0], [2, 0]] and list(short) == [2]
    left, short = K.forget(square, [0, 3], 2)
    assert [list(c) for c, _ in left] == [[0], [1]] and list(short) == [1]                # row 1 held one entry; row 2 was full at 2 and lost one
    put = K.put_rows(square, [3, 0], b)
    assert put[3] is b[0] and put[0] is b[1] and put[1] is square[1]


# ------------------------------------------------------------------------------------------ Corpus on the engine double
def _corpus(**kwargs):
    E.set_engine(K.SelfJoinCorpusOracleEngine(use_port=True))
    return sga.Corpus(CORPUS, **kwargs)


def test_keep_self_join_checks_its_options():
    corpus = _corpus(min_similarity=0.3)
    for bad in (dict(ngram_size=2), dict(group_rep="first"), dict(n_blocks=(1, 1)), dict(top_n=3)):
        with pytest.raises(TypeError):
            corpus.keep_self_join(**bad)
    with pytest.raises(ValueError, match="max_n_matches=None"):
        corpus.keep_self_join(max_n_matches=None)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            corpus.keep_self_join(max_n_matches=bad)
    assert corpus._state.kept_opts is None
    corpus.keep_self_join()
    assert corpus._state.kept_opts == (20, 0.3)                       # the corpus's own options
    corpus.keep_self_join(min_similarity=0.5, max_n_matches=3)
    assert corpus._state.kept_opts == (3, 0.5)
    corpus.close()
    with pytest.raises(ValueError, match="closed"):
        corpus.keep_self_join()
    E.set_engine(RemoveCorpusOracleEngine(use_port=True))
    with pytest.raises(NotImplementedError, match="keeps no self-join"):
        sga.Corpus(CORPUS).keep_self_join()
    sga.Corpus(CORPUS).drop_self_join()                               # nothing kept: nothing to do


def test_which_calls_are_served_and_what_the_counters_say():
    corpus = _corpus(min_similarity=0.3)
    never = dict(corpus.stats)
    assert all(never[k] == 0 for k in never if k.startswith("self_join_"))
    corpus.group_similar_strings(corpus.master)
    assert corpus.stats["self_join_served"] == 0 and corpus.stats["self_join_full"] == 0      # nothing kept, nothing served
    corpus.keep_self_join()
    assert corpus.stats["self_join_full"] == 0                        # computed on first need
    kw = dict(min_similarity=0.3)
    served = 0
    for call, want in [
        (lambda m: corpus.group_similar_strings(m), lambda m: _expected(CORPUS, "group_similar_strings", m, **kw)),
        (lambda m: corpus.group_similar_strings(m, group_rep="first"),
         lambda m: _expected(CORPUS, "group_similar_strings", m, group_rep="first", **kw)),
        (lambda m: corpus.match_strings(m), lambda m: _expected(CORPUS, "match_strings", m, **kw)),
        (lambda m: corpus.match_strings(m, force_symmetries=False, ignore_index=True),
         lambda m: _expected(CORPUS, "match_strings", m, force_symmetries=False, ignore_index=True, **kw)),
        (lambda m: corpus.match_strings(m, max_n_matches=20, min_similarity=0.3), lambda m: _expected(CORPUS, "match_strings", m, **kw)),
    ]:
        got = call(corpus.master)
        served += 1
        assert corpus.stats["self_join_served"] == served and corpus.stats["self_join_full"] == 1
        _same(got, want(CORPUS))
    # not served, and the kept result stays: other values, another Series, duplicates, an equal copy of the master
    for call in (lambda: corpus.match_strings(corpus.master, max_n_matches=2), lambda: corpus.match_strings(corpus.master, min_similarity=0.5),
                 lambda: corpus.match_strings(NEW), lambda: corpus.match_strings(corpus.master, NEW),
                 lambda: corpus.match_strings(NEW, corpus.master), lambda: corpus.match_strings(corpus.master.copy()),
                 lambda: corpus.match_most_similar(corpus.master, NEW)):
        call()
    st = corpus.stats
    assert st["self_join_served"] == served and st["self_join_full"] == 1 and corpus._state.kept is not None
    pd.testing.assert_frame_equal(corpus.match_strings(corpus.master, max_n_matches=2),
                                  _expected(CORPUS, "match_strings", CORPUS, max_n_matches=2, **kw))


def test_the_kept_result_follows_appends_and_removes_and_is_served():
    corpus = _corpus(min_similarity=0.3, max_n_matches=2)
    corpus.keep_self_join()
    left = CORPUS
    corpus.append(pd.Series(["Acme Corp", "Hooli Incorporated"], name="company"))     # nothing kept yet: nothing to update
    left = pd.concat([left, pd.Series(["Acme Corp", "Hooli Incorporated"], name="company")])
    assert corpus.stats["self_join_append_updates"] == 0
    kw = dict(min_similarity=0.3, max_n_matches=2)
    _same(corpus.group_similar_strings(corpus.master), _expected(CORPUS, "group_similar_strings", left, **kw))
    for step, change in enumerate([("append", ["Globex", "ACME CORPORATION", "zzqqxx"]), ("remove", [0, 1]), ("append", ["Acme Corp"]),
                                   ("remove", [2, -1]), ("remove", [5])]):
        if change[0] == "append":
            new = pd.Series(change[1], name="company")
            corpus.append(new)
            left = pd.concat([left, new])
        else:
            corpus.remove(change[1])
            keep = np.ones(len(left), bool)
            keep[change[1]] = False
            left = left[keep]
        pd.testing.assert_series_equal(corpus.master, left)
        pd.testing.assert_frame_equal(corpus.match_strings(corpus.master), _expected(CORPUS, "match_strings", left, **kw))
        _same(corpus.group_similar_strings(corpus.master), _expected(CORPUS, "group_similar_strings", left, **kw))
        old = corpus.master
    st = corpus.stats
    assert st["self_join_full"] == 1 and st["self_join_append_updates"] == 2 and st["self_join_remove_updates"] == 3
    assert st["self_join_served"] == 11 and st["self_join_rows_refilled"] > 0
    # an older master is a Series like any other: transformed, not served
    corpus.append(pd.Series(["Soylent"], name="company"))
    corpus.match_strings(old)
    assert corpus.stats["self_join_served"] == 11
    # other values replace the kept result; the same values keep it; drop_self_join ends it; close frees it
    corpus.keep_self_join()
    assert corpus._state.kept is not None
    corpus.keep_self_join(max_n_matches=3)
    assert corpus._state.kept is None and corpus._state.kept_opts == (3, 0.3)
    corpus.match_strings(corpus.master, max_n_matches=3)
    assert corpus.stats["self_join_full"] == 2 and corpus.stats["self_join_served"] == 12
    corpus.drop_self_join()
    corpus.match_strings(corpus.master, max_n_matches=3)
    assert corpus.stats["self_join_served"] == 12 and corpus._state.kept_opts is None
    corpus.keep_self_join(max_n_matches=3)
    corpus.match_strings(corpus.master, max_n_matches=3)
    state = corpus._state
    assert state.kept is not None
    corpus.close()
    assert state.kept is None and state.kept_opts is None


def test_the_hip_engine_s_bookkeeping_of_a_kept_result_without_a_device():
    """corpus_keep_self_join / corpus_drop_self_join only note the options; nothing is multiplied before a call needs it."""
    state = E.CorpusState.__new__(E.CorpusState)
    state.kept, state.kept_opts = None, None
    eng = E.HipEngine.__new__(E.HipEngine)
    eng.corpus_keep_self_join(state, np.int64(20), np.float32(0.5))
    assert state.kept_opts == (20, 0.5) and type(state.kept_opts[0]) is int and type(state.kept_opts[1]) is float

    class Handle:
        freed = 0

        def free(self):
            Handle.freed += 1
    state.kept = Handle()
    eng.corpus_keep_self_join(state, 20, 0.5)                         # the same values: kept
    assert Handle.freed == 0 and state.kept is not None
    eng.corpus_keep_self_join(state, 10, 0.5)                         # other values: replaced
    assert Handle.freed == 1 and state.kept is None and state.kept_opts == (10, 0.5)
    state.kept = Handle()
    eng.corpus_drop_self_join(state)
    assert Handle.freed == 2 and state.kept is None and state.kept_opts is None
