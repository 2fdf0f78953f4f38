"""One session of a living corpus on the device, counted: after every public call the handles alive (``_native.live_handles``)
are exactly the ones the corpus's state and its vectoriser list, and ``close()`` leaves none -- without waiting for the
collector.  The self-joins of the session are compared with the fixed-vocabulary oracle (tests/_corpus_refit_oracle.py), so that
the count is not one over wrong results."""
import gc

import numpy as np
import pandas as pd
import pytest

import string_grouper_amd as sga
import string_grouper_amd._native as N
import string_grouper_amd.engine as E
from string_grouper_amd.synth import synth_names
from tests import _corpus_refit_oracle as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


def test_a_corpus_session_holds_the_handles_its_state_lists_and_close_leaves_none(eng, monkeypatch):
    base = list(synth_names(2000, seed=41))
    more = list(synth_names(400, seed=42, perturb_of=base[:400], perturb_frac=0.5))
    kw = dict(min_similarity=0.8, tfidf_matrix_dtype=np.float32)
    gc.collect()
    baseline = N.live_handles()

    def counted(what):
        state = cp._state
        listed = len(state.handles()) + len(state.vec.handles())
        assert N.live_handles() - baseline == listed, f"after {what}: {N.live_handles() - baseline} alive, {listed} listed"

    def same(got, current, what):
        want = R.expected_after_refit(base, list(current), "match_strings", current, **kw)
        pd.testing.assert_frame_equal(got, want)
        assert len(got) > len(current), what                          # more than the diagonal

    cp = sga.Corpus(pd.Series(base, name="name"), **kw)
    counted("the build")
    cp.keep_self_join()
    counted("keep_self_join")
    same(cp.match_strings(cp.master), cp.master, "the first self-join")
    counted("the first self-join")
    assert cp.stats["self_join_full"] == 1 and cp._state.kept is not None

    appended = 0
    while cp.stats["compactions"] == 0:                               # the delta crosses its share of the base once
        cp.append(pd.Series(more[appended:appended + 10], name="name"))
        appended += 10
        counted(f"the append of rows {appended - 10}..{appended}")
    assert appended == 10 * (int(2000 * eng.CORPUS_COMPACT_SHARE) // 10 + 1) and cp.stats["segments"] == 1
    assert cp.stats["self_join_append_updates"] == appended // 10

    one = pd.Series([more[-1]])
    for reverse, path in (("1", "reverse"), ("0", "forward")):
        monkeypatch.setenv("SG_CORPUS_REVERSE", reverse)
        before = cp.stats[path]
        cp.match_strings(cp.master, one)
        assert cp.stats[path] == before + 1
        counted(f"a one-row query, {path}")
    monkeypatch.delenv("SG_CORPUS_REVERSE", raising=False)

    removed = 0
    while cp.stats["compactions"] == 1:                               # the dead rows cross their cap once
        cp.remove([3 + removed, 500, 900, 1500, len(cp.master) - 1])
        removed += 5
        counted(f"the remove of {removed} rows")
    assert removed == 5 * (eng.CORPUS_MAX_DEAD // 5 + 1) and cp.stats["dead_rows"] == 0
    assert cp.stats["self_join_remove_updates"] == removed // 5 and cp.stats["self_join_full"] == 1

    cp.refit_idf()
    counted("refit_idf")
    assert cp._state.kept is None and cp.stats["idf_refits"] == 1
    current = cp.master
    assert len(current) == 2000 + appended - removed
    same(cp.match_strings(current), current, "the self-join after the refit")
    counted("the last self-join")
    assert cp.stats["self_join_full"] == 2 and cp.stats["tokenisations"] == 1

    cp.close()
    assert N.live_handles() == baseline
