"""Who frees what in the resident-corpus code (string_grouper_amd/corpus_engine.py) and in the blocked multiplies of the engine:
every path, the failing ones included, on a fake context whose handles record ``free()`` and refuse to be used after it.  When a
call returns or raises, every handle made during it that is neither returned nor held by the state has been freed, nothing was
used after it was freed, and the state is what the code says it is.  No library, no GPU."""
import collections
import gc

import numpy as np
import pytest
import scipy.sparse as sp

import string_grouper_amd._native as N
import string_grouper_amd.engine as E

N_COLS = 500


class UsedAfterFree(AssertionError):
    pass


class Fake(N._Handle):
    """A handle of the fake context: counted by ``N.live_handles()`` like a real one (no library function behind it)."""

    def __init__(self, ctx, kind, rows=0, stride=0, fill=0):
        super().__init__(ctx, object())
        self.kind, self.rows, self.stride, self.fill = kind, rows, stride, fill
        self.name = f"{kind}{len(ctx.made)}"
        ctx.made.append(self)

    def free(self):
        if self._live:
            self.ctx.events.append(("free", self.name))
        super().free()

    def live(self):
        if not self._live:
            raise UsedAfterFree(self.name)
        return self

    def __len__(self):                        # (a list of row numbers)
        return self.live().rows

    def dims(self):
        self.live()
        return (self.rows, N_COLS, 3 * self.rows, N.SG_F32) if self.kind == "csr" else (self.rows, self.stride, N.SG_F32, N_COLS)

    def counts(self):
        return np.full(self.live().rows, self.fill, np.int32)

    def row_block(self, lo, hi):
        return self.ctx.call("row_block", [self], "csr", hi - lo)

    def to_scipy(self):
        return sp.csr_matrix((self.live().rows, N_COLS), dtype=np.float32)


class FakeContext:
    """The ``Context`` methods the corpus code calls.  ``fail[(method, k)] = exception``: the k-th call of it raises;
    ``fills``: the longest row of the results of the successive ``spgemm_topn`` calls (0 when the list runs out)."""

    def __init__(self, fail=None, fills=(), short_rows=()):
        self.made, self.events, self.n_calls = [], [], collections.Counter()
        self.fail, self.fills, self.short_rows = dict(fail or {}), list(fills), np.array(short_rows, np.int32)

    def call(self, method, handles, kind=None, rows=0, stride=0, fill=0):
        for h in handles:
            h.live()
        self.n_calls[method] += 1
        self.events.append(("call", method))
        if (method, self.n_calls[method]) in self.fail:
            raise self.fail[(method, self.n_calls[method])]
        return Fake(self, kind, rows, stride, fill) if kind else None

    def options(self):
        return {}

    def csr(self, rows):
        return Fake(self, "csr", rows)

    def topn(self, rows, stride):
        return Fake(self, "topn", rows, stride)

    def postings_build(self, m):
        return self.call("postings_build", [m], "index")

    def spgemm_topn(self, A, index, top_n, threshold, sort=True):
        return self.call("spgemm_topn", [A, index], "topn", A.rows, top_n, self.fills.pop(0) if self.fills else 0)

    def topn_zip(self, parts, offsets, top_n):
        assert len(parts) == len(offsets) > 1
        return self.call("topn_zip", parts, "topn", parts[0].rows, top_n)

    def topn_drop_columns(self, res, dead, top_n):
        return self.call("topn_drop_columns", [res, dead], "topn", res.rows, top_n)

    def topn_transpose_select(self, pairs, n_rows_out, top_n):
        return self.call("topn_transpose_select", [pairs], "topn", n_rows_out, top_n)

    def topn_concat_rows(self, parts):
        return self.call("topn_concat_rows", parts, "topn", sum(p.rows for p in parts), max(p.stride for p in parts))

    def topn_forget(self, res, dead, top_n):
        left = self.call("topn_forget", [res, dead], "topn", res.rows - len(dead), res.stride)
        return left, Fake(self, "ints", len(self.short_rows))

    def topn_put_rows(self, res, rows, n_rows, src):
        assert n_rows == len(rows) == src.rows
        self.call("topn_put_rows", [res, rows, src])

    def download_ints(self, ints):
        self.call("download_ints", [ints])
        return self.short_rows

    def upload_ints(self, values):
        return self.call("upload_ints", [], "ints", len(values))

    upload_sorted_ints = upload_ints

    def csr_take_rows(self, m, rows):
        return self.call("csr_take_rows", [m, rows], "csr", len(rows))

    def csr_concat(self, parts):
        return self.call("csr_concat", parts, "csr", sum(p.rows for p in parts))

    def csr_select_rows(self, m, drop):
        return self.call("csr_select_rows", [m, drop], "csr", m.rows - len(drop))

    def frees(self):
        return [name for what, name in self.events if what == "free"]


class FakeVectoriser:
    last_refit_s = {}

    def __init__(self, ctx, refuses=False):
        self.ctx, self.refuses, self.freed = ctx, refuses, 0

    def refit_idf_prepared(self, rows):
        rows.live()
        if self.refuses:
            raise NotImplementedError("made under another idf")
        return self.ctx.csr(rows.rows)

    def handles(self):
        return []

    def free(self):
        self.freed += 1


def corpus(n_base=100_000, n_delta=50_000, dead=(), kept=None, **ctx_options):
    """(engine, state, context): a corpus of one or two segments on a fake context, nothing multiplied yet."""
    ctx = FakeContext(**ctx_options)
    eng = E.HipEngine(ctx)
    state = E.CorpusState(FakeVectoriser(ctx), None, ctx.csr(n_base), engine=eng)
    if n_delta:
        state.set_segments(state.base, E.CorpusSegment(ctx.csr(n_delta)))
    if len(dead):
        state.set_dead(np.array(dead, np.int64))
    if kept is not None:
        state.kept, state.kept_opts = ctx.topn(state.matrix.shape[0], kept), (kept, 0.8)
    ctx.n_calls.clear()
    ctx.events.clear()
    return eng, state, ctx


def left_behind(ctx, state, *returned):
    mine = state.handles() + [h for h in returned if h is not None]
    return [h.name for h in ctx.made if h._live and not any(h is m for m in mine)]


def new_rows(ctx, n):
    return E.DeviceMatrix(ctx.csr(n))


# ------------------------------------------------------------------------------------------ 1. the scope
class Plain:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def free(self):
        self.log.append(self.name)


def test_the_scope_frees_in_reverse_order_also_when_the_body_raises():
    log = []
    with N.Scope() as s:
        a, b, c = (s.own(Plain(log, n)) for n in "abc")
        assert s.own(None) is None
    assert log == ["c", "b", "a"]
    del log[:]
    with pytest.raises(KeyError, match="the body's"):
        with N.Scope() as s:
            s.own(Plain(log, "a"))
            s.own(Plain(log, "b"))
            raise KeyError("the body's")
    assert log == ["b", "a"]


def test_the_scope_keeps_releases_and_frees_once():
    log = []
    with N.Scope() as s:
        a, b, c = (s.own(Plain(log, n)) for n in "abc")
        assert s.keep(b) is b                                         # the caller's now
        s.release(c)
        assert log == ["c"]                                           # freed now ...
        assert s.own(a) is a                                          # put in twice
        outsider = Plain(log, "x")
        assert s.keep(outsider) is outsider                           # never in it: nothing to take out
    assert log == ["c", "a"]                                          # ... and not again; a once; b not at all


def test_freeing_a_handle_twice_counts_and_releases_once():
    gc.collect()
    ctx, before = FakeContext(), N.live_handles()
    h = ctx.csr(3)
    ints = N.DeviceInts.adopt(ctx, None, 0)                           # (no pointer: nothing for the library to free)
    assert N.live_handles() == before + 2 and len(ints) == 0
    for _ in range(2):
        h.free()
        ints.free()
    assert N.live_handles() == before and ctx.frees() == [h.name]
    with pytest.raises(UsedAfterFree):
        h.dims()


# ------------------------------------------------------------------------------------------ 2. the reverse path
def test_reverse_frees_the_complete_list_when_a_later_multiply_is_refused():
    """The first segment's list is complete at the first cap, the second segment's comes back full, the cap grows and the
    third multiply is refused."""
    eng, state, ctx = corpus(fills=[10, 64], fail={("spgemm_topn", 3): MemoryError("refused")})
    batch = new_rows(ctx, 4)
    with pytest.raises(MemoryError, match="refused"):
        eng._corpus_reverse(state, state.matrix, batch, 20, 0.8)
    assert ctx.n_calls["spgemm_topn"] == 3
    complete, full = [h for h in ctx.made if h.kind == "topn"]
    assert ctx.frees() == [full.name, complete.name]                  # the full list before the cap grew, the complete one now
    assert left_behind(ctx, state, batch.csr) == []


def test_reverse_gives_up_over_the_budget_and_frees_everything():
    eng, state, ctx = corpus(fills=[10])
    eng.CORPUS_PAIR_BUDGET = 300                                      # 4 x 64 fits, 4 x (64 + 64) does not
    batch = new_rows(ctx, 4)
    assert eng._corpus_reverse(state, state.matrix, batch, 20, 0.8) is None
    assert ctx.n_calls["spgemm_topn"] == 1 and left_behind(ctx, state, batch.csr) == []


def test_reverse_with_dead_rows_leaves_only_its_result():
    eng, state, ctx = corpus(dead=[3, 100_001], fills=[10, 64, 70])
    batch = new_rows(ctx, 4)
    res = eng._corpus_reverse(state, state.matrix, batch, 20, 0.8)
    assert (res.rows, res.stride) == (149_998, 20) and res._live
    assert left_behind(ctx, state, batch.csr, res) == []
    # every list goes as soon as the next step has been made from it
    base_pairs, full, delta_pairs, zipped, live = [h.name for h in ctx.made if h.kind == "topn"][:5]
    assert [e for e in ctx.events if e[1] not in ("postings_build",)] == [
        ("call", "spgemm_topn"), ("call", "spgemm_topn"), ("free", full), ("call", "spgemm_topn"), ("call", "topn_zip"),
        ("free", delta_pairs), ("free", base_pairs), ("call", "topn_drop_columns"), ("free", zipped),
        ("call", "topn_transpose_select"), ("free", live)]


# ------------------------------------------------------------------------------------------ 3. _topn_device, blocked
TOO_LARGE = {("postings_build", 1): OverflowError("whole"), ("postings_build", 3): OverflowError("second of two blocks")}


def test_blocked_multiply_frees_the_blocks_that_did_not_fit_and_everything_but_its_result():
    ctx = FakeContext(fail=TOO_LARGE)
    A, B = new_rows(ctx, 10), new_rows(ctx, 1000)
    res = E.HipEngine(ctx)._topn_device(A, B, 20, 0.8)
    assert ctx.n_calls["postings_build"] == 7 and ctx.n_calls["spgemm_topn"] == 4 and ctx.n_calls["topn_zip"] == 1
    assert [h.name for h in ctx.made if h._live] == [A.csr.name, B.csr.name, res.name]
    # the two-block attempt: its first view and index, and the view whose index did not fit, went before the next attempt
    second_attempt = ctx.events.index(("call", "row_block"), 6)
    assert [e[0] for e in ctx.events[:second_attempt]] == ["call", "call", "call", "call", "call", "free", "free", "free"]


def test_blocked_multiply_frees_everything_when_a_part_is_refused():
    ctx = FakeContext(fail={**TOO_LARGE, ("spgemm_topn", 2): MemoryError("refused")})
    A, B = new_rows(ctx, 10), new_rows(ctx, 1000)
    with pytest.raises(MemoryError, match="refused"):
        E.HipEngine(ctx)._topn_device(A, B, 20, 0.8)
    assert [h.name for h in ctx.made if h._live] == [A.csr.name, B.csr.name]


def test_one_index_is_freed_when_its_multiply_is_refused():
    ctx = FakeContext(fail={("spgemm_topn", 1): MemoryError("refused")})
    A, B = new_rows(ctx, 10), new_rows(ctx, 1000)
    with pytest.raises(MemoryError):
        E.HipEngine(ctx)._topn_device(A, B, 20, 0.8)
    assert [h.name for h in ctx.made if h._live] == [A.csr.name, B.csr.name]


def test_nothing_fits_is_an_overflow_error_and_frees_everything():
    ctx = FakeContext(fail={("postings_build", k): OverflowError("too large") for k in range(1, 20)})
    A, B = new_rows(ctx, 10), new_rows(ctx, 3)
    with pytest.raises(OverflowError):
        E.HipEngine(ctx)._topn_device(A, B, 20, 0.8)
    assert [h.name for h in ctx.made if h._live] == [A.csr.name, B.csr.name]


# ------------------------------------------------------------------------------------------ 4. topn_multiply_blocked
def test_explicit_blocks_free_everything_when_the_second_left_block_is_refused():
    ctx = FakeContext(fail={("spgemm_topn", 3): MemoryError("refused")})
    A, B = new_rows(ctx, 10), new_rows(ctx, 1000)
    with pytest.raises(MemoryError, match="refused"):
        E.HipEngine(ctx).topn_multiply_blocked(A, B, (2, 2), 20, 0.8)
    assert ctx.n_calls["topn_zip"] == 1
    assert [h.name for h in ctx.made if h._live] == [A.csr.name, B.csr.name]


def test_explicit_blocks_leave_nothing_behind():
    ctx = FakeContext()
    A, B = new_rows(ctx, 10), new_rows(ctx, 1000)
    C = E.HipEngine(ctx).topn_multiply_blocked(A, B, (2, 2), 20, 0.8)
    assert C.shape == (10, 1000)
    assert ctx.n_calls["spgemm_topn"] == 4 and [h.name for h in ctx.made if h._live] == [A.csr.name, B.csr.name]


# ------------------------------------------------------------------------------------------ 5. a kept self-join
def test_append_update_drops_the_kept_result_when_the_multiply_is_refused():
    eng, state, ctx = corpus(kept=20, fail={("spgemm_topn", 1): MemoryError("refused")})
    kept, new = state.kept, ctx.csr(3)
    with pytest.raises(MemoryError, match="refused"):
        eng._kept_old_rows_against(state, new)
    assert state.kept is None and not kept._live and state.kept_opts == (20, 0.8)
    assert new._live and left_behind(ctx, state, new) == []           # the caller's rows are the caller's to free


def test_append_update_of_a_corpus_that_has_outgrown_its_indexes_leaves_nothing():
    eng, state, ctx = corpus(kept=20)
    state.index_overflow = True
    with N.Scope() as s:
        old_rows = s.own(ctx.topn(150_000 - 7, 20))
        eng._kept_add_new_rows(state, old_rows, 7)
        assert old_rows._live                                         # not the callee's to free
        assert state.kept is None and state.kept_opts == (20, 0.8) and left_behind(ctx, state, old_rows) == []
    assert state.stats["self_join_append_updates"] == 0 and left_behind(ctx, state) == []


SHORT = [7, 100_020]                                                  # live numbers: one in the base, one in the delta


@pytest.mark.parametrize("what", ["refilled", "refused", "wider"])
def test_remove_update_frees_the_list_of_short_rows(what):
    fail = {("spgemm_topn", 2): MemoryError("refused")} if what == "refused" else {}
    eng, state, ctx = corpus(kept=10 if what == "wider" else 20, short_rows=SHORT, fail=fail)
    kept_before = state.kept
    if what == "wider":
        state.kept_opts = (20, 0.8)                                   # the refilled rows come back 20 wide, the kept stride is 10
    if what == "refused":
        with pytest.raises(MemoryError, match="refused"):
            eng.corpus_remove(state, [5, 100_010])
    else:
        eng.corpus_remove(state, [5, 100_010])
    assert not kept_before._live and left_behind(ctx, state) == []
    assert not any(h._live for h in ctx.made if h.kind == "ints" and h is not state.dead_dev)      # topn_forget's list too
    assert list(state.dead) == [5, 100_010] and state.stats["dead_rows"] == 2
    if what == "refilled":
        assert state.kept._live and state.kept.rows == 149_998 and state.stats["self_join_rows_refilled"] == 2
        assert ctx.n_calls["csr_take_rows"] == 2 and ctx.n_calls["csr_concat"] == 1 and ctx.n_calls["topn_put_rows"] == 1
        assert state.stats["self_join_remove_updates"] == 1
    else:
        assert state.kept is None and state.kept_opts == (20, 0.8) and ctx.n_calls["topn_put_rows"] == 0
        assert state.stats["self_join_remove_updates"] == (1 if what == "wider" else 0)


# ------------------------------------------------------------------------------------------ 6. compact, refit
def _snapshot(state):
    return state.segments, [h for seg in state.segments for h in seg.handles()], list(state.dead), state.dead_dev, dict(state.stats)


def test_a_refused_compaction_leaves_the_corpus_as_it_was():
    eng, state, ctx = corpus(dead=[3, 100_001], fail={("csr_select_rows", 1): MemoryError("refused")})
    eng.corpus_indexes(state)
    before = _snapshot(state)
    with pytest.raises(MemoryError, match="refused"):
        eng.corpus_compact(state)
    after = _snapshot(state)
    assert all(a is b for a, b in zip(after[0], before[0])) and after[1:] == before[1:]
    assert all(h._live for h in before[1]) and state.dead_dev._live and len(before[1]) == 4
    assert left_behind(ctx, state) == []                              # (the concatenation it made is the state's cache)


def test_a_refused_refit_leaves_the_corpus_as_it_was():
    eng, state, ctx = corpus()
    state.vec.refuses = True
    eng.corpus_indexes(state)
    before = _snapshot(state)
    with pytest.raises(NotImplementedError, match="another idf"):
        eng.corpus_refit_idf(state)
    after = _snapshot(state)
    assert all(a is b for a, b in zip(after[0], before[0])) and after[1:] == before[1:]
    assert all(h._live for h in before[1]) and left_behind(ctx, state) == []


def test_compaction_and_refit_hand_their_rows_to_the_state():
    eng, state, ctx = corpus(dead=[3, 100_001], kept=20)
    eng.corpus_indexes(state)
    old = [h for seg in state.segments for h in seg.handles()]
    eng.corpus_compact(state)
    assert state.base.n_rows == 149_998 and state.delta is None and not len(state.dead) and state.kept._live
    assert not any(h._live for h in old) and left_behind(ctx, state) == []
    old = state.base.handles()
    eng.corpus_refit_idf(state)
    assert state.kept is None and state.stats["idf_refits"] == 1
    assert not any(h._live for h in old) and left_behind(ctx, state) == []


# ------------------------------------------------------------------------------------------ 7. corpus_free
def test_corpus_free_frees_every_handle_index_before_matrix():
    gc.collect()
    baseline = N.live_handles()
    eng, state, ctx = corpus(dead=[3, 100_001], kept=20)
    eng.corpus_indexes(state)
    state.physical()
    held = state.handles()
    assert [h.kind for h in held] == ["index", "csr", "index", "csr", "csr", "topn", "ints"] and all(h._live for h in held)
    assert N.live_handles() == baseline + len(held)
    vec = state.vec
    eng.corpus_free(state)
    assert ctx.frees() == [h.name for h in held]                      # in the order the state lists them
    assert vec.freed == 1 and not any(h._live for h in ctx.made)
    assert N.live_handles() == baseline
    assert state.kept is None and state.kept_opts is None and state.base is None and state.matrix is None
