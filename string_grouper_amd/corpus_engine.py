"""The engine's side of a resident corpus (string_grouper_amd/corpus.py): what the corpus keeps on the
device (``CorpusState``), its rows as the front end sees them (``CorpusMatrix``), and ``CorpusEngine`` -- fit, transform,
append, remove, compact, refit, the multiplies against the corpus's own indexes, named pairs, records of several fields and
the self-join that is kept.

One rule for device handles: whoever makes one puts it into a scope (``N.Scope``) or into the state, and no function frees
an argument it was handed -- but the ones whose name says so (``free``, ``drop_whole``, ``drop_kept``, ``corpus_free``)."""
from __future__ import annotations

import contextlib
import time
from typing import List, Optional, Tuple

import numpy as np

from . import _native as N
from .device_matrix import DeviceMatrix
from .record_call import RecordCall
from .strprep import StringColumn, _ascii_lower
from .vectorizer import HipTfidfVectorizer


class CorpusSegment:
    """A run of corpus rows and the inverted index over them (K3), built on first need.  The index borrows the arrays of the
    matrix it was built over (include/sg_hip.h: sg_postings_build), so the two live and die together: index first."""

    def __init__(self, csr: "N.Csr"):
        self.csr = csr
        self.index: Optional["N.Postings"] = None
        self.n_rows, _, self.nnz, _ = csr.dims()

    def handles(self) -> list:
        return [h for h in (self.index, self.csr) if h is not None]

    def free(self) -> None:
        for h in self.handles():
            h.free()
        self.index = self.csr = None


class CorpusState:
    """What a resident corpus keeps on the device (string_grouper_amd/corpus.py): the fitted vectoriser (vocabulary + idf)
    and its own TF-IDF rows in one or two segments -- ``base``, and ``delta`` for the rows appended since the last
    compaction -- each with its own inverted index from the first call that needs it.  ``whole`` is
    the concatenation of the two for the calls that need every row in one matrix (made on first need after an append, kept
    until the next).  ``stats`` counts the work, so that tests can prove the reuse.

    Removed rows stay in their segment until the next compaction: ``dead`` is the sorted list of their PHYSICAL numbers
    (counting through base, then delta), ``dead_dev`` its copy on the device.  A live row's physical number is its own plus
    the dead rows up to it (``physical_rows``); the calls against the indexes filter the dead columns out
    (CorpusEngine._corpus_topn), every call that reads the rows as one matrix compacts first (``rows``).

    A self-join that is kept (``Corpus.keep_self_join``): ``kept_opts`` is the (max_n_matches,
    min_similarity) it is kept for, ``kept`` the result over the LIVE rows -- None until the first call needs it, and again
    whenever an update could not follow a change (it is then multiplied anew on next need).  It is numbered by live rows, so a
    compaction does not touch it."""

    def __init__(self, vec: HipTfidfVectorizer, column, base: Optional["N.Csr"] = None, engine: Optional["CorpusEngine"] = None):
        self.vec = vec
        self.column = column
        self.engine = engine
        self.dead = np.zeros(0, np.int64)
        self.dead_dev: Optional["N.DeviceInts"] = None
        self.base: Optional[CorpusSegment] = None
        self.delta: Optional[CorpusSegment] = None
        self.whole: Optional["N.Csr"] = None
        self.matrix: Optional["CorpusMatrix"] = None
        self.index_overflow = False           # the corpus does not fit its indexes: every call takes today's blocked path
        self.placeholder: Optional[int] = None
        self.kept: Optional["N.TopN"] = None
        self.kept_opts: Optional[Tuple[int, float]] = None
        self.stats = {"tokenisations": 1, "index_builds": 0, "transforms": 0, "resident_index": 0, "forward": 0,
                      "reverse": 0, "reverse_fallbacks": 0, "appends": 0, "rows_appended": 0, "compactions": 0,
                      "segments": 1, "base_index_builds": 0, "removals": 0, "rows_removed": 0, "dead_rows": 0,
                      "self_join_full": 0, "self_join_served": 0, "self_join_append_updates": 0,
                      "self_join_remove_updates": 0, "self_join_rows_refilled": 0, "idf_refits": 0, "pair_calls": 0,
                      "pairs_scored": 0, "record_calls": 0, "record_union_calls": 0,
                      "record_floor_calls": 0, "record_field_score_calls": 0, "record_skip_empty_calls": 0}
        if base is not None:
            self.set_segments(CorpusSegment(base), None)

    def handles(self) -> list:
        """Every handle the state holds, in the order they must go: each segment's index before its matrix, the cached
        concatenation, the kept result, the dead list.  (The vectoriser lists its own: ``vec.handles()``.)"""
        segs = self.segments if self.base is not None else []
        held = [h for seg in segs for h in seg.handles()] + [self.whole, self.kept, self.dead_dev]
        return [h for h in held if h is not None]

    def set_segments(self, base: CorpusSegment, delta: Optional[CorpusSegment]) -> None:
        """New rows: whoever holds the old ``matrix`` object keeps its (now stale) view; every call asks for the new one."""
        self.base, self.delta = base, delta
        self.stats["segments"] = 1 if delta is None else 2
        self.matrix = CorpusMatrix(self)

    @property
    def segments(self) -> List[CorpusSegment]:
        return [self.base] if self.delta is None else [self.base, self.delta]

    @property
    def index(self) -> Optional["N.Postings"]:
        """The base segment's index (the whole corpus's as long as nothing has been appended since the last compaction)."""
        return self.base.index if self.base is not None else None

    def set_dead(self, dead: np.ndarray) -> None:
        """The dead physical rows are now ``dead`` (sorted, distinct): uploaded, the old device copy freed."""
        if self.dead_dev is not None:
            self.dead_dev.free()
        self.dead = dead
        self.dead_dev = self.base.csr.ctx.upload_sorted_ints(dead) if len(dead) else None
        self.stats["dead_rows"] = len(dead)
        self.matrix = CorpusMatrix(self)

    def physical_rows(self, live: np.ndarray) -> np.ndarray:
        """Where the live rows ``live`` lie in the segments: dead row i has dead[i] - i live rows before it."""
        return live + np.searchsorted(self.dead - np.arange(len(self.dead)), live, side="right")

    def dead_nnz(self) -> int:
        """Entries of the dead rows, read from the segments' row pointers (one small read-back per dead row, CORPUS_MAX_DEAD
        of them at the most: only when somebody asks for ``nnz`` while rows are dead)."""
        total, first = 0, 0
        for seg in self.segments:
            for d in self.dead[(self.dead >= first) & (self.dead < first + seg.n_rows)]:
                with N.Scope() as s:
                    total += s.own(seg.csr.row_block(int(d) - first, int(d) - first + 1)).dims()[2]
            first += seg.n_rows
        return total

    def rows(self) -> "N.Csr":
        """Every LIVE row in one matrix: the base segment itself, or the cached concatenation (sg_csr_concat); with dead rows
        pending, the new base segment of a compaction."""
        if len(self.dead):
            self.engine.corpus_compact(self)
        return self.physical()

    def physical(self) -> "N.Csr":
        """Every row of the segments, dead ones included, in one matrix."""
        if self.delta is None:
            return self.base.csr
        if self.whole is None:
            self.whole = self.base.csr.ctx.csr_concat([self.base.csr, self.delta.csr])
        return self.whole

    def drop_whole(self) -> None:
        if self.whole is not None:
            self.whole.free()
            self.whole = None

    def drop_kept(self) -> None:
        """The kept self-join is stale (or no longer wanted): freed, multiplied anew when a call next needs it."""
        if self.kept is not None:
            self.kept.free()
            self.kept = None

    @contextlib.contextmanager
    def updating_kept(self):
        """Around every step that makes the kept self-join follow a change: a step that fails leaves it stale, so it goes."""
        try:
            yield
        except Exception:
            self.drop_kept()
            raise


class CorpusMatrix(DeviceMatrix):
    """The TF-IDF rows of a resident corpus: the multiply uses the corpus's indexes instead of building one.  ``shape``,
    ``nnz`` and ``dtype`` come from the segments and count the LIVE rows only; ``csr`` (every live row in one matrix) is
    only made when something reads it -- which compacts a corpus that has removed rows pending."""

    def __init__(self, corpus: CorpusState):
        self.corpus = corpus
        segs = corpus.segments
        _, n_cols, _, d = segs[0].csr.dims()
        self.n_dead = len(corpus.dead)
        self.shape = (sum(s.n_rows for s in segs) - self.n_dead, n_cols)
        self._nnz_physical = sum(s.nnz for s in segs)
        self._nnz: Optional[int] = None if self.n_dead else self._nnz_physical
        self.dtype = N.code_np_dtype(d)
        self._host = None

    @property
    def nnz(self) -> int:
        if self._nnz is None:                  # (dead rows: their entries are read back when first asked for)
            if self.corpus.matrix is self:
                self._nnz = self._nnz_physical - self.corpus.dead_nnz()
            elif self.corpus.matrix is None:
                raise ValueError("the corpus is closed")
            else:                              # the corpus has moved on (compacted): its live rows are these rows
                return self.corpus.matrix.nnz
        return self._nnz

    @property
    def csr(self) -> "N.Csr":
        return self.corpus.rows()


class CorpusEngine:
    """The resident-corpus half of ``HipEngine`` (string_grouper_amd/engine.py), which inherits it.  Of the engine it needs
    ``self.ctx`` (the library context), ``self.timings`` (the dict bench.py reads), ``self._topn_device`` (the generic
    top-n multiply, for new rows against the corpus when no index of the corpus serves) and ``self._match_list_from_topn`` (the
    fused tail K6, for the list of a record call) -- nothing else."""
    # reverse path of a resident corpus: the pair slots (new rows x per-row cap) it may hold; a call
    # whose complete pair list would need more takes the forward path
    CORPUS_PAIR_BUDGET = 1 << 27
    CORPUS_FIRST_CAP = 64
    CORPUS_MAX_TOP_N = 2048                   # sg_topn_transpose_select
    # the rule: the reverse path for batches of at most this many rows.  Measured (scripts/corpus_latency.py,
    # profiles/corpus_latency_*.log): the forward path costs about what streaming the corpus costs, whatever the batch
    # (4.4 ms at 663 k names, 35 ms at 5 M); the reverse path what the batch's rows cost against the corpus index -- it is
    # the faster one up to 32 rows and the slower one from 64 on, at both sizes
    CORPUS_REVERSE_MAX_ROWS = 32
    # appended rows wait in a delta segment with an index of its own until they exceed this share of the base segment's
    # rows; then the two are folded into one (corpus_compact).  Measured (scripts/corpus_append_latency.py,
    # profiles/corpus_append_latency.log): a step of a living list (append one row, match one name) costs the more the larger
    # the delta is -- its index is rebuilt after every append: 3.8 -> 5.1 ms at 663 k names from an empty delta to a quarter
    # of the base -- while a compaction costs 1-1.4 ms at 663 k and 5-30 ms at 5 M, under 0.001 ms per appended row at any
    # share: the cheapest of the measured shares (1/64, 1/16, 1/8, 1/4) is the smallest at both sizes
    CORPUS_COMPACT_SHARE = 1 / 64
    # removed rows stay in their segment, and every multiply against the indexes is asked for top_n + dead rows, until there
    # are more than this many; then a compaction drops them (corpus_compact).  Measured (scripts/corpus_remove_latency.py,
    # profiles/corpus_remove_latency.log; caps 8, 32, 64, 128, two rounds each): the step of a living list (remove one row,
    # append one, match one name) does not separate the caps -- 663 k names: 20.0, 20.1 / 18.0, 21.4 / 21.7, 21.4 / 18.3, 21.4 ms;
    # 5 M: 143, 133 / 126, 138 / 122, 131 / 129, 133 ms (64 the cheapest of both rounds there, by 3-5 %, where one cap moves by
    # 10 % between rounds): 11-15 and 90-110 ms of a step are the host's copy of the Series, which no cap touches, the rest
    # is 6.1-6.7 and 29.4-32.9 ms at every cap (a compaction is 0.2 / 0.7 ms, the index rebuild behind it 1.2 / 5.5 ms).  What
    # does separate them is the 1 000-name batch against the index, asked for 20 + dead entries a row: 2.1 ms at 0, 8, 32
    # and 64 dead rows and 9.3 at 128 (663 k); 9.6-10.5 ms at 0, 8 and 32, 42.6 at 64 and 89.9 at 128 (5 M).  32 is the largest
    # measured cap that costs no query anything at either size -- the default max_n_matches of 20 plus 32 stays inside the
    # one register list of 64 (plan_multiply) -- and a step gains nothing measurable beyond it
    CORPUS_MAX_DEAD = 32

    # ------------------------------------------------------------------ fit, transform, free
    def corpus_fit(self, strings, ngram_size, regex, ignore_case, normalize_to_ascii, dtype) -> CorpusState:
        """TfidfVectorizer(min_df=1, analyzer=n_grams, dtype).fit(strings), once; the corpus's own rows stay on the device."""
        vec = HipTfidfVectorizer(ngram_size=ngram_size, regex=regex, ignore_case=ignore_case,
                                 normalize_to_ascii=normalize_to_ascii, dtype=dtype, ctx=self.ctx)
        col = vec.prepare(strings)
        vec.fit_prepared([col])
        return CorpusState(vec, col, vec.transform_prepared(col), engine=self)

    def corpus_transform(self, state: CorpusState, strings) -> DeviceMatrix:
        """The rows of ``strings`` under the corpus's vocabulary and idf: n-grams the corpus never had are dropped."""
        state.stats["transforms"] += 1
        return DeviceMatrix(self._corpus_rows_of(state, strings))

    def _corpus_rows_of(self, state: CorpusState, strings) -> "N.Csr":
        vec = state.vec
        with N.Scope() as s:
            col = s.own(vec.prepare(strings))                       # (its upload: by prepare, or by the transform below)
            if col.kind == "symbols" and vec._alphabet is None:
                # characters beyond ASCII (normalize_to_ascii=False) against a vocabulary of ASCII n-grams: every n-gram with
                # one of them is out of vocabulary.  Each such character becomes one byte the corpus never had, so that the
                # device drops exactly those n-grams (its own treatment of bytes >= 0x80 would join the neighbours instead).
                col = s.own(self._corpus_bytes_column(state, col))
            return vec.transform_prepared(col)

    @staticmethod
    def _corpus_bytes_column(state: CorpusState, col):
        if state.placeholder is None:
            data = state.column.data if state.column.kind == "bytes" else np.zeros(0, np.uint8)
            seen = np.zeros(256, bool)
            seen[np.unique(data)] = True
            seen[np.unique(_ascii_lower(data))] = True
            deleted = state.vec._delete_table.astype(bool)
            free = [c for c in range(1, 128) if not seen[c] and not deleted[c] and not (65 <= c <= 90)]
            if not free:
                raise NotImplementedError("the corpus uses every ASCII character: no byte is left to stand for the "
                                          "characters it never had")
            state.placeholder = free[0]
        cps = col.data
        data = np.where(cps < 128, cps, state.placeholder).astype(np.uint8)
        return StringColumn("bytes", data, col.offsets, prelowered=True)

    def corpus_matrix(self, state: CorpusState) -> "CorpusMatrix":
        return state.matrix

    def corpus_free(self, state: CorpusState) -> None:
        for h in state.handles():
            h.free()
        state.vec.free()
        state.whole = state.kept = state.kept_opts = state.dead_dev = None
        state.dead = np.zeros(0, np.int64)
        state.base = state.delta = state.matrix = None

    # ------------------------------------------------------------------ append, remove, compact, refit
    def corpus_append(self, state: CorpusState, strings) -> None:
        """The rows of ``strings`` (under the corpus's vocabulary and idf, as corpus_transform makes them) join the corpus
        behind its last row.  The cost follows the batch and the delta segment, not the corpus: the new rows are
        concatenated to the delta's (sg_csr_concat), whose index is dropped and rebuilt on first need; the base segment and
        its index are not touched until the delta outgrows CORPUS_COMPACT_SHARE of the base (corpus_compact)."""
        n_new = len(strings)
        if n_new == 0:
            return
        with N.Scope() as s:
            new = s.own(self._corpus_rows_of(state, strings))
            old_rows = s.own(self._kept_old_rows_against(state, new))   # (None: no self-join is kept)
            state.drop_whole()
            if state.delta is None:
                delta = CorpusSegment(s.keep(new))
            else:
                delta = CorpusSegment(self.ctx.csr_concat([state.delta.csr, new]))
                state.delta.free()
                s.release(new)
            state.set_segments(state.base, delta)
            state.stats["appends"] += 1
            state.stats["rows_appended"] += n_new
            if delta.n_rows > self.CORPUS_COMPACT_SHARE * state.base.n_rows:
                self.corpus_compact(state)
            if old_rows is not None:
                self._kept_add_new_rows(state, old_rows, n_new)

    def corpus_remove(self, state: CorpusState, positions) -> None:
        """The rows ``positions`` (sorted, distinct, numbered as the corpus's live rows are now) leave the corpus.  Nothing on
        the device is touched but the list of dead rows: they stay in their segment and its index, the multiplies against
        the indexes ask for as many entries more and drop them (_corpus_topn), and a compaction (corpus_compact: explicit, by
        an append's share rule, by a call that needs the rows in one matrix, or here once more than CORPUS_MAX_DEAD are
        pending) takes them out."""
        positions = np.asarray(positions, dtype=np.int64)
        if len(positions) == 0:
            return
        n_live = state.matrix.shape[0]
        if positions[0] < 0 or positions[-1] >= n_live or np.any(positions[1:] <= positions[:-1]):
            raise IndexError(f"positions must be ascending, distinct and inside [0, {n_live})")
        if len(positions) == n_live:
            raise ValueError("every row of the corpus would be removed: build a new corpus instead")
        with N.Scope() as s:
            short = s.own(self._kept_forget(state, positions))          # (None: no self-join is kept)
            state.set_dead(np.union1d(state.dead, state.physical_rows(positions)))
            state.stats["removals"] += 1
            state.stats["rows_removed"] += len(positions)
            if len(state.dead) > self.CORPUS_MAX_DEAD:
                self.corpus_compact(state)
            if short is not None:
                self._kept_refill(state, short)

    def corpus_compact(self, state: CorpusState) -> None:
        """Fold the delta segment into the base and drop the dead rows: one matrix of the live rows (sg_csr_concat, then
        sg_csr_select_rows), one index (built on first need), and with them the self-join form of the multiply for a self-join
        of the corpus.  Nothing to do without a delta and without dead rows."""
        if state.delta is None and not len(state.dead):
            return
        with N.Scope() as s:
            whole = state.physical()
            if len(state.dead):
                whole = s.own(self.ctx.csr_select_rows(whole, state.dead_dev))
                state.drop_whole()
            state.whole = None                # (handed to the new base segment)
            old = state.segments
            state.set_dead(np.zeros(0, np.int64))
            state.set_segments(CorpusSegment(s.keep(whole)), None)
        for seg in old:
            seg.free()
        state.stats["compactions"] += 1

    def corpus_refit_idf(self, state: CorpusState) -> None:
        """The idf follows the CURRENT list, the vocabulary stays the original's: what sklearn's vectoriser gives when it is
        fitted on the live strings with ``vocabulary=`` fixed.  No string is read (``stats['tokenisations']`` stays 1): the live
        rows in one matrix (a compaction when rows are dead), their column counts, numpy's idf of those, and one pass that
        weights the rows anew (HipTfidfVectorizer.refit_idf_prepared) into a NEW base segment; then the old segments go, index
        first, and with them the cached concatenation and a kept self-join -- every score has changed, so it is multiplied
        anew when next needed (its options stay).  A refusal of the device leaves the corpus as it was."""
        t0 = time.perf_counter()
        rows = state.rows()
        t1 = time.perf_counter()
        new = CorpusSegment(state.vec.refit_idf_prepared(rows))     # (made and handed to the state: nothing between)
        old = state.segments
        state.set_segments(new, None)
        for seg in old:
            seg.free()
        state.drop_whole()
        state.drop_kept()
        state.stats["idf_refits"] += 1
        self.timings = dict(refit_rows_s=t1 - t0, **{f"refit_{k}_s": v for k, v in state.vec.last_refit_s.items()})

    # ------------------------------------------------------------------ the corpus's indexes and the multiplies against them
    def _segment_index(self, state: CorpusState, seg: CorpusSegment) -> Optional["N.Postings"]:
        if seg.index is None and not state.index_overflow:
            try:
                seg.index = self.ctx.postings_build(seg.csr)
                state.stats["index_builds"] += 1
                if seg is state.base:
                    state.stats["base_index_builds"] += 1
            except OverflowError:
                state.index_overflow = True
        return None if state.index_overflow else seg.index

    def corpus_index(self, state: CorpusState) -> Optional["N.Postings"]:
        """The inverted index over the base segment's rows (all rows as long as no delta exists), built on first need and
        kept; None when the corpus is too large for its indexes (the callers then take the blocked path of _topn_device)."""
        return self._segment_index(state, state.base)

    def corpus_indexes(self, state: CorpusState) -> Optional[List[Tuple["N.Postings", int, int]]]:
        """(index, first row, rows) of every segment, or None when one of them does not fit an index."""
        out, first = [], 0
        for seg in state.segments:
            idx = self._segment_index(state, seg)
            if idx is None:
                return None
            out.append((idx, first, seg.n_rows))
            first += seg.n_rows
        return out

    def _corpus_reverse_mode(self) -> Optional[bool]:
        v = self.ctx.options().get("SG_CORPUS_REVERSE")
        return None if v in (None, "") else v.strip() not in ("0", "false", "False")

    def _corpus_topn(self, A: DeviceMatrix, B: DeviceMatrix, top_n: int, threshold: float) -> Optional["N.TopN"]:
        """The multiply of a call on a resident corpus, or None for the generic path of _topn_device.
        B the corpus (a self-join of it included): the new rows against the corpus's own index.
        A the corpus, B new rows: the forward path (the corpus rows against an index of the new rows: the generic path) or
        the reverse path (the new rows against the corpus index, turned round by sg_topn_transpose_select)."""
        if isinstance(B, CorpusMatrix):
            state = B.corpus
            if A is B and B is state.matrix and state.kept_opts == (int(top_n), float(threshold)):
                return self._kept_copy(state)
            return self._corpus_against_indexes(state, A, top_n, threshold)
        state = A.corpus
        mode = self._corpus_reverse_mode()
        if mode is None:
            mode = B.shape[0] <= self.CORPUS_REVERSE_MAX_ROWS and B.shape[0] < A.shape[0]
        if mode:
            res = self._corpus_reverse(state, A, B, top_n, threshold)
            if res is not None:
                state.stats["reverse"] += 1
                return res
            state.stats["reverse_fallbacks"] += 1
        state.stats["forward"] += 1
        return None

    def _corpus_against_indexes(self, state: CorpusState, A: DeviceMatrix, top_n: int, threshold: float) -> Optional["N.TopN"]:
        """The rows of ``A`` (the corpus itself: a self-join) against the corpus's own indexes, in live numbering; None when
        the corpus does not fit its indexes."""
        if isinstance(A, CorpusMatrix) and len(state.dead):
            self.corpus_compact(state)    # a self-join reads the rows as one matrix: no dead rows in it
        segs = self.corpus_indexes(state)
        if segs is None:
            return None
        state.stats["resident_index"] += 1
        # dead rows are still in the indexes: at most that many of a row's first top_n + dead entries are dead, so the
        # first top_n live ones of the longer list are the top_n over the live rows
        n_dead = len(state.dead)
        ask = top_n + n_dead
        with N.Scope() as s:
            with N.Scope() as per_segment:
                parts = [per_segment.own(self.ctx.spgemm_topn(A.csr, idx, ask, threshold, True)) for idx, _, _ in segs]
                res = s.own(per_segment.keep(self._zip_segments(parts, segs, ask)))
            return self._drop_dead(state, res, top_n) if n_dead else s.keep(res)

    def _zip_segments(self, parts: List["N.TopN"], segs, top_n: int) -> "N.TopN":
        """The results against the segments' indexes as one over the corpus's rows: columns offset by the segment's first
        row, merged by score descending, then row ascending (K5), cut at top_n.  One segment: its part ITSELF, not a copy --
        so the caller holds the parts in a scope of their own and ``keep``s the result out of it, which takes the part out
        when it is the result and nothing when it is not; the scope then frees the parts that have been merged."""
        if len(parts) == 1:
            return parts[0]
        return self.ctx.topn_zip(parts, np.array([first for _, first, _ in segs], dtype=np.int64), top_n)

    def _drop_dead(self, state: CorpusState, res: "N.TopN", top_n: int) -> "N.TopN":
        """``res`` over the segments' physical rows as a new result over the live rows: dead columns out, the others
        renumbered, rows cut at top_n (sg_topn_drop_columns)."""
        return self.ctx.topn_drop_columns(res, state.dead_dev, top_n)

    def _corpus_reverse(self, state: CorpusState, A: DeviceMatrix, B: DeviceMatrix, top_n: int,
                        threshold: float) -> Optional["N.TopN"]:
        """Every pair above the threshold from the new rows' side -- per segment, the cap per new row grows until no row
        comes back full -- then the top_n per corpus row.  None (nothing returned, the caller takes the forward path) when
        the pair lists of the segments together would exceed the budget or top_n exceeds what the select kernel takes."""
        n_corpus, n_new = A.shape[0], B.shape[0]
        if top_n > self.CORPUS_MAX_TOP_N or n_new == 0 or n_corpus == 0:
            return None
        segs = self.corpus_indexes(state)
        if segs is None:
            return None
        with N.Scope() as s:
            with N.Scope() as per_segment:
                parts, slots = [], 0          # slots: what the complete parts so far hold per new row
                for idx, _, n_seg in segs:
                    cap = self.CORPUS_FIRST_CAP
                    while True:
                        stride = min(cap, n_seg)
                        if n_new * (slots + stride) > self.CORPUS_PAIR_BUDGET:
                            return None
                        pairs = per_segment.own(self.ctx.spgemm_topn(B.csr, idx, stride, threshold, True))
                        cnt = pairs.counts()
                        if stride >= n_seg or int(cnt.max()) < stride:
                            break
                        per_segment.release(pairs)
                        cap *= 8
                    parts.append(pairs)
                    slots += stride
                # asked for the sum of the strides: nothing is cut
                pairs = s.own(per_segment.keep(self._zip_segments(parts, segs, slots)))
            if len(state.dead):               # (a dead row counted towards a full row and the budget like any other)
                physical, pairs = pairs, s.own(self._drop_dead(state, pairs, pairs.dims()[1]))
                s.release(physical)
            return self.ctx.topn_transpose_select(pairs, n_corpus, top_n)

    # ------------------------------------------------------------------ named pairs
    def corpus_pairs(self, state: CorpusState, left, right, other: Optional[DeviceMatrix] = None) -> np.ndarray:
        """The similarity of the corpus rows ``left[p]`` and ``right[p]`` (LIVE numbering), or with ``other`` of the corpus
        row ``left[p]`` and row ``right[p]`` of ``other``: the element the multiply reports for the pair, bit for bit
        (sg_csr_pairs_dot).  The rows are read where they lie: live numbers become physical ones (``physical_rows``) and the
        matrix is ``state.physical()`` -- the base segment, or with appended rows waiting the cached concatenation, dead rows
        and all -- so a pair call never compacts.  No handle is made here but the state's own cached concatenation; the two
        index lists live and die inside ``Context.pairs_dot``."""
        left = state.physical_rows(np.asarray(left, dtype=np.int64))
        right = np.asarray(right, dtype=np.int64)
        if other is None:
            right = state.physical_rows(right)
        rows = state.physical()
        state.stats["pair_calls"] += 1
        state.stats["pairs_scored"] += len(left)
        return self.ctx.pairs_dot(rows, rows if other is None else other.csr, left, right)

    # ------------------------------------------------------------------ records of several fields
    RECORD_OPTIONS = frozenset({"union", "floors", "field_scores", "skip_empty"})     # what RecordCall.needs may ask

    def corpus_records(self, state: CorpusState, others: List[CorpusState], B: DeviceMatrix,
                       B_fields: Optional[List[DeviceMatrix]], call: RecordCall, top_n: int, threshold: float,
                       self_join_fix: bool, keep_on_device: bool = False):
        """The match list of RECORDS as ``call`` describes it (string_grouper_amd/record_call.py): the candidate fields find
        the candidates, every field -- ``state``'s first, row p of every corpus is record p -- scores them, and the weighed
        sum is filtered, ordered and cut on the device (sg_topn_rescore; with ``call.floors`` a floor a field before the cut,
        with ``call.skip_empty`` the fields empty for a pair left out) before the list is built (K6).  Returns ``(list,
        planes)``: the list as ``match_list`` returns it for the same ``keep_on_device``; ``planes`` None, or with
        ``call.field_scores`` an array ``[fields, entries]`` of the corpus's dtype, plane k every list entry's score on field k
        with the bits ``corpus_pairs`` of that field returns, the diagonal and the mirrored entries of ``self_join_fix``
        included (sg_matchlist_field_scores, on the list where it lies before it is freed or kept).

        ``B``: the primary field's right-hand rows -- ``state.matrix`` itself for a self-join, else the transformed duplicates
        -- and ``B_fields`` the further fields' (None for a self-join).  A candidate field's multiply is ``_topn_device``'s on
        that field's own matrices: the resident index, the forward and the reverse path and a kept self-join serve as for
        ``match_strings``, so a candidate field's corpus builds its index and a self-join compacts it.  Several candidate fields'
        results are united on the device (sg_topn_union: the primary's score fills in what its multiply did not find).  A
        corpus that is NOT a candidate field is read where it lies -- ``physical()`` with the dead list -- and is never
        compacted, never indexed.  The rows and the dead lists the union, the rescoring and the planes read are taken AFTER
        the multiplies, which may have compacted a candidate corpus; results number the live rows, which no compaction changes.

        Handles: the candidates live in a scope that ends with the rescoring, every candidate field's own in one that ends with
        the union, the rescored result in the method's (``_match_list_from_topn`` frees it early, as it frees a multiply's)."""
        t = time.perf_counter()
        states, rights = self._record_matrices(state, others, B, B_fields, call)
        self_join = B_fields is None

        def field(k: int):
            """Field k as the union, the rescoring and the planes take it, read where it lies NOW: after the multiplies."""
            rows = states[k].physical()       # (the state's own cached concatenation when rows wait in a delta)
            dead = states[k].dead_dev
            return (rows, rows, dead, dead) if self_join else (rows, rights[k].csr, dead, None)

        with N.Scope() as s:
            with N.Scope() as before:         # the candidates go as soon as they are rescored
                cand = before.own(self._record_candidates(states, rights, call, self_join, field))
                fields = [field(k) for k in range(1, call.n_fields)]
                weighed = [(rows, right, w, dead_a, dead_b) for (rows, right, dead_a, dead_b), w in zip(fields, call.weights[1:])]
                # one call, the library's one entry: the floors and skip_empty go along in its call description
                res = s.own(self.ctx.topn_rescore(cand, call.weights[0], weighed, threshold, top_n, floors=call.floors,
                                                  skip_empty=call.skip_empty, primary=field(0) if call.skip_empty else None))
            self._record_count(states, call)
            # (_match_list_from_topn frees the result once the list is built; if it raises before that, the scope does)
            out = self._match_list_from_topn(res, state.matrix.dtype, B.shape[0], self_join_fix,
                                             keep_on_device or call.field_scores, t)
        if not call.field_scores:
            return out, None
        return self._record_planes(out, [field(0)] + fields, keep_on_device)

    @staticmethod
    def _record_matrices(state: CorpusState, others: List[CorpusState], B: DeviceMatrix,
                         B_fields: Optional[List[DeviceMatrix]], call: RecordCall):
        """(every field's corpus, every field's right-hand rows), checked against each other and against ``call``."""
        states, A = [state] + list(others), state.matrix
        self_join = B_fields is None          # (duplicates whose first Series is corpus.master have B is A and fields of their own)
        if len(states) != call.n_fields:
            raise ValueError(f"{len(states)} fields for a call of {call.n_fields}: one corpus a field is expected")
        if self_join and B is not A:
            raise ValueError("duplicates of the first field without duplicates of the further fields")
        for k, o in enumerate(others):
            if o.matrix.shape[0] != A.shape[0]:
                raise ValueError(f"the corpora differ in length ({o.matrix.shape[0]} and {A.shape[0]} rows): row p of every "
                                 f"corpus must be record p")
            if not self_join and B_fields[k].shape[0] != B.shape[0]:
                raise ValueError(f"the duplicates differ in length ({B_fields[k].shape[0]} and {B.shape[0]} rows)")
        return states, [B] + list(B_fields or [])   # (a self-join reads B alone, which is A)

    def _record_candidates(self, states: List[CorpusState], rights, call: RecordCall, self_join: bool, field) -> "N.TopN":
        """The candidates: the primary field's multiply, or every candidate field's and their union -- the fields' own
        results go as soon as they are united."""
        if not call.union:
            return self._topn_device(states[0].matrix, rights[0], *call.candidates[0])
        with N.Scope() as per_field:
            parts = []
            for f, (cand_top_n, cand_threshold) in zip(call.candidate_fields, call.candidates):
                A_f = states[f].matrix
                parts.append(per_field.own(self._topn_device(A_f, A_f if self_join else rights[f], cand_top_n, cand_threshold)))
            return self.ctx.topn_union(parts, field(0))

    @staticmethod
    def _record_count(states: List[CorpusState], call: RecordCall) -> None:
        for st in states:
            st.stats["record_calls"] += 1
            if call.floors is not None:
                st.stats["record_floor_calls"] += 1
            if call.field_scores:
                st.stats["record_field_score_calls"] += 1
            if call.skip_empty:
                st.stats["record_skip_empty_calls"] += 1
        for f in call.candidate_fields if call.union else ():
            states[f].stats["record_union_calls"] += 1

    def _record_planes(self, out, fields, keep_on_device: bool):
        """The list kept on the device (``out[4]``) scored field by field before it is freed or handed on."""
        kept = out[4]
        t = time.perf_counter()
        try:
            planes = kept.ml.field_scores(fields)
        except BaseException:
            kept.free()
            raise
        self.timings["field_scores_s"] = time.perf_counter() - t
        if keep_on_device:
            return out, planes
        kept.free()
        return out[:4], planes

    # ------------------------------------------------------------------ a self-join that is kept
    def corpus_keep_self_join(self, state: CorpusState, top_n: int, threshold: float) -> None:
        """From now on the self-join of the corpus with these two options is kept on the device and follows every append and
        remove; it is multiplied when a call first needs it.  Other values than the ones kept so far replace the result."""
        opts = (int(top_n), float(threshold))
        if state.kept_opts != opts:
            state.drop_kept()
        state.kept_opts = opts

    def corpus_drop_self_join(self, state: CorpusState) -> None:
        state.drop_kept()
        state.kept_opts = None

    def _kept_result(self, state: CorpusState) -> Optional["N.TopN"]:
        """The kept self-join, multiplied now if it is not there: the multiply a self-join of the corpus takes anyway."""
        if state.kept is None:
            top_n, threshold = state.kept_opts
            state.kept = self._corpus_against_indexes(state, state.matrix, top_n, threshold)
            if state.kept is not None:
                state.stats["self_join_full"] += 1
        return state.kept

    def _kept_copy(self, state: CorpusState) -> Optional["N.TopN"]:
        """What a served call gets: a copy it may free (callers free what _topn_device returns), never the kept object."""
        kept = self._kept_result(state)
        if kept is None:
            return None
        state.stats["self_join_served"] += 1
        return self.ctx.topn_concat_rows([kept])

    def _kept_old_rows_against(self, state: CorpusState, new: "N.Csr") -> Optional["N.TopN"]:
        """First half of an append's update, before the rows join: every old row's kept top-n merged (K5) with its top-n over
        the NEW rows -- the product of match_strings(master, new), by the same reverse-or-forward rule.  A row's top-n over a
        union of column sets is the merge of its top-n over each, and the new columns carry the highest numbers, so the order
        of equal scores (column ascending) holds across the boundary."""
        if state.kept is None:
            return None
        top_n, threshold = state.kept_opts
        n_old = state.matrix.shape[0]
        with state.updating_kept(), N.Scope() as s:
            over_new = s.own(self._topn_device(state.matrix, DeviceMatrix(new), top_n, threshold))
            return self.ctx.topn_zip([state.kept, over_new], np.array([0, n_old], dtype=np.int64), top_n)

    def _kept_add_new_rows(self, state: CorpusState, old_rows: "N.TopN", n_new: int) -> None:
        """Second half, after the rows have joined: the new rows -- the last ones of the last segment -- against the grown
        corpus, stacked under the old rows."""
        top_n, threshold = state.kept_opts
        state.drop_kept()
        with N.Scope() as s:
            last = state.segments[-1]
            view = s.own(last.csr.row_block(last.n_rows - n_new, last.n_rows))
            new_rows = s.own(self._corpus_against_indexes(state, DeviceMatrix(view), top_n, threshold))
            if new_rows is not None:                  # (None: the corpus has outgrown its indexes; stale)
                state.kept = self.ctx.topn_concat_rows([old_rows, new_rows])
                state.stats["self_join_append_updates"] += 1

    def _kept_forget(self, state: CorpusState, positions: np.ndarray) -> Optional["N.DeviceInts"]:
        """First half of a remove's update: the kept result without the rows and columns ``positions`` (live numbering).
        Returns the rows that were full and are not any more -- the only ones the cut may have hidden a candidate from -- as
        a list on the device, the caller's to free."""
        if state.kept is None:
            return None
        with N.Scope() as s:
            gone = s.own(self.ctx.upload_sorted_ints(positions))
            with state.updating_kept():
                left, short = self.ctx.topn_forget(state.kept, gone, state.kept_opts[0])
        state.drop_kept()
        state.kept = left
        return short

    def _kept_refill(self, state: CorpusState, short: "N.DeviceInts") -> None:
        """Second half, with the rows gone from the corpus: the short rows are taken from their segments, multiplied against
        the corpus's indexes (which over-ask for the dead rows and answer in live numbering) and written back."""
        top_n, threshold = state.kept_opts
        with state.updating_kept(), N.Scope() as s:
            if len(short):
                where = state.physical_rows(self.ctx.download_ints(short).astype(np.int64))
                taken, first = [], 0
                for seg in state.segments:
                    mine = where[(where >= first) & (where < first + seg.n_rows)] - first
                    if len(mine):
                        rows = s.own(self.ctx.upload_ints(mine))
                        taken.append(s.own(self.ctx.csr_take_rows(seg.csr, rows)))
                        s.release(rows)
                    first += seg.n_rows
                short_rows = taken[0] if len(taken) == 1 else s.own(self.ctx.csr_concat(taken))
                again = s.own(self._corpus_against_indexes(state, DeviceMatrix(short_rows), top_n, threshold))
                if again is None or again.dims()[1] > state.kept.dims()[1]:
                    state.drop_kept()                 # (the corpus has outgrown its indexes; stale)
                else:
                    self.ctx.topn_put_rows(state.kept, short, len(short), again)
                    state.stats["self_join_rows_refilled"] += len(short)
            state.stats["self_join_remove_updates"] += 1

