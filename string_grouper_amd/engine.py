"""Compute engine behind the StringGrouper front end: the MI355X library, nothing else.

The front end (string_grouper_amd/string_grouper.py) talks to an engine object with four
operations -- vectorise, wrap a host matrix, top-n multiply, blocked top-n multiply -- so that the
host logic can be unit-tested on a machine without a GPU by injecting a test double
(tests/_oracle_engine.py).  The product ships exactly one engine, ``HipEngine``; there is no CPU
engine in this package and ``get_engine()`` raises if the HIP library cannot be used.
"""
from __future__ import annotations

import os
import time
from typing import List, Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp

from . import _hostops
from . import _native as N
from .strprep import _ascii_lower
from .vectorizer import HipTfidfVectorizer


class DeviceMatrix:
    """A CSR matrix resident in HBM (rows = strings, columns = n-grams)."""

    def __init__(self, csr: "N.Csr"):
        self.csr = csr
        r, c, nnz, d = csr.dims()
        self.shape = (r, c)
        self.nnz = nnz
        self.dtype = N.code_np_dtype(d)
        self._host: Optional[sp.csr_matrix] = None

    def to_scipy(self) -> sp.csr_matrix:
        if self._host is None:
            self._host = self.csr.to_scipy()
        return self._host


def chunk_ranges(length: int, n_chunks: int) -> List[Tuple[int, int]]:
    """Contiguous ranges of ceil(length / n_chunks) rows (the reference's define_chunks,
    string_grouper.py:714-722)."""
    size = int(np.ceil(length / n_chunks))
    return [(lo, min(lo + size, length)) for lo in range(0, length, size)] if length > 0 else []


class DeviceMatchList:
    """The match list of one fit(), resident in HBM, for the reductions the reference runs over it:
    best master per duplicate (K7) and group representatives (K8)."""

    def __init__(self, ml: "N.MatchList", n_cols: int):
        self.ml = ml
        self.n_cols = n_cols

    def best_master(self) -> np.ndarray:
        return self.ml.best_master(self.n_cols)

    def group_reps(self, centroid: bool) -> np.ndarray:
        return self.ml.group_reps(centroid)

    def free(self):
        if self.ml is not None:
            self.ml.free()
            self.ml = None


class CorpusSegment:
    """A run of corpus rows and the inverted index over them (K3), built on first need.  The index borrows the arrays of the
    matrix it was built over (include/sg_hip.h: sg_postings_build), so the two live and die together: index first."""

    def __init__(self, csr: "N.Csr"):
        self.csr = csr
        self.index: Optional["N.Postings"] = None
        self.n_rows, _, self.nnz, _ = csr.dims()

    def free(self) -> None:
        for h in (self.index, self.csr):
            if h is not None:
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
    (HipEngine._corpus_topn), every call that reads the rows as one matrix compacts first (``rows``).

    A self-join that is kept (``Corpus.keep_self_join``): ``kept_opts`` is the (max_n_matches,
    min_similarity) it is kept for, ``kept`` the result over the LIVE rows -- None until the first call needs it, and again
    whenever an update could not follow a change (it is then multiplied anew on next need).  It is numbered by live rows, so a
    compaction does not touch it."""

    def __init__(self, vec: HipTfidfVectorizer, column, base: Optional["N.Csr"] = None, engine: Optional["HipEngine"] = None):
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
                      "self_join_remove_updates": 0, "self_join_rows_refilled": 0, "idf_refits": 0}
        if base is not None:
            self.set_segments(CorpusSegment(base), None)

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
                view = seg.csr.row_block(int(d) - first, int(d) - first + 1)
                total += view.dims()[2]
                view.free()
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


class HipEngine:
    name = "hip"
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

    def __init__(self, ctx: Optional[N.Context] = None):
        self._ctx = ctx
        # wall-clock split of the most recent fit() through this engine (seconds): host string preparation +
        # upload, device vectorise, device multiply + match list, download.  Read by bench.py (end_to_end).
        self.timings = {}

    def _tick(self, name: str, t0: float) -> float:
        now = time.perf_counter()
        self.timings[name] = self.timings.get(name, 0.0) + now - t0
        return now

    @property
    def ctx(self) -> N.Context:
        if self._ctx is None:
            self._ctx = N.default_context()
        return self._ctx

    # ------------------------------------------------------------------ seam b1
    def tfidf(self, master, duplicates, ngram_size, regex, ignore_case, normalize_to_ascii, dtype):
        """fit on master (+ duplicates), transform both (string_grouper.py:685-707).  One
        tokenisation pass per series: transform reuses the tokens of fit."""
        vec = HipTfidfVectorizer(ngram_size=ngram_size, regex=regex, ignore_case=ignore_case,
                                 normalize_to_ascii=normalize_to_ascii, dtype=dtype, ctx=self.ctx)
        self.timings = {}
        t = time.perf_counter()
        pm = vec.prepare(master)
        sets = [pm]
        if duplicates is not None:
            pd_ = vec.prepare(duplicates)
            sets.append(pd_)
        t = self._tick("prepare_and_upload_s", t)
        vec.fit_prepared(sets)
        A = DeviceMatrix(vec.transform_prepared(pm))
        B = A if duplicates is None else DeviceMatrix(vec.transform_prepared(sets[1]))
        self._tick("vectorise_s", t)             # fit_prepared reads the vocabulary back: a synchronisation point
        return A, B, vec

    def wrap(self, m) -> DeviceMatrix:
        if isinstance(m, DeviceMatrix):
            return m
        m = sp.csr_matrix(m)
        if m.dtype not in (np.float32, np.float64):
            m = m.astype(np.float64)
        d = DeviceMatrix(self.ctx.csr_from_scipy(m))
        return d

    # ------------------------------------------------------------------ resident corpus (string_grouper_amd/corpus.py)
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
        col = vec.prepare(strings)
        if col.kind == "symbols" and vec._alphabet is None:
            # characters beyond ASCII (normalize_to_ascii=False) against a vocabulary of ASCII n-grams: every n-gram with one
            # of them is out of vocabulary.  Each such character becomes one byte the corpus never had, so that the device
            # drops exactly those n-grams (its own treatment of bytes >= 0x80 would join the neighbours instead).
            col = self._corpus_bytes_column(state, col)
        csr = vec.transform_prepared(col)
        if col.dev is not None:
            col.dev.free()
        return csr

    @staticmethod
    def _corpus_bytes_column(state: CorpusState, col):
        from .strprep import StringColumn
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

    def corpus_append(self, state: CorpusState, strings) -> None:
        """The rows of ``strings`` (under the corpus's vocabulary and idf, as corpus_transform makes them) join the corpus
        behind its last row.  The cost follows the batch and the delta segment, not the corpus: the new rows are
        concatenated to the delta's (sg_csr_concat), whose index is dropped and rebuilt on first need; the base segment and
        its index are not touched until the delta outgrows CORPUS_COMPACT_SHARE of the base (corpus_compact)."""
        n_new = len(strings)
        if n_new == 0:
            return
        new = self._corpus_rows_of(state, strings)
        old_rows = self._kept_old_rows_against(state, new)          # (None: no self-join is kept)
        state.drop_whole()
        if state.delta is None:
            delta = CorpusSegment(new)
        else:
            delta = CorpusSegment(self.ctx.csr_concat([state.delta.csr, new]))
            state.delta.free()
            new.free()
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
        short = self._kept_forget(state, positions)                 # (None: no self-join is kept)
        state.set_dead(np.union1d(state.dead, state.physical_rows(positions)))
        state.stats["removals"] += 1
        state.stats["rows_removed"] += len(positions)
        if len(state.dead) > self.CORPUS_MAX_DEAD:
            self.corpus_compact(state)
        if short is not None:
            self._kept_refill(state, *short)

    def corpus_compact(self, state: CorpusState) -> None:
        """Fold the delta segment into the base and drop the dead rows: one matrix of the live rows (sg_csr_concat, then
        sg_csr_select_rows), one index (built on first need), and with them the self-join form of the multiply for a self-join
        of the corpus.  Nothing to do without a delta and without dead rows."""
        if state.delta is None and not len(state.dead):
            return
        whole = state.physical()
        if len(state.dead):
            live = self.ctx.csr_select_rows(whole, state.dead_dev)
            state.drop_whole()
            whole = live
        state.whole = None                    # (handed to the new base segment)
        old = state.segments
        state.set_dead(np.zeros(0, np.int64))
        state.set_segments(CorpusSegment(whole), None)
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
        new = state.vec.refit_idf_prepared(rows)
        old = state.segments
        state.set_segments(CorpusSegment(new), None)
        for seg in old:
            seg.free()
        state.drop_whole()
        state.drop_kept()
        state.stats["idf_refits"] += 1
        self.timings = dict(refit_rows_s=t1 - t0, **{f"refit_{k}_s": v for k, v in state.vec.last_refit_s.items()})

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

    def corpus_free(self, state: CorpusState) -> None:
        state.drop_whole()
        state.drop_kept()
        state.kept_opts = None
        if state.dead_dev is not None:
            state.dead_dev.free()
        state.dead_dev, state.dead = None, np.zeros(0, np.int64)
        for seg in state.segments if state.base is not None else []:
            seg.free()
        handles = [state.vec._vocab]
        for col in list(getattr(state.vec, "_fit_sets", [])) + list(getattr(state.vec, "_fit_originals", [])) + [state.column]:
            handles.append(getattr(col, "dev", None))
        for h in handles:
            if h is not None:
                h.free()
        state.vec._dev_of = {}
        state.base = state.delta = state.matrix = None

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
        parts = [self.ctx.spgemm_topn(A.csr, idx, ask, threshold, True) for idx, _, _ in segs]
        res = self._zip_segments(parts, segs, ask)
        return self._drop_dead(state, res, top_n) if n_dead else res

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
        try:
            over_new = self._topn_device(state.matrix, DeviceMatrix(new), top_n, threshold)
            try:
                return self.ctx.topn_zip([state.kept, over_new], np.array([0, n_old], dtype=np.int64), top_n)
            finally:
                over_new.free()
        except Exception:
            state.drop_kept()
            raise

    def _kept_add_new_rows(self, state: CorpusState, old_rows: "N.TopN", n_new: int) -> None:
        """Second half, after the rows have joined: the new rows -- the last ones of the last segment -- against the grown
        corpus, stacked under the old rows."""
        top_n, threshold = state.kept_opts
        state.drop_kept()
        view = new_rows = None
        try:
            last = state.segments[-1]
            view = last.csr.row_block(last.n_rows - n_new, last.n_rows)
            new_rows = self._corpus_against_indexes(state, DeviceMatrix(view), top_n, threshold)
            if new_rows is not None:                  # (None: the corpus has outgrown its indexes; stale)
                state.kept = self.ctx.topn_concat_rows([old_rows, new_rows])
                state.stats["self_join_append_updates"] += 1
        finally:
            for h in (new_rows, view, old_rows):
                if h is not None:
                    h.free()

    def _kept_forget(self, state: CorpusState, positions: np.ndarray):
        """First half of a remove's update: the kept result without the rows and columns ``positions`` (live numbering), and
        the rows that were full and are not any more -- (device pointer, how many) -- the only ones the cut may have hidden
        a candidate from."""
        if state.kept is None:
            return None
        gone = self.ctx.upload_sorted_ints(positions)
        try:
            left, d_short, n_short = self.ctx.topn_forget(state.kept, gone, state.kept_opts[0])
        except Exception:
            state.drop_kept()
            raise
        finally:
            gone.free()
        state.drop_kept()
        state.kept = left
        return d_short, n_short

    def _kept_refill(self, state: CorpusState, d_short: int, n_short: int) -> None:
        """Second half, with the rows gone from the corpus: the short rows are taken from their segments, multiplied against
        the corpus's indexes (which over-ask for the dead rows and answer in live numbering) and written back."""
        top_n, threshold = state.kept_opts
        made = []
        try:
            if n_short:
                where = state.physical_rows(self.ctx.download_ints(d_short, n_short).astype(np.int64))
                first = 0
                for seg in state.segments:
                    mine = where[(where >= first) & (where < first + seg.n_rows)] - first
                    if len(mine):
                        rows = self.ctx.upload_ints(mine)
                        made.append(self.ctx.csr_take_rows(seg.csr, rows))
                        rows.free()
                    first += seg.n_rows
                if len(made) > 1:
                    made.append(self.ctx.csr_concat(made))
                again = self._corpus_against_indexes(state, DeviceMatrix(made[-1]), top_n, threshold)
                if again is None or again.dims()[1] > state.kept.dims()[1]:
                    state.drop_kept()                 # (the corpus has outgrown its indexes; stale)
                else:
                    self.ctx.topn_put_rows(state.kept, d_short, n_short, again)
                    state.stats["self_join_rows_refilled"] += n_short
                if again is not None:
                    again.free()
            state.stats["self_join_remove_updates"] += 1
        except Exception:
            state.drop_kept()
            raise
        finally:
            self.ctx.device_free(d_short)
            for h in reversed(made):
                h.free()

    def _zip_segments(self, parts: List["N.TopN"], segs, top_n: int) -> "N.TopN":
        """The results against the segments' indexes as one over the corpus's rows: columns offset by the segment's first
        row, merged by score descending, then row ascending (K5), cut at top_n."""
        if len(parts) == 1:
            return parts[0]
        res = self.ctx.topn_zip(parts, np.array([first for _, first, _ in segs], dtype=np.int64), top_n)
        for p in parts:
            p.free()
        return res

    def _drop_dead(self, state: CorpusState, res: "N.TopN", top_n: int) -> "N.TopN":
        """``res`` over the segments' physical rows as the result over the live rows: dead columns out, the others
        renumbered, rows cut at top_n (sg_topn_drop_columns).  ``res`` is freed."""
        live = self.ctx.topn_drop_columns(res, state.dead_dev, top_n)
        res.free()
        return live

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
        parts, slots = [], 0                  # slots: what the complete parts so far hold per new row
        for idx, _, n_seg in segs:
            cap = self.CORPUS_FIRST_CAP
            while True:
                stride = min(cap, n_seg)
                if n_new * (slots + stride) > self.CORPUS_PAIR_BUDGET:
                    for p in parts:
                        p.free()
                    return None
                pairs = self.ctx.spgemm_topn(B.csr, idx, stride, threshold, True)
                cnt = pairs.counts()
                if stride >= n_seg or int(cnt.max()) < stride:
                    break
                pairs.free()
                cap *= 8
            parts.append(pairs)
            slots += stride
        pairs = self._zip_segments(parts, segs, slots)      # asked for the sum of the strides: nothing is cut
        if len(state.dead):                   # (a dead row counted towards a full row and the budget like any other)
            pairs = self._drop_dead(state, pairs, pairs.dims()[1])
        res = self.ctx.topn_transpose_select(pairs, n_corpus, top_n)
        pairs.free()
        return res

    # ------------------------------------------------------------------ seam b2
    def _topn_device(self, A: DeviceMatrix, B: DeviceMatrix, top_n: int, threshold: float) -> "N.TopN":
        """Top-n multiply with the result left on the device.  One inverted index normally; when the
        right-hand side is too large for one (SG_ERR_OVERFLOW -> OverflowError, what the reference's
        fit() reacts to by splitting, string_grouper.py:397-413) it is cut into the fewest row blocks that
        fit and the partial results are merged on the device (K5 = zip_sp_matmul_topn).  A resident corpus on
        either side: _corpus_topn."""
        ctx = self.ctx
        if isinstance(A, CorpusMatrix) or isinstance(B, CorpusMatrix):
            res = self._corpus_topn(A, B, top_n, threshold)
            if res is not None:
                return res
        try:
            post = ctx.postings_build(B.csr)
        except OverflowError:
            post = None
        if post is not None:
            res = ctx.spgemm_topn(A.csr, post, top_n, threshold, True)
            post.free()
            return res
        n_blocks = 2
        while True:
            ranges = chunk_ranges(B.shape[0], n_blocks)
            views, posts = [], []
            try:
                for lo, hi in ranges:
                    v = B.csr.row_block(lo, hi)
                    views.append(v)
                    posts.append(ctx.postings_build(v))
                break
            except OverflowError:
                for h in posts + views:
                    h.free()
                n_blocks *= 2
                if n_blocks > max(B.shape[0], 2):
                    raise
        parts = [ctx.spgemm_topn(A.csr, p, top_n, threshold, True) for p in posts]
        res = ctx.topn_zip(parts, np.array([lo for lo, _ in ranges], dtype=np.int64), top_n)
        for h in parts + posts + views:
            h.free()
        return res

    def topn_multiply(self, A: DeviceMatrix, B: DeviceMatrix, top_n: int, threshold: float) -> sp.csr_matrix:
        """sp_matmul_topn(A, B.T, top_n, threshold, sort=True) (string_grouper.py:725-732)."""
        res = self._topn_device(A, B, top_n, threshold)
        C = res.to_scipy()
        C = sp.csr_matrix((C.data, C.indices, C.indptr), shape=(A.shape[0], B.shape[0]))
        res.free()
        return C

    def rowwise_dot(self, A: DeviceMatrix, B: DeviceMatrix) -> np.ndarray:
        """Row-wise similarity of master and duplicates (string_grouper.py:433-440) on the device (K9)."""
        return self.ctx.rowwise_dot(A.csr, B.csr)

    # ------------------------------------------------------------------ fused tail of fit() (K6)
    def match_list(self, A: DeviceMatrix, B: DeviceMatrix, top_n: int, threshold: float, self_join_fix: bool,
                   keep_on_device: bool = False):
        """Multiply and build the match list without leaving the device: (master_side, dupe_side,
        similarity, true_max_n_matches).  ``self_join_fix``: set the diagonal to 1 and symmetrise
        (string_grouper.py:419-427); the rows then come back sorted by column.  ``keep_on_device``: a fifth
        element, the device-resident list (``DeviceMatchList``), for the reductions over it (K7, K8)."""
        t = time.perf_counter()
        res = self._topn_device(A, B, top_n, threshold)
        return self._match_list_from_topn(res, A.dtype, B.shape[0], self_join_fix, keep_on_device, t)

    def _match_list_from_topn(self, res: "N.TopN", dtype, n_cols: int, self_join_fix: bool, keep_on_device: bool,
                              t: float):
        cnt = res.counts()
        true_max = int(cnt.max()) if len(cnt) else 0
        t = self._tick("multiply_s", t)           # counts() waits for the multiply
        # the reference up-casts a float32 result to float64 through scipy (vstack(dtype=float64), :750),
        # which re-sorts every row by column; a float64 result keeps the multiply's score-descending order
        ml = self.ctx.matchlist_build(res, self_join_fix, self_join_fix,
                                      sort_by_column=(not self_join_fix) and dtype == np.float32)
        if os.environ.get("SG_E2E_SPLIT"):            # (diagnostic: the list's kernels and its download apart)
            self.ctx.sync()
            t_ml = time.perf_counter()
            self.timings["match_list_kernels_s"] = t_ml - t
        row_ptr, cols, vals = ml.to_host()
        t = self._tick("match_list_and_download_s", t)
        res.free()
        # (round 6: the three expansions on host threads -- _hostops; numpy's own below 262 144 entries or without the helpers)
        rows = _hostops.expand_rows(row_ptr)
        cols = _hostops.widen(cols, np.int64)
        if keep_on_device:
            return rows, cols, vals, true_max, DeviceMatchList(ml, n_cols)
        ml.free()
        return rows, cols, vals, true_max

    def topn_multiply_blocked(self, A: DeviceMatrix, B: DeviceMatrix, n_blocks: Tuple[int, int], top_n: int,
                              threshold: float) -> sp.csr_matrix:
        """Block-pair products, zipped over right blocks, stacked over left blocks
        (string_grouper.py:733-752)."""
        ctx = self.ctx
        a_ranges = chunk_ranges(A.shape[0], n_blocks[0])
        b_ranges = chunk_ranges(B.shape[0], n_blocks[1])
        b_views = [B.csr.row_block(lo, hi) for lo, hi in b_ranges]
        b_posts = [ctx.postings_build(v) for v in b_views]
        offsets = np.array([lo for lo, _ in b_ranges], dtype=np.int64)
        stacked = []
        for lo, hi in a_ranges:
            a_view = A.csr.row_block(lo, hi)
            parts = [ctx.spgemm_topn(a_view, p, top_n, threshold, True) for p in b_posts]
            if len(parts) == 1:
                stacked.append(parts[0].to_scipy())
            else:
                z = ctx.topn_zip(parts, offsets, top_n)
                C = z.to_scipy()
                stacked.append(sp.csr_matrix((C.data, C.indices, C.indptr), shape=(hi - lo, B.shape[0])))
                z.free()
            for p in parts:
                p.free()
            a_view.free()
        for p in b_posts:
            p.free()
        for v in b_views:
            v.free()
        if not stacked:
            return sp.csr_matrix((A.shape[0], B.shape[0]), dtype=np.float64)
        return sp.vstack(stacked, dtype=np.float64).tocsr()


class ShardedMatrix(DeviceMatrix):
    """This rank's contiguous row block of a TF-IDF matrix whose other rows live on the other ranks.  ``shape`` is
    the shape of the WHOLE matrix (what the front end reasons about); ``csr`` holds rows [lo, hi)."""

    def __init__(self, csr: "N.Csr", n_total: int, row_range: Tuple[int, int], ops, group):
        super().__init__(csr)
        self.local_shape = self.shape
        self.shape = (n_total, self.shape[1])
        self.row_range = row_range
        self._ops, self._group = ops, group
        self._full: Optional["N.Csr"] = None

    def full(self) -> "N.Csr":
        """The whole matrix on this rank (one all-gather of the ranks' blocks, cached)."""
        if self._full is None:
            from . import distributed as D
            self._full = D.replicate_csr(self._ops, self.csr, self._group)
        return self._full

    def to_scipy(self) -> sp.csr_matrix:
        if self._host is None:
            self._host = self.full().to_scipy()
        return self._host


class DistributedHipEngine(HipEngine):
    """The engine behind ``fit()`` when the process is one rank of a ``torch.distributed`` group (one process per
    GPU, RCCL): every rank runs the SAME script on the SAME input Series and gets the SAME results.  The ranks split
    the rows of every string column (vectorise), all-reduce the document frequencies, all-gather the right-hand
    TF-IDF rows, multiply their block of left rows and all-gather the fixed-stride results, which are concatenated
    on the host (string_grouper.py:750 vstack) -- string_grouper_amd/distributed.py.  The tail of fit() (match
    list, groups) then runs on every rank's GPU over the whole result, as on one GPU."""
    name = "hip-distributed"

    def __init__(self, ctx: Optional[N.Context] = None, group=None):
        super().__init__(ctx)
        self.group = group

    def tfidf(self, master, duplicates, ngram_size, regex, ignore_case, normalize_to_ascii, dtype):
        import torch.distributed as dist
        from . import distributed as D
        rank, world = dist.get_rank(self.group), dist.get_world_size(self.group)

        def factory():
            return HipTfidfVectorizer(ngram_size=ngram_size, regex=regex, ignore_case=ignore_case,
                                      normalize_to_ascii=normalize_to_ascii, dtype=dtype, ctx=self.ctx)
        ops = D.HipOps(self.ctx, factory)
        self.timings = {}
        t = time.perf_counter()
        probe = factory()
        ranges, blocks = [], []
        for series in ([master] if duplicates is None else [master, duplicates]):
            lo, hi = D.row_block(rank, world, len(series))
            ranges.append((lo, hi))
            blocks.append(probe.prepare(series.iloc[lo:hi] if hasattr(series, "iloc") else series[lo:hi]))
        t = self._tick("prepare_and_upload_s", t)
        try:
            vec, mats = D.sharded_tfidf(ops, blocks, self.group)
        except D.ShardedFitNotApplicable:
            # (raised on every rank alike.)  n-gram keys coded over the alphabet of the strings at hand -- ngram_size > 3,
            # characters kept by normalize_to_ascii=False -- mean something else on every rank: every rank vectorises the
            # WHOLE columns (it holds them: the public API runs the same script on the same Series everywhere), and only
            # the multiply is shared: this rank's rows on the left, the whole matrix, which is already here, on the right.
            return self._tfidf_replicated(master, duplicates, factory, ops, ranges, t)
        self._tick("vectorise_s", t)
        A = ShardedMatrix(mats[0], len(master), ranges[0], ops, self.group)
        B = A if duplicates is None else ShardedMatrix(mats[1], len(duplicates), ranges[1], ops, self.group)
        return A, B, vec

    def _tfidf_replicated(self, master, duplicates, factory, ops, ranges, t):
        vec = factory()
        sets = [vec.prepare(master)] + ([] if duplicates is None else [vec.prepare(duplicates)])
        vec.fit_prepared(sets)
        full = [vec.transform_prepared(s) for s in sets]
        self._tick("vectorise_s", t)
        out = []
        for csr, (lo, hi) in zip(full, ranges):
            m = ShardedMatrix(csr.row_block(lo, hi), csr.dims()[0], (lo, hi), ops, self.group)
            m._full = csr                      # no all-gather: the whole matrix is this rank's own work
            out.append(m)
        return out[0], (out[0] if duplicates is None else out[1]), vec

    def _topn_device(self, A, B, top_n: int, threshold: float) -> "N.TopN":
        if not isinstance(A, ShardedMatrix):
            # replicated left side: every rank does it all -- against the WHOLE right-hand side, not this rank's block of it
            if isinstance(B, ShardedMatrix):
                B = DeviceMatrix(B.full())
            return super()._topn_device(A, B, top_n, threshold)
        from . import distributed as D
        right = B.full() if isinstance(B, ShardedMatrix) else B.csr
        try:
            res_local = D.sharded_topn(A._ops, A.csr, right, top_n, threshold, self_join=B is A, group=self.group)
        except OverflowError:
            # the right-hand side does not fit one inverted index (on every rank alike: it is the same matrix): the local
            # rows against row blocks of it, merged on the device (K5), as on one GPU and as fit() expects of the engine
            # (string_grouper.py:397-413)
            res_local = HipEngine._topn_device(self, DeviceMatrix(A.csr), DeviceMatrix(right), top_n, threshold)
        cols, vals, counts = D.gather_topn(A._ops, res_local, self.group, on_device=True)
        res_local.free()
        return A._ops.topn_from_tensors(cols, vals, counts, B.shape[0])

    def rowwise_dot(self, A, B) -> np.ndarray:
        """Row-wise similarity: local rows on the device (K9), the ranks' pieces concatenated."""
        if not isinstance(A, ShardedMatrix):
            return super().rowwise_dot(A, B)
        import torch
        from . import distributed as D
        local = self.ctx.rowwise_dot(A.csr, B.csr)
        parts = D.all_gather_ragged(torch.from_numpy(np.ascontiguousarray(local)).to(A._ops.device), self.group)
        return torch.cat(parts).cpu().numpy()

    def topn_multiply_blocked(self, A, B, n_blocks, top_n, threshold):
        if isinstance(A, ShardedMatrix):          # explicit n_blocks only cut the work differently: same result
            return self.topn_multiply(A, B, top_n, threshold).astype(np.float64)
        return super().topn_multiply_blocked(A, B, n_blocks, top_n, threshold)


def enable_distributed(group=None, ctx: Optional[N.Context] = None) -> "HipEngine":
    """Make fit() of this process use all ranks of the (already initialised) ``torch.distributed`` process group.
    Call on every rank after ``dist.init_process_group("nccl")`` and ``torch.cuda.set_device(local_rank)``."""
    import torch.distributed as dist
    N.lib()
    eng = DistributedHipEngine(ctx, group) if dist.is_initialized() and dist.get_world_size(group) > 1 else HipEngine(ctx)
    set_engine(eng)
    return eng


_engine = None


def get_engine():
    """The process-wide engine.  Raises (ImportError / RuntimeError) when libsg_hip.so is missing or
    no MI355X is visible -- the package never substitutes a CPU implementation."""
    global _engine
    if _engine is None:
        N.lib()
        _engine = HipEngine()
    return _engine


def set_engine(engine) -> None:
    """Test hook: inject an engine double (tests/_oracle_engine.py).  Not used by the product."""
    global _engine
    _engine = engine
