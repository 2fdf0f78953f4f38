"""A fitted corpus that stays on the GPU: match new strings against it without refitting.

The reference documents this use (``sg = StringGrouper(master)``, then ``sg.match_strings(new_master)`` "using the corpus
already built above without rebuilding or changing it in any way", docs/references/sg_class.md Example 1) but its code
refits on master + duplicates every call (string_grouper.py:685-707), and so does ``StringGrouper`` here.  ``Corpus`` is
the fixed-corpus form:

    corpus = Corpus(master)                      # vocabulary + idf of TfidfVectorizer(...).fit(master), once
    corpus.match_strings(master, new_batch)      # new_batch.transform()ed with them; master's rows and index are resident

A corpus may grow: ``corpus.append(new_strings)`` puts new rows behind the last one, transformed with the SAME vocabulary and
idf (nothing is refitted, no score between two old rows changes), ``corpus.master`` is then the longer Series.  And it may
forget: ``corpus.remove(rows)`` takes rows out, ``corpus.master`` is then the shorter Series and row numbers count through
it; vocabulary and idf stay what the original list gave -- until ``corpus.refit_idf()``, which makes the idf follow the
CURRENT list on the device without reading a string again (the vocabulary is still the original's; only a new ``Corpus`` learns
new n-grams).

A service that asks after every change which group each record belongs to now -- ``corpus.group_similar_strings(corpus.master)``
-- may have the corpus keep that self-join on the device: ``corpus.keep_self_join()``.  ``append`` and ``remove`` then edit the
kept result with work that follows the change, and the call is served from it, bit for bit what the whole multiply gives.

Every Series a method receives is transformed with the corpus's vocabulary and idf (an n-gram the corpus never had is
dropped, as sklearn's transform drops it); everything after that is what ``StringGrouper.fit()`` and its frames do with the
two matrices.  The methods have the signatures of the module-level functions (string_grouper.py:55-153).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import pandas as pd

from . import engine as _engine_mod
from .pairs import checked_pairs
from .record_call import MAX_RECORD_CANDIDATES, MAX_RECORD_FIELDS, RecordCall, checked_record_call
from .string_grouper import StringGrouper, StringGrouperConfig

# options that define the vectoriser: a call may not change them (the corpus was fitted with them)
VECTORISER_OPTIONS = ("ngram_size", "regex", "ignore_case", "normalize_to_ascii", "tfidf_matrix_dtype")


class _GrowingSeries:
    """A Series that grows at its end: ``pd.concat([series] + parts)`` without copying the old rows every time.  pd.concat
    costs what the WHOLE list costs (9 ms at 663 k strings, and as much again to drop the old copy) -- per append that was
    more than everything the device does.  Object-dtype values (and int64 labels) are kept in buffers with spare capacity;
    every joined Series is a view of the buffer's head, which later appends never write to.  Anything else (extension
    dtypes, other label types) is joined by pandas."""

    def __init__(self, series: pd.Series):
        self.series = series
        self._values: Optional[np.ndarray] = None
        self._labels: Optional[np.ndarray] = None

    @staticmethod
    def _room(buffer, old: np.ndarray, total: int, dtype) -> np.ndarray:
        if buffer is not None and total <= len(buffer):
            return buffer
        grown = np.empty(total + total // 2 + 1024, dtype=dtype)
        grown[:len(old)] = old
        return grown

    def extend(self, parts) -> pd.Series:
        s = self.series
        if s.dtype != object or any(p.dtype != object for p in parts):
            self.series, self._values, self._labels = pd.concat([s] + list(parts)), None, None
            return self.series
        n, total = len(s), len(s) + sum(len(p) for p in parts)
        self._values = self._room(self._values, s.to_numpy(), total, object)
        plain = all(type(x.index) in (pd.Index, pd.RangeIndex) and x.index.dtype == np.int64 for x in [s] + list(parts))
        if plain:
            self._labels = self._room(self._labels, s.index.to_numpy(), total, np.int64)
        at = n
        for p in parts:
            self._values[at:at + len(p)] = p.to_numpy()
            if plain:
                self._labels[at:at + len(p)] = p.index.to_numpy()
            at += len(p)
        if plain:
            index = pd.Index(self._labels[:total], name=s.index.name if all(p.index.name == s.index.name for p in parts) else None)
        else:
            index, self._labels = s.index.append([p.index for p in parts]), None
        name = s.name if all(p.name == s.name for p in parts) else None
        self.series = pd.Series(self._values[:total], index=index, name=name, copy=False)
        return self.series

    @staticmethod
    def _kept(old: np.ndarray, keep: np.ndarray, drop: np.ndarray, total: int, dtype) -> np.ndarray:
        """``old[keep]`` at the head of a new buffer with spare capacity.  Between two dropped rows the kept ones are
        contiguous: a few dropped rows are a few slice copies (7.5 ms a remove at 663 k strings where np.compress took 17)."""
        fresh = np.empty(total + total // 2 + 1024, dtype=dtype)
        if len(drop) > 4096:
            fresh[:total] = old[keep]
            return fresh
        src = dst = 0
        for d in drop.tolist() + [len(old)]:
            fresh[dst:dst + d - src] = old[src:d]
            dst += d - src
            src = d + 1
        return fresh

    def without(self, keep: np.ndarray) -> pd.Series:
        """``series[keep]`` (a boolean mask) as the new Series.  The Series handed out so far are views of the buffers'
        heads, so nothing is moved inside them: the kept rows are copied into NEW buffers (with room for the appends that
        follow), the old ones live on with whoever holds an old Series.  This costs what the whole list costs."""
        s = self.series
        if s.dtype != object:
            self.series, self._values, self._labels = s[keep], None, None
            return self.series
        total = int(np.count_nonzero(keep))
        drop = np.flatnonzero(~keep)
        self._values = self._kept(s.to_numpy(), keep, drop, total, object)
        if type(s.index) in (pd.Index, pd.RangeIndex) and s.index.dtype == np.int64:
            self._labels = self._kept(s.index.to_numpy(), keep, drop, total, np.int64)
            index = pd.Index(self._labels[:total], name=s.index.name)
        else:
            index, self._labels = s.index[keep], None
        self.series = pd.Series(self._values[:total], index=index, name=s.name, copy=False)
        return self.series


class _CorpusGrouper(StringGrouper):
    """StringGrouper whose TF-IDF matrices come from the corpus (transform only) instead of a fit on its inputs."""

    def __init__(self, corpus: "Corpus", master, duplicates=None, master_id=None, duplicates_id=None, **kwargs):
        self._corpus = corpus
        self._made = []
        super().__init__(master, duplicates, master_id, duplicates_id, **kwargs)

    def _tfidf_on_engine(self):
        A = self._corpus._rows_of(self._master, self._made)
        if self._duplicates is None or self._duplicates is self._master:
            B = A
        else:
            B = self._corpus._rows_of(self._duplicates, self._made)
        self._vectorizer = self._corpus.vectorizer
        return A, B

    def _release(self):
        self._drop_device_matches()
        for m in self._made:
            csr = getattr(m, "csr", None)
            if csr is not None:
                csr.free()
        self._made = []


class _RecordGrouper(_CorpusGrouper):
    """_CorpusGrouper whose match list is the engine's over RECORDS: the corpus finds the candidates, further corpora score them
    on their fields, and the weighed sum is what the list holds (CorpusEngine.corpus_records).  Everything behind the list --
    the frames, the groups -- is StringGrouper's own."""

    def __init__(self, corpus: "Corpus", others, call: RecordCall, dup_fields, master, duplicates=None, master_id=None,
                 duplicates_id=None, **kwargs):
        """``call``: the description of the call (string_grouper_amd/record_call.py), handed to the engine as it is."""
        self._others, self._call, self._dup_fields = others, call, dup_fields
        self._planes = None
        super().__init__(corpus, master, duplicates, master_id, duplicates_id, **kwargs)

    def _can_fuse_on_device(self) -> bool:
        return True                           # (explicit n_blocks were refused by the caller; there is no host route)

    def fit(self):
        """StringGrouper's, and with ``field_scores`` the planes as further columns ``similarity_k`` of the match list
        (float64, as ``similarity`` is).  They are added in place: the list on the device stays with the grouper."""
        self._planes = None
        super().fit()
        if self._call.field_scores:
            ml = self._matches_list
            for k, plane in enumerate(self._planes):
                ml[f'similarity_{k}'] = plane.astype(np.float64, copy=False)
            self._planes = None
        return self

    def get_matches(self, ignore_index: Optional[bool] = None, include_zeroes: Optional[bool] = None) -> pd.DataFrame:
        """StringGrouper's frame, and with ``field_scores`` the columns ``similarity_k`` right after ``similarity``.  The rows
        ``include_zeroes`` adds come after the list's own, in the frame as in the list, and carry 0.0 in every field column
        as they carry 0 in ``similarity``."""
        frame = super().get_matches(ignore_index=ignore_index, include_zeroes=include_zeroes)
        if not self._call.field_scores:
            return frame
        ml = self._matches_list
        at = list(frame.columns).index('similarity') + 1
        for k in range(len(self._others) + 1):
            column = np.zeros(len(frame), np.float64)
            column[:len(ml)] = ml[f'similarity_{k}'].to_numpy()
            frame.insert(at + k, f'similarity_{k}', column)
        return frame

    def _engine_match_list(self, eng, master_matrix, duplicate_matrix, fix: bool):
        """One engine call: the list as ``match_list`` gives it, kept on the device, and with ``field_scores`` the planes,
        one a field, in list order (taken by ``fit``)."""
        call = self._call
        fields = None
        if self._dup_fields is not None:                             # one transform a field (duplicates[0] may be corpus.master)
            fields = [o._rows_of(series, self._made) for o, series in zip(self._others, self._dup_fields)]
        top_n = call.all_candidates if self._max_n_matches is None else min(int(self._max_n_matches), call.all_candidates)
        try:
            out, self._planes = eng.corpus_records(self._corpus._live(), [o._live() for o in self._others], duplicate_matrix,
                                                   fields, call, top_n, self._config.min_similarity, fix, keep_on_device=True)
            return out
        except OverflowError as e:
            # fit() answers an OverflowError with the block-wise multiply of ONE field: that is no record match.  There is no
            # block-wise route for records, so the call is refused instead
            now = (f"{[k for k, _ in call.candidates]} on the fields {list(call.candidate_fields)}" if call.union else
                   f"{call.candidates[0][0]}")
            raise ValueError(f"records x candidates exceed what one result on the device can index ({e}): lower "
                             f"candidates['max_n_matches'] (now {now}) or match the records in batches of duplicates") from e


class Corpus:
    """A master list fitted once and kept on the device; see the module docstring."""
    MAX_RECORD_FIELDS = MAX_RECORD_FIELDS     # (string_grouper_amd/record_call.py)
    MAX_RECORD_CANDIDATES = MAX_RECORD_CANDIDATES

    def __init__(self, master: pd.Series, master_id: Optional[pd.Series] = None, **kwargs):
        StringGrouper(master, master_id=master_id, **kwargs)        # the reference's validation of data and options
        self._config = StringGrouperConfig(**kwargs)
        eng = _engine_mod.get_engine()
        if isinstance(eng, _engine_mod.DistributedHipEngine):
            raise NotImplementedError("Corpus is single-GPU: it cannot be used after engine.enable_distributed()")
        if not hasattr(eng, "corpus_fit"):
            raise NotImplementedError(f"the engine {getattr(eng, 'name', type(eng).__name__)!r} keeps no corpus")
        self._engine = eng
        self._master = master
        self._master_id = master_id
        self._pending = []                    # (strings, ids) appended since ``master`` was last asked for
        self._grown = _GrowingSeries(master)
        self._grown_id = _GrowingSeries(master_id) if master_id is not None else None
        cfg = self._config
        self._state = eng.corpus_fit(master, cfg.ngram_size, cfg.regex, cfg.ignore_case, cfg.normalize_to_ascii,
                                     cfg.tfidf_matrix_dtype)

    # ------------------------------------------------------------------ resources
    def close(self) -> None:
        """Free everything the corpus holds on the device (vocabulary, idf, its rows and indexes, segment by segment, a kept
        self-join)."""
        if self._state is not None:
            self._engine.corpus_free(self._state)
            self._state = None

    def __enter__(self) -> "Corpus":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if self._state is None:
            raise ValueError("the corpus is closed")
        return self._state

    @property
    def master(self) -> pd.Series:
        """The corpus's strings: the Series it was built from, or after an append the concatenation of the parts (a new
        object after every append).  Only THIS object stands for the resident rows in a call; any other Series -- an older
        ``corpus.master`` included -- is transformed like a batch (the same result, just slower)."""
        self._join_pending()
        return self._master

    @property
    def master_id(self) -> Optional[pd.Series]:
        """The ids that go with ``master`` (None when the corpus was built without)."""
        self._join_pending()
        return self._master_id

    def _join_pending(self) -> None:
        if self._pending:
            self._master = self._grown.extend([s for s, _ in self._pending])
            if self._master_id is not None:
                self._master_id = self._grown_id.extend([i for _, i in self._pending])
            self._pending = []

    # ------------------------------------------------------------------ growing
    def append(self, new_strings: pd.Series, new_ids: Optional[pd.Series] = None) -> None:
        """Put ``new_strings`` behind the corpus's last row; ``new_ids`` is required when the corpus has ``master_id`` and
        refused when it has none.  An empty Series changes nothing.

        The vocabulary and the idf do NOT change: the new strings are transformed as every batch is (n-grams the corpus
        never had are dropped; a string with none it knows is an empty row that still matches itself in a self-join), and
        every result afterwards is what ``TfidfVectorizer.fit(original master).transform(all strings)`` gives, row numbers
        counting through the concatenated list.  The idf therefore drifts from what a refit on the grown list would give;
        ``refit_idf()`` brings the idf up to the current list (the vocabulary stays), ``Corpus(corpus.master,
        corpus.master_id)`` is the whole refit, new n-grams included.  The cost follows the batch, not the corpus: the new rows
        wait in a second segment with an index of its own, which is folded into the first once it exceeds
        ``engine.HipEngine.CORPUS_COMPACT_SHARE`` of it (or by ``compact()``).  ``remove`` takes rows out again."""
        state = self._live()
        self._same_engine()
        if not hasattr(self._engine, "corpus_append"):
            raise NotImplementedError(f"the engine {getattr(self._engine, 'name', type(self._engine).__name__)!r} grows no corpus")
        if not StringGrouper._is_series_of_strings(new_strings):
            raise TypeError('Appended input does not consist of pandas.Series containing only Strings')
        if self._master_id is None and new_ids is not None:
            raise ValueError("the corpus has no master_id: new_ids cannot be kept")
        if self._master_id is not None and new_ids is None:
            raise ValueError("the corpus has master_id: new_ids is required")
        if new_ids is not None and (not isinstance(new_ids, pd.Series) or len(new_ids) != len(new_strings)):
            raise Exception('Both new_strings and new_ids must be pandas.Series of the same length.')
        if len(new_strings) == 0:
            return
        self._engine.corpus_append(state, new_strings)
        # the Series are joined when they are next asked for: a run of appends copies the list once, not once per append
        self._pending.append((new_strings, new_ids))

    # ------------------------------------------------------------------ forgetting
    def _positions(self, rows, n: int) -> np.ndarray:
        """``rows`` of ``remove`` as sorted distinct positions in [0, n)."""
        if isinstance(rows, (bool, np.bool_)):
            raise TypeError("rows must be positions (an int or a sequence of ints) or a boolean mask, not a single bool")
        if isinstance(rows, (int, np.integer)):
            rows = [int(rows)]
        try:
            arr = np.asarray(rows)
        except Exception:
            raise TypeError("rows must be positions (an int or a sequence of ints) or a boolean mask")
        if arr.ndim != 1:
            raise TypeError("rows must be one-dimensional: positions or a boolean mask")
        if arr.dtype == bool:
            if len(arr) != n:
                raise IndexError(f"the boolean mask has {len(arr)} entries, the corpus has {n} rows")
            return np.flatnonzero(arr).astype(np.int64)
        if arr.size == 0:
            return np.zeros(0, np.int64)
        if arr.dtype.kind not in "iu":
            raise TypeError(f"rows must be integer positions or a boolean mask, not {arr.dtype}")
        arr = arr.astype(np.int64)
        if arr.min() < -n or arr.max() >= n:
            raise IndexError(f"a position lies outside [{-n}, {n}): the corpus has {n} rows")
        return np.unique(np.where(arr < 0, arr + n, arr))

    def remove(self, rows) -> None:
        """Take rows out of the corpus.  ``rows``: positions in the CURRENT ``corpus.master`` -- an int, a sequence or array
        of ints (negative ones count from the end, a position named twice is removed once) or a boolean mask of its
        length.  Afterwards ``corpus.master`` (and ``master_id``) is ``master[keep]``, a new object: the other rows in their
        old order with their labels, and row numbers in every later result count through that shorter list.  Nothing named
        changes nothing; removing every row is refused (build a new corpus).  To remove by id:
        ``corpus.remove(np.flatnonzero(corpus.master_id.isin(ids)))``.

        The vocabulary and the idf do NOT change (nor the number of documents behind the idf): every result afterwards is
        what ``TfidfVectorizer.fit(original master).transform(remaining strings)`` gives, and an n-gram whose last row went
        away keeps its column.  ``refit_idf()`` brings the idf up to the remaining list, ``Corpus(corpus.master,
        corpus.master_id)`` is the whole refit.  On the device a removed row stays
        where it is until the next compaction (more than ``engine.HipEngine.CORPUS_MAX_DEAD`` of them, an append's share
        rule, ``compact()``, or a call that needs all rows in one matrix); on the host the Series is copied without it,
        which costs what the list costs."""
        state = self._live()
        self._same_engine()
        if not hasattr(self._engine, "corpus_remove"):
            raise NotImplementedError(f"the engine {getattr(self._engine, 'name', type(self._engine).__name__)!r} removes no rows")
        n = len(self._master) + sum(len(s) for s, _ in self._pending)
        positions = self._positions(rows, n)
        if len(positions) == 0:
            return
        if len(positions) == n:
            raise ValueError("every row of the corpus would be removed: build a new corpus instead")
        self._engine.corpus_remove(state, positions)
        self._join_pending()
        keep = np.ones(n, dtype=bool)
        keep[positions] = False
        self._master = self._grown.without(keep)
        if self._master_id is not None:
            self._master_id = self._grown_id.without(keep)

    def compact(self) -> None:
        """Fold the appended rows into the corpus's first segment now (one matrix, one index) instead of when they exceed
        their share, and drop the removed rows from it.  Results do not change; nothing to do when nothing was appended or
        removed since the last compaction."""
        state = self._live()
        self._same_engine()
        if hasattr(self._engine, "corpus_compact"):
            self._engine.corpus_compact(state)

    # ------------------------------------------------------------------ an idf that follows the list
    def refit_idf(self) -> None:
        """Refit the idf on the CURRENT ``corpus.master``; the vocabulary stays the original list's.  Afterwards every result is,
        bit for bit, what sklearn's vectoriser gives when it is fitted on the current list with
        ``vocabulary=corpus.vectorizer.vocabulary_``: the document count is the number of rows now in the corpus (a string with
        no known n-gram counts, as sklearn counts it), a column's document frequency is the number of those rows that hold
        it, a column whose last row was removed keeps its place with frequency 0 and a finite idf that no row uses, and an
        n-gram the original list never had is still dropped -- ``Corpus(corpus.master, corpus.master_id)`` remains the only way
        to a new vocabulary.  Batches transformed afterwards are weighted with the new idf; ``corpus.vectorizer.idf_`` reports
        it.

        No string is read again (``stats['tokenisations']`` stays 1, ``stats['idf_refits']`` counts the calls): the rows on the
        device are counted by column and weighted anew from the whole counts they were made of.  Removed
        rows still pending are dropped first (a compaction).  A kept self-join (``keep_self_join``) is dropped and multiplied
        anew when next needed -- every score has changed -- with its options kept.  On a corpus that was never appended to
        nor removed from, nothing changes, to the bit."""
        state = self._live()
        self._same_engine()
        if not hasattr(self._engine, "corpus_refit_idf"):
            raise NotImplementedError(f"the engine {getattr(self._engine, 'name', type(self._engine).__name__)!r} refits no idf")
        self._engine.corpus_refit_idf(state)

    # ------------------------------------------------------------------ a self-join that is kept
    def keep_self_join(self, **kwargs) -> None:
        """Keep the result of the corpus's self-join on the device and keep it current across ``append`` and ``remove``.
        ``min_similarity`` and ``max_n_matches`` only (defaults: the corpus's own options); ``max_n_matches=None`` is refused,
        because the cut would move with every append.  From now on a self-join of the CURRENT ``corpus.master`` --
        ``match_strings(corpus.master)`` or ``group_similar_strings(corpus.master)``, whatever ``group_rep``,
        ``force_symmetries`` and ``ignore_index`` -- whose effective ``min_similarity`` and ``max_n_matches`` equal the kept
        ones is served from the kept result; every other call runs as it always did.  The result is multiplied when a call
        first needs it, once (``stats['self_join_full']``); an append then costs the new rows against the corpus and the
        corpus rows against the new ones, a remove the rows that were cut at ``max_n_matches`` and named a removed row
        (``stats['self_join_rows_refilled']``).  Calling it again with other values replaces the kept result."""
        state = self._live()
        self._same_engine()
        unknown = sorted(set(kwargs) - {"min_similarity", "max_n_matches"})
        if unknown:
            raise TypeError(f"keep_self_join() takes min_similarity and max_n_matches only, not {', '.join(unknown)}")
        if not hasattr(self._engine, "corpus_keep_self_join"):
            raise NotImplementedError(f"the engine {getattr(self._engine, 'name', type(self._engine).__name__)!r} keeps no self-join")
        options = self._options(kwargs)
        if options["max_n_matches"] is None:
            raise ValueError("max_n_matches=None cannot be kept: the cut would move with every append")
        top_n = options["max_n_matches"]
        if isinstance(top_n, (bool, np.bool_)) or not isinstance(top_n, (int, np.integer)) or top_n < 1:
            raise ValueError(f"max_n_matches={top_n!r} cannot be kept: a whole number of at least 1 is expected")
        self._engine.corpus_keep_self_join(state, int(top_n), float(options["min_similarity"]))

    def drop_self_join(self) -> None:
        """Free the kept self-join; every call runs the whole multiply again.  Nothing to do when none is kept."""
        state = self._live()
        self._same_engine()
        if hasattr(self._engine, "corpus_drop_self_join"):
            self._engine.corpus_drop_self_join(state)

    def _same_engine(self) -> None:
        if _engine_mod.get_engine() is not self._engine:
            raise RuntimeError("the engine has changed since the corpus was built (engine.set_engine / enable_distributed): "
                               "its device state belongs to the old one")

    @property
    def vectorizer(self):
        """The fitted vectoriser (``vocabulary_``, ``idf_``)."""
        return self._live().vec

    @property
    def stats(self) -> dict:
        """Work done so far: corpus tokenisations, index builds, transforms of other Series and the calls per path
        (``resident_index``: against the corpus's index; ``forward`` / ``reverse``: the corpus rows against new rows, and
        ``reverse_fallbacks``: reverse calls whose pair list exceeded the budget); ``appends`` / ``rows_appended``,
        ``compactions``, ``segments`` (1, or 2 while appended rows wait in their own segment) and ``base_index_builds``
        (builds of the first segment's index: 1 + compactions at most, whatever the number of appends; ``index_builds``
        counts every build, the second segment's included); ``removals`` / ``rows_removed`` and ``dead_rows`` (removed rows
        that still lie in the segments, until the next compaction); for a kept self-join (``keep_self_join``)
        ``self_join_full`` (whole multiplies made for it), ``self_join_served`` (calls answered from it),
        ``self_join_append_updates`` / ``self_join_remove_updates`` (changes it followed without a whole multiply) and
        ``self_join_rows_refilled`` (rows a remove had to multiply again); ``idf_refits`` (calls of ``refit_idf``);
        ``pair_calls`` / ``pairs_scored`` (calls of ``pair_similarities`` that reached the device, and their pairs);
        ``record_calls`` (calls of ``match_records`` / ``group_similar_records`` this corpus took part in, as the one that
        finds the candidates or as a further field), ``record_union_calls`` (those of them with several
        ``candidate_fields``, counted on the corpora that found candidates), ``record_floor_calls`` (those of them with a
        ``field_min_similarity``), ``record_field_score_calls`` (those of them with ``field_similarities=True``) and
        ``record_skip_empty_calls`` (those of them with ``empty_fields="skip"``)."""
        return dict(self._live().stats)

    def _rows_of(self, series, made):
        state = self._live()
        if not self._pending and series is self._master:
            return self._engine.corpus_matrix(state)
        m = self._engine.corpus_transform(state, series)
        made.append(m)
        return m

    # ------------------------------------------------------------------ options
    def _options(self, kwargs) -> dict:
        StringGrouperConfig(**kwargs)                   # TypeError on an unknown option
        for name in VECTORISER_OPTIONS:
            if name not in kwargs:
                continue
            mine, theirs = getattr(self._config, name), kwargs[name]
            same = (np.dtype(mine) == np.dtype(theirs)) if name == "tfidf_matrix_dtype" else mine == theirs
            if not same:
                raise ValueError(f"{name}={theirs!r} differs from the corpus's {name}={mine!r}: the vectoriser options are "
                                 f"fixed when the corpus is built")
        merged = self._config._asdict()
        merged.update(kwargs)
        return merged

    def _run(self, master, duplicates, master_id, duplicates_id, kwargs, finish):
        self._live()
        self._same_engine()
        g = _CorpusGrouper(self, master, duplicates, master_id, duplicates_id, **self._options(kwargs))
        try:
            return finish(g)
        finally:
            g._release()

    # ------------------------------------------------------------------ the four functions (string_grouper.py:55-153)
    def match_strings(self, master: pd.Series, duplicates: Optional[pd.Series] = None, master_id: Optional[pd.Series] = None,
                      duplicates_id: Optional[pd.Series] = None, **kwargs) -> pd.DataFrame:
        """All pairs of highly similar strings (self-join when ``duplicates`` is None), under the corpus's vocabulary."""
        return self._run(master, duplicates, master_id, duplicates_id, kwargs, lambda g: g.fit().get_matches())

    def match_most_similar(self, master: pd.Series, duplicates: pd.Series, master_id: Optional[pd.Series] = None,
                           duplicates_id: Optional[pd.Series] = None, **kwargs):
        """For every string in ``duplicates`` the most similar string of ``master`` (or itself)."""
        kwargs["max_n_matches"] = 1          # string_grouper.py:120
        return self._run(master, duplicates, master_id, duplicates_id, kwargs, lambda g: g.fit().get_groups())

    def group_similar_strings(self, strings_to_group: pd.Series, string_ids: Optional[pd.Series] = None, **kwargs):
        """For every string the representative of its group of similar strings."""
        return self._run(strings_to_group, None, string_ids, None, kwargs, lambda g: g.fit().get_groups())

    def compute_pairwise_similarities(self, string_series_1: pd.Series, string_series_2: pd.Series, **kwargs) -> pd.Series:
        """Row-wise similarity of two equally long series."""
        return self._run(string_series_1, string_series_2, None, None, kwargs, lambda g: g.dot())

    # ------------------------------------------------------------------ named pairs
    def pair_similarities(self, left, right, duplicates: Optional[pd.Series] = None) -> np.ndarray:
        """How similar are these particular records?  ``left[p]`` and ``right[p]`` are POSITIONS in the CURRENT
        ``corpus.master`` (a sequence or array of ints; negative ones count from the end); the answer is a numpy array of
        the corpus's dtype, one similarity a pair, in the order given.  With ``duplicates`` the right-hand positions count
        through that Series, which is transformed once as a batch (``duplicates is corpus.master``: the resident rows).

        The promise: for every pair (i, j) that ``match_strings`` reports for the same rows, the same bits -- a pair's score
        is the element of the multiply's product, in its arithmetic (string_grouper_amd/pairs.py) -- but for the diagonal of a
        self-join, which the frames set to 1.  ``compute_pairwise_similarities`` on the two gathered Series sums in numpy's
        order and may differ in the last bit; it also reads and vectorises every string again, which this call does not:
        the rows are on the device, two index lists go up and the scores come back (``stats['tokenisations']`` does not
        move; ``stats['pair_calls']`` / ``['pairs_scored']`` count).  Appended rows waiting in the second segment and removed
        rows still pending are served where they lie: no compaction (``stats['compactions']`` does not move).

        Bools or non-integers: TypeError; lists of different lengths: ValueError; a position outside [-n, n): IndexError,
        found before anything is uploaded; no pairs: an empty array and no device call."""
        state = self._live()
        self._same_engine()
        if not hasattr(self._engine, "corpus_pairs"):
            raise NotImplementedError(f"the engine {getattr(self._engine, 'name', type(self._engine).__name__)!r} scores no pairs")
        if duplicates is not None and not StringGrouper._is_series_of_strings(duplicates):
            raise TypeError('Input does not consist of pandas.Series containing only Strings')
        n = len(self._master) + sum(len(s) for s, _ in self._pending)
        resident = duplicates is None or (not self._pending and duplicates is self._master)
        left, right = checked_pairs(left, right, n, n if resident else len(duplicates))
        if len(left) == 0:
            return np.zeros(0, self._config.tfidf_matrix_dtype)
        if resident:
            return self._engine.corpus_pairs(state, left, right, None)
        made = []
        try:
            return self._engine.corpus_pairs(state, left, right, self._rows_of(duplicates, made))
        finally:
            for m in made:
                csr = getattr(m, "csr", None)
                if csr is not None:
                    csr.free()

    # ------------------------------------------------------------------ records of several fields
    def _record_call(self, others, duplicates, duplicates_id, weights, candidates, kwargs, finish, candidate_fields=(0,),
                     field_min_similarity=None, field_similarities=False, empty_fields="zero"):
        """The checks of ``match_records`` / ``group_similar_records`` that need the corpora, the description of the call
        (checked_record_call), what the engine can do of it, then the call."""
        self._live()
        self._same_engine()
        name = getattr(self._engine, 'name', type(self._engine).__name__)
        if not hasattr(self._engine, "corpus_records"):
            raise NotImplementedError(f"the engine {name!r} matches no records")
        if isinstance(others, Corpus) or not isinstance(others, (list, tuple)) or not all(isinstance(o, Corpus) for o in others):
            raise TypeError("others must be a list of Corpus objects, one for every further field")
        others = list(others)
        if not 1 <= len(others) <= self.MAX_RECORD_FIELDS:
            raise ValueError(f"{len(others)} further fields: between 1 and {self.MAX_RECORD_FIELDS} are expected")
        n = len(self._master) + sum(len(s) for s, _ in self._pending)
        for o in others:
            o._live()
            o._same_engine()
            if o._engine is not self._engine:
                raise RuntimeError("the corpora were built on different engines")
            if np.dtype(o._config.tfidf_matrix_dtype) != np.dtype(self._config.tfidf_matrix_dtype):
                raise ValueError(f"tfidf_matrix_dtype={o._config.tfidf_matrix_dtype!r} of a further corpus differs from the "
                                 f"corpus's tfidf_matrix_dtype={self._config.tfidf_matrix_dtype!r}")
            m = len(o._master) + sum(len(s) for s, _ in o._pending)
            if m != n:
                raise ValueError(f"the corpora differ in length ({m} and {n} rows): row p of every corpus must be record p")
        if kwargs.get("n_blocks") is not None:
            raise NotImplementedError("record matching takes no explicit n_blocks: the candidates stay on one device")
        options = self._options(kwargs)
        for o in others:
            o._options({k: v for k, v in kwargs.items() if k in VECTORISER_OPTIONS})
        # duplicates: one Series a field, equally long
        dup_fields = None
        if duplicates is not None:
            if isinstance(duplicates, pd.Series) or not isinstance(duplicates, (list, tuple)):
                raise TypeError("duplicates must be a list of pandas.Series, one for every field (this corpus's first)")
            if len(duplicates) != len(others) + 1:
                raise ValueError(f"{len(duplicates)} duplicates Series for {len(others) + 1} fields: one a field is expected")
            for d in duplicates:
                if not StringGrouper._is_series_of_strings(d):
                    raise TypeError('Duplicates input does not consist of pandas.Series containing only Strings')
            if len({len(d) for d in duplicates}) != 1:
                raise ValueError("the duplicates Series differ in length: row p of every Series must be record p")
            dup_fields = list(duplicates[1:])
        elif duplicates_id is not None:
            raise ValueError("duplicates_id without duplicates")
        n_right = n if duplicates is None else len(duplicates[0])
        call = checked_record_call([c._config for c in [self] + others], n_right, weights, candidates, candidate_fields,
                                   field_min_similarity, field_similarities, empty_fields)
        missing = call.needs - getattr(self._engine, "RECORD_OPTIONS", frozenset())
        for option, refusal in (("union", "unites no candidates of several fields"), ("floors", "takes no field_min_similarity"),
                                ("field_scores", "gives no field_similarities"), ("skip_empty", "takes no empty_fields='skip'")):
            if option in missing:
                raise NotImplementedError(f"the engine {name!r} {refusal}")
        g = _RecordGrouper(self, others, call, dup_fields, self.master, None if duplicates is None else duplicates[0],
                           self.master_id, duplicates_id, **options)
        for o in others:
            o._join_pending()
        try:
            return finish(g)
        finally:
            g._release()

    def match_records(self, others, duplicates=None, duplicates_id: Optional[pd.Series] = None, weights=None, candidates=None,
                      candidate_fields=(0,), field_min_similarity=None, field_similarities=False, empty_fields="zero",
                      **kwargs) -> pd.DataFrame:
        """Match RECORDS of several fields.  This corpus holds one field of every record (say the names), ``others`` -- a list
        of 1 to 7 ``Corpus`` objects -- the further fields (addresses, cities ...): row p of every corpus is record p, which is
        the caller's duty (append to and remove from all of them together; different lengths: ValueError).  The call is
        ``match_strings`` with another similarity:

        1. this corpus finds the candidates: its multiply at ``candidates=dict(min_similarity=..., max_n_matches=...)`` (the
           corpus's own options by default; at most 2 048 a record), served as ``match_strings`` is -- the resident index,
           the forward and the reverse path, a kept self-join;
        2. every candidate pair is scored on every further field, on the device, with the very bits
           ``other.pair_similarities(left_positions, right_positions)`` returns for it;
        3. ``similarity = weights[0] * s_0 + weights[1] * s_1 + ...`` in this order, in the corpus's dtype, every product and
           every sum rounded on its own.  ``weights``: one a field, this corpus's first, finite and > 0, equal shares
           ``1 / (fields)`` by default.  They are used as given: make them sum to 1 and ``min_similarity`` keeps its scale;
        4. pairs with ``similarity > min_similarity`` stay, a record's pairs are ordered by similarity descending, then
           position, and the first ``max_n_matches`` stay (``None``: all candidates).

        Candidates never leave the device; only the surviving pairs are downloaded.  ``duplicates``: None -- the records
        against themselves -- or a list of one Series a field (this corpus's first), equally long, each transformed once
        with its corpus's vocabulary; ``duplicates_id`` as in ``match_strings``.  Every other option of ``match_strings``
        (``ignore_index``, ``force_symmetries`` ...) means what it means there, applied to the combined similarity -- so in a
        self-join a record always matches itself with 1, and with ``force_symmetries`` the list is symmetric.  Vectoriser
        options that differ from a corpus's: ValueError; explicit ``n_blocks``: NotImplementedError; records x candidates
        beyond what one result on the device can index (2 * 10^9 cells): ValueError -- there is no block-wise route for
        records, and the one-field match ``match_strings`` falls back to is never returned in its place.  ``duplicates``
        whose first Series is ``corpus.master`` are still duplicates: the further Series given are the ones scored.

        The frame is ``match_strings(corpus.master, duplicates[0], corpus.master_id, duplicates_id)``'s, with the combined
        similarity (``field_similarities=True`` adds a column a field, below).  No further corpus is compacted or indexed by
        the call (``stats['record_calls']`` counts it on every corpus that took part).

        ``candidate_fields``: the fields that find the candidates, as ascending distinct positions -- 0 is this corpus, k is
        ``others[k - 1]``, and 0 is always among them; ``(0,)`` by default, which is the call described above.  With several,
        the candidates of a record are the UNION, over the candidate fields, of what that field's ``match_strings`` reports at
        its candidate options -- two records that share address and city are compared although their names share nothing.
        ``candidates`` is then one dict for every candidate field (a field's own corpus options fill what it leaves out) or a
        list of dicts, one a candidate field; their ``max_n_matches`` may be at most 2 048 TOGETHER (ValueError), and
        ``max_n_matches=None`` of the call keeps all of them.  Every candidate gets the same combined similarity of step 3,
        with ``s_f`` the bits ``corpus_f.pair_similarities`` returns, whichever field found it: the union and the missing
        scores are made on the device (``stats['record_union_calls']`` counts the call on the candidate fields' corpora).  A
        further corpus named as a candidate field is treated as this corpus is -- it builds its index and a self-join
        compacts it; the others are still only read.

        ``field_min_similarity``: a floor a FIELD -- one entry a field, this corpus's first, each ``None`` (no floor) or a
        finite number (a wrong length, NaN, inf: ValueError; a bool: TypeError); ``None`` by default, which is the call
        described above -- and so is a list whose entries are all ``None``.  "The city must agree" is a condition on one field, which no ``min_similarity`` of the weighed sum
        can express.  With floors, step 4 keeps a pair when ``s_f > field_min_similarity[f]`` (in the corpus's dtype; strict,
        as ``min_similarity`` is) for every field with a floor AND ``similarity > min_similarity``; the similarity, the order
        and the cut are unchanged, and the floors act BEFORE the cut: the first ``max_n_matches`` of the pairs that passed
        stay.  ``s_0`` is the score the candidate carries.  A floor may sit on any field, candidate field or not.  It is
        decided on the device (``stats['record_floor_calls']`` counts the call), and a candidate a floor has refused is not
        scored on the fields after it.  In a self-join a record still matches itself whatever the floors say, and with
        ``force_symmetries`` the list is still symmetric: both are made after the floors, as they are made after
        ``min_similarity``.

        ``field_similarities=True``: which field carried a match.  The frame gets the columns ``similarity_0``,
        ``similarity_1`` ... (float64, as ``similarity`` is) right after ``similarity``; k counts as in ``candidate_fields``.
        For a row whose left and right records have the POSITIONS l and r, ``similarity_k`` is bit for bit
        ``corpus_k.pair_similarities([l], [r], duplicates=...)[0]``, widened -- for every row of the frame: the diagonal a
        self-join adds carries the field's own product there (not 1; 0 for an empty string), the mirrored rows of
        ``force_symmetries`` the score of the pair they name.  The rows ``include_zeroes`` adds carry 0.0.  The list is scored
        where it lies on the device, before it is freed or handed to the group kernels; the planes are a second read-back
        after the list's own (``stats['record_field_score_calls']`` counts the call): no position list goes up, no label is
        translated, whatever the index is.  Anything but a bool: TypeError.

        ``empty_fields``: ``"zero"`` (the default: the call described above, launch for launch) or ``"skip"`` (anything but a
        str: TypeError; another string: ValueError).  Real records have blanks, and a blank field scores 0 and enters the sum
        with its full weight: two records with identical names and cities, one of them without an address, reach 0.7 at
        weights 0.5 / 0.3 / 0.2.  With ``"skip"`` a field that is EMPTY for a pair takes no part in that pair and its weight
        is shared among the fields that are known.  A field is empty for a pair when the string of either record is empty
        for that field's corpus: a string with no n-gram that the corpus knows -- ``""``, a string shorter than
        ``ngram_size`` after the regex, and in ``duplicates`` a string made only of n-grams the corpus has never seen.  This
        holds for this corpus's field as well.  Step 3 becomes, with ``W`` the weights in the corpus's dtype::

            c  = sum of W[f] * s_f  over the fields that are not empty for the pair   (in field order, as in step 3)
            wp = sum of W[f]        over the same fields
            wt = sum of W[f]        over all fields
            similarity = c               when no field is empty for the pair: bit for bit the similarity of "zero"
                       = (c * wt) / wp   when some are: every step rounded on its own, one division
                       dropped           when every field is empty

        so on records without blanks the option changes no bit, and ``min_similarity`` keeps the scale it has for the
        weights given.  A floor of ``field_min_similarity`` on a field that is empty for the pair is not held against it
        (this corpus's floor included when its field is empty); on the other fields floors act as before.  The filter, the
        order and the cut act on ``similarity`` as they always did.  The columns of ``field_similarities`` are unchanged: an
        empty field shows its product, 0.0 -- so ``acc = acc + W[f] * similarity_f`` recombines to ``similarity`` only on rows
        without an empty field.  In a self-join a record still matches itself with 1, also a record all of whose fields are
        blank, and ``force_symmetries`` still gives a symmetric list.  All of it is decided on the device
        (``stats['record_skip_empty_calls']`` counts the call on every corpus that took part); nothing of a field's right
        rows is read for a record whose own field is blank."""
        return self._record_call(others, duplicates, duplicates_id, weights, candidates, kwargs, lambda g: g.fit().get_matches(),
                                 candidate_fields, field_min_similarity, field_similarities, empty_fields)

    def group_similar_records(self, others, weights=None, candidates=None, candidate_fields=(0,), field_min_similarity=None,
                              empty_fields="zero", **kwargs):
        """For every record the representative of its group of similar records: ``group_similar_strings(corpus.master,
        corpus.master_id)`` over the match list of ``match_records(others, weights=..., candidates=..., candidate_fields=...,
        field_min_similarity=..., empty_fields=...)``."""
        return self._record_call(others, None, None, weights, candidates, kwargs, lambda g: g.fit().get_groups(), candidate_fields,
                                 field_min_similarity, False, empty_fields)
