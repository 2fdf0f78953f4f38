"""A fitted corpus that stays on the GPU: match new strings against it without refitting.

The reference documents this use (``sg = StringGrouper(master)``, then ``sg.match_strings(new_master)`` "using the corpus
already built above without rebuilding or changing it in any way", docs/references/sg_class.md Example 1) but its code
refits on master + duplicates every call (string_grouper.py:685-707), and so does ``StringGrouper`` here.  ``Corpus`` is
the fixed-corpus form:

    corpus = Corpus(master)                      # vocabulary + idf of TfidfVectorizer(...).fit(master), once
    corpus.match_strings(master, new_batch)      # new_batch.transform()ed with them; master's rows and index are resident

Every Series a method receives is transformed with the corpus's vocabulary and idf (an n-gram the corpus never had is
dropped, as sklearn's transform drops it); everything after that is what ``StringGrouper.fit()`` and its frames do with the
two matrices.  The methods have the signatures of the module-level functions (string_grouper.py:55-153).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import pandas as pd

from . import engine as _engine_mod
from .string_grouper import StringGrouper, StringGrouperConfig

# options that define the vectoriser: a call may not change them (the corpus was fitted with them)
VECTORISER_OPTIONS = ("ngram_size", "regex", "ignore_case", "normalize_to_ascii", "tfidf_matrix_dtype")


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


class Corpus:
    """A master list fitted once and kept on the device; see the module docstring."""

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
        cfg = self._config
        self._state = eng.corpus_fit(master, cfg.ngram_size, cfg.regex, cfg.ignore_case, cfg.normalize_to_ascii,
                                     cfg.tfidf_matrix_dtype)

    # ------------------------------------------------------------------ resources
    def close(self) -> None:
        """Free everything the corpus holds on the device (vocabulary, idf, its rows, its index)."""
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
        return self._master

    @property
    def vectorizer(self):
        """The fitted vectoriser (``vocabulary_``, ``idf_``)."""
        return self._live().vec

    @property
    def stats(self) -> dict:
        """Work done so far: corpus tokenisations, index builds, transforms of other Series and the calls per path
        (``resident_index``: against the corpus's index; ``forward`` / ``reverse``: the corpus rows against new rows, and
        ``reverse_fallbacks``: reverse calls whose pair list exceeded the budget)."""
        return dict(self._live().stats)

    def _rows_of(self, series, made):
        state = self._live()
        if series is self._master:
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
        if _engine_mod.get_engine() is not self._engine:
            raise RuntimeError("the engine has changed since the corpus was built (engine.set_engine / enable_distributed): "
                               "its device state belongs to the old one")
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
