"""Seam b1: a TfidfVectorizer-shaped front end of the device vectoriser (K1 + K2).

Mirrors how the reference builds and drives its vectoriser
(string_grouper/string_grouper.py:306 ``TfidfVectorizer(min_df=1, analyzer=self.n_grams, dtype=...)``,
``.fit`` at :706, ``.transform`` at :689/:692) and the analyzer ``StringGrouper.n_grams`` (:365-378).

Host work is limited to what has no byte-level definition -- Unicode ``str.lower()`` / NFKD for strings with
non-ASCII characters and ``re.sub`` for a regex that is not a plain character class -- and is vectorised
(string_grouper_amd/strprep.py: numpy over code points, Python's own semantics consulted once per distinct code
point).  Everything else -- ASCII lower-casing, character deletion, n-gramming, vocabulary, counts, idf weighting,
L2 normalisation -- runs on the GPU.  There is no CPU tokeniser fallback.

Two kinds of columns reach the device (strprep.StringColumn): BYTE columns (ASCII after the host step; the default
``normalize_to_ascii=True`` always ends here) and SYMBOL columns (``normalize_to_ascii=False`` with non-ASCII
characters: uint16 ranks in the alphabet of the fit, which is the sorted set of the code points of all columns of
that fit -- so that the packed keys still sort like sklearn's vocabulary).
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _native as N
from . import strprep as SP
from .strprep import StringColumn, delete_table_for, regex_is_char_class   # noqa: F401  (re-exported)

DEFAULT_REGEX = r'[,-./]|\s'
SYMBOL_ABSENT = 0xFFFF

PreparedStrings = StringColumn      # round-1 name


def keys_to_terms(keys: np.ndarray, ngram_size: int, bits: int = 7, alphabet: Optional[np.ndarray] = None) -> List[str]:
    """The n-gram strings of packed keys: ``bits`` per character code, big-endian; ``alphabet[code]`` = code point of a
    character code (None: the code is the code point)."""
    out = []
    mask = (1 << bits) - 1
    for k in keys.tolist():
        codes = [(k >> (bits * (ngram_size - 1 - q))) & mask for q in range(ngram_size)]
        out.append("".join(chr(int(alphabet[c])) if alphabet is not None else chr(c) for c in codes))
    return out


def idf_from_df(df: np.ndarray, n_docs: int, dtype) -> np.ndarray:
    """sklearn TfidfTransformer.fit op sequence (text.py:1664-1679) so that log() is bit-identical."""
    d = df.astype(dtype, copy=True)
    d += float(True)                   # smooth_idf
    idf = np.full_like(d, fill_value=n_docs + 1, dtype=dtype)
    idf /= d
    np.log(idf, out=idf)
    idf += 1.0
    return idf


class HipTfidfVectorizer:
    """fit / transform with the semantics of the reference's TfidfVectorizer instance.

    ``transform`` returns a scipy CSR (host) for the drop-in seam; ``transform_prepared`` keeps the
    matrix in HBM for the fused path."""

    def __init__(self, ngram_size: int = 3, regex: str = DEFAULT_REGEX, ignore_case: bool = True,
                 normalize_to_ascii: bool = True, dtype=np.float64, ctx: Optional[N.Context] = None):
        self.ngram_size = int(ngram_size)
        self.regex = regex
        self.ignore_case = bool(ignore_case)
        self.normalize_to_ascii = bool(normalize_to_ascii)
        self.dtype = np.dtype(dtype).type
        N.np_dtype_code(self.dtype)
        self._ctx = ctx
        self._vocab: Optional[N.Vocab] = None
        self._fit_sets: List[StringColumn] = []
        self._fit_originals: List[StringColumn] = []
        self._dev_of: Dict[int, StringColumn] = {}
        self._keys = None
        self._df = None
        self._idf = None
        self._n_docs = 0
        self._vocabulary: Optional[Dict[str, int]] = None
        self._alphabet: Optional[np.ndarray] = None        # symbol fits: sorted code points, rank = symbol
        # a regex that is not a character class is applied on the host (strprep): nothing left for the device to delete
        self._delete_table = delete_table_for(regex) if regex_is_char_class(regex) else np.zeros(128, np.uint8)
        self._params = N.SgVecParams()
        self._params.ngram_size = self.ngram_size
        self._params.ascii_lower = 1 if self.ignore_case else 0
        self._params.dtype = N.np_dtype_code(self.dtype)
        for c in range(128):
            self._params.delete_table[c] = int(self._delete_table[c])

    @property
    def ctx(self) -> N.Context:
        if self._ctx is None:
            self._ctx = N.default_context()
        return self._ctx

    # ------------------------------------------------------------------ device-level API
    def prepare(self, strings) -> StringColumn:
        """Host step + upload of one string column.  Byte columns go to HBM right away; a symbol column is uploaded
        when its alphabet is known (at fit, or against the fitted alphabet at transform)."""
        col = SP.prepare_column(strings, self.ignore_case, self.normalize_to_ascii, self.regex)
        if col.kind == "bytes":
            self._upload_bytes(col)
        return col

    def _upload_bytes(self, col: StringColumn):
        col.dev = self.ctx.strings_from_host(col.data, col.offsets)
        if col.prelowered:
            self.ctx.strings_set_prelowered(col.dev, True)

    def _as_symbols(self, col: StringColumn) -> StringColumn:
        return col if col.kind == "symbols" else SP.bytes_column_to_symbols(col, self.ignore_case, self._delete_table)

    def _upload_symbols(self, col: StringColumn, alphabet: np.ndarray) -> StringColumn:
        """Rank the code points of a symbol column in ``alphabet`` (sorted) and upload the ranks."""
        at = np.searchsorted(alphabet, col.data)
        at_c = np.minimum(at, len(alphabet) - 1)
        known = alphabet[at_c] == col.data if len(alphabet) else np.zeros(len(col.data), bool)
        ranks = np.where(known, at_c, SYMBOL_ABSENT).astype(np.uint16)
        out = StringColumn("symbols", col.data, col.offsets, prelowered=True)
        out.dev = self.ctx.strings_from_host_symbols(ranks, col.offsets, len(alphabet))
        return out

    def _device_sets(self, sets: Sequence[StringColumn]) -> List[StringColumn]:
        """The columns of one fit as the device wants them: all byte columns, or -- as soon as one of them carries
        non-ASCII symbols -- all symbol columns over one shared alphabet."""
        if all(s.kind == "bytes" for s in sets):
            self._alphabet = None
            for s in sets:
                if s.dev is None:
                    self._upload_bytes(s)
            return list(sets)
        syms = [self._as_symbols(s) for s in sets]
        alphabet = np.unique(np.concatenate([s.data for s in syms])) if syms else np.zeros(0, np.uint32)
        if len(alphabet) == 0:
            raise ValueError("empty vocabulary; perhaps the documents only contain stop words")
        if len(alphabet) >= SYMBOL_ABSENT:
            raise NotImplementedError(f"{len(alphabet)} distinct characters; the device codes symbols in 16 bits")
        self._alphabet = alphabet.astype(np.uint32)
        return [self._upload_symbols(s, self._alphabet) for s in syms]

    def fit_prepared(self, sets: Sequence[StringColumn]) -> "HipTfidfVectorizer":
        """TfidfVectorizer.fit(concat(sets)) (string_grouper.py:699-707)."""
        dev_sets = self._device_sets(sets)
        self._vocab = self.ctx.vec_fit([s.dev for s in dev_sets], self._params)
        self._remember(sets, dev_sets)
        return self._finish_fit()

    def _remember(self, sets, dev_sets):
        # transform_prepared() of a column that was part of the fit must reuse the fit's tokens: the library
        # recognises the device handle, so keep the (possibly converted) device column of every input column
        # (the ORIGINAL columns are kept alive too: the table is keyed by id(), and the id of a freed column can be handed
        #  to a later one -- which would then silently get the fit column's matrix)
        self._fit_sets = list(dev_sets)
        self._fit_originals = list(sets)
        self._dev_of = {id(s): d for s, d in zip(sets, dev_sets)}

    def handles(self) -> list:
        """What the fit holds on the device: the vocabulary and the string columns that were uploaded for it."""
        hs = [self._vocab] + [col.dev for col in self._fit_sets + self._fit_originals]
        return [h for k, h in enumerate(hs) if h is not None and not any(h is x for x in hs[:k])]

    def free(self) -> None:
        """Release ``handles()``; the vectoriser is of no use afterwards."""
        for h in self.handles():
            h.free()
        for col in self._fit_sets + self._fit_originals:
            col.dev = None
        self._fit_sets, self._fit_originals, self._dev_of = [], [], {}

    # the idf of a term is a function of its document count and the number of documents only: for fits of up to this many
    # documents the function is tabulated once per (documents, dtype) -- with numpy, so that log() stays sklearn's --, kept
    # on the device, and a fit() weights its terms there: no download of the counts, no upload of the weights, no
    # synchronisation (include/sg_hip.h: sg_ctx_put_idf_table).  Larger fits take the round trip (the table would be
    # as large as the strings).
    IDF_TABLE_MAX_DOCS = 4_000_000
    # ... and the table is only worth its upload (documents + 1 weights, one synchronisation) when it is used again or is
    # not much larger than what the round trip moves (the vocabulary's counts down, its weights up): a one-shot fit of a
    # long list over a small vocabulary -- 663 k names, 18 k 3-grams -- takes the round trip the first time and gets its
    # table when the same (documents, dtype) comes a second time (repeated fits of one list: a service, the benchmark loop)
    IDF_TABLE_RATIO = 4

    def _finish_fit(self) -> "HipTfidfVectorizer":
        n_terms, n_docs = self.ctx.vocab_size(self._vocab)
        self._n_docs = n_docs
        self._keys = self._df = self._idf = None
        self._vocabulary = None
        if n_docs <= self.IDF_TABLE_MAX_DOCS:
            if self.ctx.vocab_apply_idf_table(self._vocab):          # a table for this (documents, dtype) is installed
                return self
            # (a first fit of a long list takes the host round trip below, the second one of the same shape installs the
            #  table: single fits must not be compared with looped ones -- bench.py's warm-up runs make the timed steps "second" fits)
            fits = self.ctx.note_idf_fit(n_docs, np.dtype(self.dtype).str)
            if n_docs + 1 <= self.IDF_TABLE_RATIO * max(int(n_terms), 1) or fits >= 2:
                self.ctx.put_idf_table(n_docs, idf_from_df(np.arange(n_docs + 1, dtype=np.int64), n_docs, self.dtype))
                if not self.ctx.vocab_apply_idf_table(self._vocab):
                    raise RuntimeError("the idf table that was just installed is not there")
                return self
        self._fetch_vocabulary()
        self._idf = idf_from_df(self._df, n_docs, self.dtype)
        self.ctx.vocab_set_idf(self._vocab, self._idf)
        return self

    def _fetch_vocabulary(self) -> None:
        """Keys and document counts of the fitted vocabulary on the host (downloaded when first asked for)."""
        if self._keys is None:
            if self._vocab is None:
                raise AttributeError("available after fit()")
            self._keys, self._df = self.ctx.vocab_to_host(self._vocab)

    @property
    def idf_(self) -> np.ndarray:
        """sklearn's attribute: the inverse document frequency of every column (computed as sklearn computes it)."""
        if getattr(self, "_idf", None) is None:
            self._fetch_vocabulary()
            self._idf = idf_from_df(self._df, self._n_docs, self.dtype)
        return self._idf

    # ---- the two halves of fit for a caller that shards the strings over several GPUs (distributed.py)
    def fit_begin_prepared(self, sets: Sequence[StringColumn]) -> "HipTfidfVectorizer":
        """Tokenise the LOCAL sets and count their document frequencies; ``df_table()`` is then summed across
        ranks and ``fit_end`` finishes the vocabulary + idf identically on every rank."""
        dev_sets = self._device_sets(sets)
        self._vocab = self.ctx.vec_fit_begin([s.dev for s in dev_sets], self._params)
        self._remember(sets, dev_sets)
        return self

    def df_table(self):
        """(device pointer, entries, shareable) of the dense int32 document-frequency table of ``fit_begin``."""
        return self.ctx.vocab_df_table(self._vocab)

    def fit_end(self, n_docs_total: int = 0) -> "HipTfidfVectorizer":
        self.ctx.vec_fit_end(self._vocab, n_docs_total)
        return self._finish_fit()

    def transform_prepared(self, s: StringColumn) -> N.Csr:
        if self._vocab is None:
            raise RuntimeError("vectoriser is not fitted")
        dev = self._dev_of.get(id(s))
        if dev is None:
            if self._alphabet is not None:
                dev = self._upload_symbols(self._as_symbols(s), self._alphabet)
            elif s.kind == "bytes":
                if s.dev is None:
                    self._upload_bytes(s)
                dev = s
            else:
                raise NotImplementedError(
                    "transform() of strings with non-ASCII characters (normalize_to_ascii=False) on a vocabulary that "
                    "was fitted on ASCII-only strings: fit on a corpus that contains the characters, as StringGrouper "
                    "does (it fits on master + duplicates)")
        return self.ctx.vec_transform(self._vocab, dev.dev)

    def refit_idf_prepared(self, m: N.Csr) -> N.Csr:
        """The idf refitted on the documents whose rows ``m`` holds (a matrix this vectoriser made, under its current idf),
        the vocabulary staying what it is: ``TfidfVectorizer(vocabulary=self.vocabulary_, ...).fit(docs)``.  Returns
        ``.transform(docs)`` under the new idf as a new matrix; ``m`` is only read.  No string is read: the document counts
        are the column counts of ``m`` (a row names a column once), the number of documents is its rows (empty ones count, as
        sklearn counts them), the idf is ``idf_from_df`` of the two -- numpy's log -- and the device recovers every entry's
        count from its value and its row's norm (include/sg_hip.h: sg_vec_reweigh).  ``idf_`` and the counts
        ``sg_vocab_to_host`` reports are the new ones afterwards, and later transforms use them.  ``last_refit_s`` holds the
        seconds of the three steps."""
        if self._vocab is None:
            raise RuntimeError("vectoriser is not fitted")
        t0 = time.perf_counter()
        df = m.column_counts().astype(np.int64)
        n_docs = m.dims()[0]
        t1 = time.perf_counter()
        idf = idf_from_df(df, n_docs, self.dtype)
        t2 = time.perf_counter()
        out = self.ctx.vec_reweigh(self._vocab, m, df, n_docs, idf)
        self.last_refit_s = {"counts": t1 - t0, "host_idf": t2 - t1, "reweigh": time.perf_counter() - t2}
        self._df, self._idf, self._n_docs = df, idf, n_docs
        return out

    # ------------------------------------------------------------------ sklearn-shaped API (seam b1)
    def fit(self, raw_documents, y=None):
        return self.fit_prepared([self.prepare(raw_documents)])

    def transform(self, raw_documents):
        """Always re-reads ``raw_documents`` (as sklearn does): the tokens of fit() are only reused through the
        explicit handles (``prepare`` / ``fit_prepared`` / ``transform_prepared``, or ``fit_transform``)."""
        return self.transform_prepared(self.prepare(raw_documents)).to_scipy()

    def fit_transform(self, raw_documents, y=None):
        p = self.prepare(raw_documents)
        return self.fit_prepared([p]).transform_prepared(p).to_scipy()      # one tokenisation pass

    def _terms(self) -> List[str]:
        self._fetch_vocabulary()
        bits, symbols, _ = self.ctx.vocab_coding(self._vocab)
        alphabet = self._alphabet if symbols else self.ctx.vocab_byte_alphabet(self._vocab)
        return keys_to_terms(self._keys, self.ngram_size, bits, alphabet)

    @property
    def vocabulary_(self) -> Dict[str, int]:
        if self._vocabulary is None:
            if self._vocab is None:
                raise AttributeError("vocabulary_ is available after fit()")
            self._vocabulary = {t: i for i, t in enumerate(self._terms())}
        return self._vocabulary

    def get_feature_names_out(self):
        return np.asarray(self._terms(), dtype=object)


class TfidfVectorizer(HipTfidfVectorizer):
    """Seam b1 BY NAME: the constructor call the reference makes, ``TfidfVectorizer(min_df=1, analyzer=self.n_grams,
    dtype=self._config.tfidf_matrix_dtype)`` (string_grouper/string_grouper.py:306), served by the device vectoriser.  With

        import string_grouper.string_grouper as ref
        ref.TfidfVectorizer = string_grouper_amd.vectorizer.TfidfVectorizer

    (or the one-line import patch of INTEGRATION.md) the unmodified reference vectorises on the GPU.  The analyzer is a
    Python callable, which the device cannot run; what it computes is fully described by the options of the object it is
    bound to -- ``StringGrouper.n_grams`` reads ``self._config.{ngram_size, regex, ignore_case, normalize_to_ascii}``
    (:365-378) -- so those are taken from ``analyzer.__self__._config``.  Any other analyzer is refused: there is no CPU
    tokeniser to fall back to."""

    def __init__(self, *, min_df=1, analyzer=None, dtype=np.float64, ctx: Optional[N.Context] = None, **unsupported):
        if unsupported:
            raise TypeError(f"TfidfVectorizer options the device vectoriser does not implement: {sorted(unsupported)}")
        if min_df != 1:
            raise NotImplementedError("min_df != 1 (the reference always passes 1, string_grouper.py:306)")
        owner = getattr(analyzer, "__self__", None)
        cfg = getattr(owner, "_config", None)
        if getattr(analyzer, "__name__", "") != "n_grams" or cfg is None:
            raise TypeError("analyzer must be the bound n_grams method of a StringGrouper (string_grouper.py:365-378): its "
                            "options, not its code, are what reaches the device")
        super().__init__(ngram_size=cfg.ngram_size, regex=cfg.regex, ignore_case=cfg.ignore_case,
                         normalize_to_ascii=cfg.normalize_to_ascii, dtype=dtype, ctx=ctx)
        self.min_df, self.analyzer = min_df, analyzer
