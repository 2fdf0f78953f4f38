"""What Corpus.refit_idf is held to, for the CPU and the GPU tests alike.  TEST INFRASTRUCTURE ONLY.

- the oracle definition: sklearn's TfidfVectorizer fitted on the CURRENT list with the vocabulary FIXED to the original list's
  (``fixed_vocabulary_matrices``), and the frames of the four functions over its matrices (``expected_after_refit``);
- the engine double that refits with it (``RefitCorpusOracleEngine``);
- a numpy restatement of what the device does instead -- no string is read: the whole count behind an entry is recovered from
  the entry, its row's norm and the old idf, verified, weighted with the new idf, and the row is normalised by a sum taken in
  column order in double (``reweigh_restated``), with the wrong turns a restatement could take as ``variant``;
- the list the restatement and the kernels are tried on (``bite_list``)."""
import functools

import numpy as np
import scipy.sparse as sp
from sklearn.feature_extraction.text import TfidfVectorizer

from oracle import oracle as O
from string_grouper_amd.string_grouper import StringGrouper
from string_grouper_amd.vectorizer import idf_from_df
from tests._corpus_oracle import CorpusHostMatrix
from tests._corpus_selfjoin_cases import SelfJoinCorpusOracleEngine
from tests._oracle_engine import HostMatrix, OracleEngine


# ------------------------------------------------------------------------------------------ the oracle definition
def fixed_vocabulary_vectoriser(original, current, dtype=np.float64, **ngram_kw):
    """TfidfVectorizer(vocabulary=<fit(original)'s>, ...).fit(current): the idf follows ``current``, the columns do not."""
    first = TfidfVectorizer(min_df=1, analyzer=lambda s: O.ngrams(s, **ngram_kw), dtype=dtype).fit(list(original))
    vec = TfidfVectorizer(min_df=1, analyzer=lambda s: O.ngrams(s, **ngram_kw), dtype=dtype, vocabulary=dict(first.vocabulary_))
    return vec.fit(list(current))


def fixed_vocabulary_matrices(original, current, sets, dtype=np.float64, **ngram_kw):
    vec = fixed_vocabulary_vectoriser(original, current, dtype, **ngram_kw)
    return [vec.transform(list(s)).tocsr() for s in sets], dict(vec.vocabulary_), vec.idf_.copy()


class _RefittedGrouper(StringGrouper):
    """The oracle definition of a call after a refit: the mirror's fit() and frames over the matrices above."""

    def __init__(self, original, current, *args, **kwargs):
        self._original, self._current = original, current
        super().__init__(*args, **kwargs)

    def _tfidf_on_engine(self):
        cfg = self._config
        kw = dict(ngram_size=cfg.ngram_size, regex=cfg.regex, ignore_case=cfg.ignore_case,
                  normalize_to_ascii=cfg.normalize_to_ascii)
        sets = [self._master] + ([] if self._duplicates is None else [self._duplicates])
        mats, _, _ = fixed_vocabulary_matrices(self._original, self._current, sets, dtype=cfg.tfidf_matrix_dtype, **kw)
        A = HostMatrix(mats[0])
        return A, (A if self._duplicates is None else HostMatrix(mats[1]))


def expected_after_refit(original, current, method, *args, **kwargs):
    import string_grouper_amd.engine as E
    before = E._engine
    E.set_engine(OracleEngine(use_port=True))
    try:
        if method == "match_strings":
            master, dupes, mid, did = (list(args) + [None] * 4)[:4]
            return _RefittedGrouper(original, current, master, dupes, mid, did, **kwargs).fit().get_matches()
        if method == "match_most_similar":
            master, dupes, mid, did = (list(args) + [None] * 4)[:4]
            kwargs["max_n_matches"] = 1
            return _RefittedGrouper(original, current, master, dupes, mid, did, **kwargs).fit().get_groups()
        if method == "group_similar_strings":
            strings, ids = (list(args) + [None] * 2)[:2]
            return _RefittedGrouper(original, current, strings, master_id=ids, **kwargs).fit().get_groups()
        s1, s2 = args
        return _RefittedGrouper(original, current, s1, s2, **kwargs).dot()
    finally:
        E.set_engine(before)


# ------------------------------------------------------------------------------------------ the engine double
class RefitCorpusOracleEngine(SelfJoinCorpusOracleEngine):
    """The corpus double (it grows, forgets and keeps a self-join) that remembers its strings and refits the idf on them with
    sklearn, the vocabulary fixed."""
    name = "oracle-corpus-refit"

    def corpus_fit(self, strings, ngram_size, regex, ignore_case, normalize_to_ascii, dtype):
        state = super().corpus_fit(strings, ngram_size, regex, ignore_case, normalize_to_ascii, dtype)
        state.strings = list(strings)
        state.ngram_kw = dict(ngram_size=ngram_size, regex=regex, ignore_case=ignore_case, normalize_to_ascii=normalize_to_ascii)
        state.dtype = dtype
        state.stats["idf_refits"] = 0
        return state

    def corpus_append(self, state, strings):
        super().corpus_append(state, strings)
        state.strings += list(strings)

    def corpus_remove(self, state, positions):
        super().corpus_remove(state, positions)
        gone = set(np.asarray(positions, dtype=np.int64).tolist())
        state.strings = [s for i, s in enumerate(state.strings) if i not in gone]

    def corpus_refit_idf(self, state):
        kw = state.ngram_kw
        vec = TfidfVectorizer(min_df=1, analyzer=lambda s: O.ngrams(s, **kw), dtype=state.dtype,
                              vocabulary=dict(state.vec.vocabulary_))
        vec.fit(state.strings)
        state.vec = vec
        state.matrix = CorpusHostMatrix(vec.transform(state.strings), state)
        state.index = None
        state.kept = None                     # every score has changed; the options stay
        state.stats["idf_refits"] += 1


# ------------------------------------------------------------------------------------------ the restatement
def k2_restated(counts: sp.csr_matrix, idf: np.ndarray, dtype):
    """K2 on whole counts: (values, norms) -- w = (T)tf * idf[col]; the squares, each rounded to T, summed in column order in
    double; v = (T)((double)w / sqrt(sum)); the norm of a row without entries is 0.0."""
    T = np.dtype(dtype).type
    w = (counts.data.astype(T) * idf[counts.indices].astype(T)).astype(T)
    sq = (w * w).astype(T).astype(np.float64)
    norms = np.zeros(counts.shape[0], np.float64)
    out = np.zeros(len(w), T)
    for r in range(counts.shape[0]):
        a, b = counts.indptr[r], counts.indptr[r + 1]
        if b > a:
            norms[r] = np.sqrt(np.cumsum(sq[a:b])[-1])         # cumsum adds one after the other, left to right
            out[a:b] = (w[a:b].astype(np.float64) / norms[r]).astype(T)
    return out, norms


def _row_sum(sq: np.ndarray, variant: str, T) -> np.float64:
    if variant == "sum_in_float":
        return np.float64(np.cumsum(sq.astype(T), dtype=T)[-1])
    if variant == "sum_in_another_order":
        return np.cumsum(sq[::-1])[-1]
    return np.cumsum(sq)[-1]


def reweigh_restated(m: sp.csr_matrix, norms: np.ndarray, idf_old: np.ndarray, idf_new: np.ndarray, variant: str = ""):
    """sg_vec_reweigh in numpy: (new values, new norms, recovered counts, entries that failed the verification).
    ``variant``: "" the statement; "tf_by_smallest_ratio", "sum_in_float", "sum_in_another_order": a wrong turn each."""
    T = m.dtype.type
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    io = idf_old[m.indices].astype(T)
    v = m.data
    if variant == "tf_by_smallest_ratio":          # without the norm: the smallest v / idf of a row taken for a count of one
        ratio = v.astype(np.float64) / io.astype(np.float64)
        least = np.full(m.shape[0], np.inf)
        np.minimum.at(least, rows, ratio)
        tf = np.rint(ratio / least[rows])
    else:
        tf = np.rint(v.astype(np.float64) * norms[rows] / io.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        again = ((tf.astype(T) * io).astype(T).astype(np.float64) / norms[rows]).astype(T)
    bits = np.uint32 if T is np.float32 else np.uint64
    failed = int(np.count_nonzero(again.view(bits) != v.view(bits)))
    w = (tf.astype(T) * idf_new[m.indices].astype(T)).astype(T)
    sq = (w * w).astype(T).astype(np.float64)
    out, new_norms = np.zeros(len(w), T), np.zeros(m.shape[0], np.float64)
    for r in range(m.shape[0]):
        a, b = m.indptr[r], m.indptr[r + 1]
        if b > a:
            new_norms[r] = np.sqrt(_row_sum(sq[a:b], variant, T))
            out[a:b] = (w[a:b].astype(np.float64) / new_norms[r]).astype(T)
    return out, new_norms, tf.astype(np.int64), failed


def refit_idf_of(m: sp.csr_matrix, dtype) -> np.ndarray:
    """The idf the refit installs: document counts = entries per column, documents = rows."""
    return idf_from_df(np.bincount(m.indices, minlength=m.shape[1]).astype(np.int64), m.shape[0], dtype)


# ------------------------------------------------------------------------------------------ the list
ROW_LENGTHS = (0, 1, 16, 17, 32, 33)
_SYMBOLS = "abcdefghijklmnopqrstuvwxyz0123456789"


@functools.lru_cache(maxsize=None)
def bite_list():
    """(original, appended, removed positions in original + appended, live): the list the reweigh is tried on.

    Rows of 0, 1, 16, 17, 32, 33 and more than 128 distinct n-grams (the kernel walks sixteen entries a trip and keeps the
    first 32 in registers); counts far from one ("a" * 70 000: one n-gram 69 998 times, "ab" * 3 000: two n-grams 2 999 times
    each) and mixed counts in one row; an appended string with no n-gram the original list has (an empty row that counts as a
    document) and one that repeats known n-grams; a column whose every row is removed ("qzx", only in "qzxj")."""
    rng = np.random.default_rng(17)
    distinct = lambda k: _SYMBOLS[:k + 2] if k else "ab"          # k + 2 different characters: k different 3-grams
    long_row = "".join(rng.choice(list(_SYMBOLS), 400))
    original = [distinct(k) for k in ROW_LENGTHS] + [long_row, "a" * 70_000, "ab" * 3_000, "qzxj", "abcabcabcab bcd",
                                                    "aaab aaab aaa b", "hooli inc", "hooli", "acme corp", "acme corporation",
                                                    "globex inc", "globex incorporated", "initech llc", "initech"]
    original += ["".join(rng.choice(list(_SYMBOLS[:12]), int(rng.integers(3, 40)))) for _ in range(40)]
    appended = ["!!??", "hooli incorporated", "acme acme acme corp", "ab" * 50 + "cde", distinct(17)[::-1], "", long_row[:200],
                "globex globex", "initech initech llc"]
    appended += ["".join(rng.choice(list(_SYMBOLS[:14]), int(rng.integers(3, 30)))) for _ in range(20)]
    grown = original + appended
    removed = sorted({original.index("qzxj"), original.index("hooli"), original.index("globex inc"), len(original) - 2,
                      len(original) - 1, len(original) + 1, len(grown) - 1, 35, 36})
    live = [s for i, s in enumerate(grown) if i not in set(removed)]
    return tuple(original), tuple(appended), tuple(removed), tuple(live)
