"""Engine double with the corpus operations of string_grouper_amd.engine.HipEngine, computed by the oracle: sklearn's
TfidfVectorizer fitted on the corpus once, its transform for every other Series.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
from sklearn.feature_extraction.text import TfidfVectorizer

from oracle import oracle as O
from tests._oracle_engine import HostMatrix, OracleEngine


class CorpusHostMatrix(HostMatrix):
    def __init__(self, m, corpus):
        super().__init__(m)
        self.corpus = corpus


class OracleCorpus:
    def __init__(self, strings, dtype, **ngram_kw):
        self.vec = TfidfVectorizer(min_df=1, analyzer=lambda s: O.ngrams(s, **ngram_kw), dtype=dtype)
        self.vec.fit(list(strings))
        self.matrix = CorpusHostMatrix(self.vec.transform(list(strings)), self)
        self.index = None
        self.stats = {"tokenisations": 1, "index_builds": 0, "transforms": 0, "resident_index": 0, "forward": 0,
                      "reverse": 0, "reverse_fallbacks": 0}


class CorpusOracleEngine(OracleEngine):
    name = "oracle-corpus"

    def corpus_fit(self, strings, ngram_size, regex, ignore_case, normalize_to_ascii, dtype):
        return OracleCorpus(strings, dtype, ngram_size=ngram_size, regex=regex, ignore_case=ignore_case,
                            normalize_to_ascii=normalize_to_ascii)

    def corpus_transform(self, state, strings):
        state.stats["transforms"] += 1
        return HostMatrix(state.vec.transform(list(strings)))

    def corpus_matrix(self, state):
        return state.matrix

    def corpus_index(self, state):
        if state.index is None:
            state.index = state.matrix.m.T.tocsr()
            state.stats["index_builds"] += 1
        return state.index

    def corpus_free(self, state):
        state.index = None
        state.matrix = None

    def topn_multiply(self, A, B, top_n, threshold):
        if isinstance(B, CorpusHostMatrix):
            self.corpus_index(B.corpus)
            B.corpus.stats["resident_index"] += 1
        elif isinstance(A, CorpusHostMatrix):
            A.corpus.stats["forward"] += 1
        return super().topn_multiply(A, B, top_n, threshold)


def fixed_corpus_matrices(corpus, sets, dtype=np.float64, **ngram_kw):
    """The oracle definition: TfidfVectorizer(...).fit(corpus), then .transform() of every set."""
    mats, vocab, idf = O.tfidf_sklearn(list(corpus), [list(s) for s in sets], dtype=dtype, **ngram_kw)
    return mats, vocab, idf
