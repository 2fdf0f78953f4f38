"""The corpus engine double that grows, forgets, keeps a self-join and refits (tests/_corpus_refit_oracle.py) with the scoring
of named pairs, computed by the numpy statement of tests/_pair_cases.py on the double's scipy matrices.  TEST INFRASTRUCTURE
ONLY."""
import numpy as np

from tests._corpus_refit_oracle import RefitCorpusOracleEngine
from tests._pair_cases import ref_pairs_dot


class PairCorpusOracleEngine(RefitCorpusOracleEngine):
    name = "oracle-corpus-pairs"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.pair_calls = []                  # (rows of A, rows of B, pairs) of every call that reached the engine

    def corpus_fit(self, *args, **kwargs):
        state = super().corpus_fit(*args, **kwargs)
        state.stats.update(pair_calls=0, pairs_scored=0)
        return state

    def pairs_dot(self, A, B, left, right):
        self.pair_calls.append((A.shape[0], B.shape[0], len(left)))
        return ref_pairs_dot(A.m, B.m, np.asarray(left), np.asarray(right))

    def corpus_pairs(self, state, left, right, other=None):
        state.stats["pair_calls"] += 1
        state.stats["pairs_scored"] += len(left)
        return self.pairs_dot(state.matrix, state.matrix if other is None else other, left, right)
