"""The corpus engine double (tests/_corpus_oracle.py) with the operations that grow a corpus, computed by sklearn and scipy:
the appended strings go through the transform of the vectoriser fitted on the ORIGINAL corpus and are stacked under its
rows.  TEST INFRASTRUCTURE ONLY."""
import scipy.sparse as sp

from tests._corpus_oracle import CorpusHostMatrix, CorpusOracleEngine


class AppendCorpusOracleEngine(CorpusOracleEngine):
    name = "oracle-corpus-append"

    def corpus_fit(self, *args, **kwargs):
        state = super().corpus_fit(*args, **kwargs)
        state.stats.update(appends=0, rows_appended=0, compactions=0, segments=1, base_index_builds=0)
        return state

    def corpus_append(self, state, strings):
        if len(strings) == 0:
            return
        new = state.vec.transform(list(strings))
        state.matrix = CorpusHostMatrix(sp.vstack([state.matrix.m, new]).tocsr(), state)
        state.index = None                    # (one piece: the double has no segments to keep)
        state.stats["appends"] += 1
        state.stats["rows_appended"] += len(strings)

    def corpus_compact(self, state):
        state.stats["compactions"] += 1
