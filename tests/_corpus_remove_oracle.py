"""The corpus engine double that grows (tests/_corpus_append_oracle.py) with the operation that takes rows out, computed by
scipy: the matrix of the remaining rows is m[keep] of the rows the vectoriser fitted on the ORIGINAL corpus gave.  TEST
INFRASTRUCTURE ONLY."""
import numpy as np

from tests._corpus_append_oracle import AppendCorpusOracleEngine
from tests._corpus_oracle import CorpusHostMatrix


class RemoveCorpusOracleEngine(AppendCorpusOracleEngine):
    name = "oracle-corpus-remove"

    def corpus_fit(self, *args, **kwargs):
        state = super().corpus_fit(*args, **kwargs)
        state.stats.update(removals=0, rows_removed=0, dead_rows=0)
        return state

    def corpus_remove(self, state, positions):
        positions = np.asarray(positions, dtype=np.int64)
        if len(positions) == 0:
            return
        keep = np.ones(state.matrix.m.shape[0], dtype=bool)
        keep[positions] = False
        state.matrix = CorpusHostMatrix(state.matrix.m[keep], state)
        state.index = None                    # (one piece, nothing pending: the double has no tombstones)
        state.stats["removals"] += 1
        state.stats["rows_removed"] += len(positions)
