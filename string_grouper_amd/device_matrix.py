"""What the engine hands to the front end, resident in HBM: a TF-IDF matrix, the match list of one fit(), and the row blocks
both are cut into.  A leaf: it knows the binding and nothing of the engines above it."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import scipy.sparse as sp

from . import _native as N


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
