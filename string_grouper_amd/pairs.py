"""Pair similarities: how similar are these two particular records, whose positions are known?

The top-n questions (``match_strings`` and the others) answer "which rows are most like this row"; this one scores NAMED pairs
-- the candidate pairs of a record linkage scored on a second field, a reviewed pair list scored again after ``refit_idf()``.
The reference's only offer is ``compute_pairwise_similarities(series_1, series_2)`` (string_grouper.py:55), which has to be
handed both rows of every pair as strings, vectorises all of them again and sums in numpy's order.  Here a pair names two rows
of matrices that are already on the device, and the score is the element of the multiply's product for that pair, in the
multiply's arithmetic (include/sg_hip.h: sg_csr_pairs_dot):

    for every pair (i, j) that ``match_strings`` reports for the same matrices, ``pair_similarities`` gives the same bits --
    but for the diagonal of a self-join, which the frames set to 1 (``_fix_diagonal``) whatever the product gives.

``Corpus.pair_similarities`` (string_grouper_amd/corpus.py) is the resident form; ``pair_similarities`` below fits on its
inputs as ``match_strings`` does."""
from __future__ import annotations

from typing import Optional

import numpy as np
import pandas as pd

from . import engine as _engine_mod
from .string_grouper import StringGrouper


def pair_positions(values, n: int, what: str) -> np.ndarray:
    """``values`` -- a sequence or array of ints, negative ones counting from the end -- as positions in [0, n), int64, in
    the order given.  Bools and non-integers: TypeError; a position outside [-n, n): IndexError."""
    if isinstance(values, (bool, np.bool_, int, np.integer, float, str, bytes)) or values is None:
        raise TypeError(f"{what} must be a sequence or array of integer positions, not {type(values).__name__}")
    try:
        arr = np.asarray(values)
    except Exception:
        raise TypeError(f"{what} must be a sequence or array of integer positions")
    if arr.ndim != 1:
        raise TypeError(f"{what} must be one-dimensional: a sequence of integer positions")
    if arr.size == 0:
        return np.zeros(0, np.int64)
    if arr.dtype.kind not in "iu":
        raise TypeError(f"{what} must hold integer positions, not {arr.dtype}")
    if arr.dtype.kind == "u" and arr.max() > np.iinfo(np.int64).max:
        raise IndexError(f"a position of {what} lies outside [{-n}, {n}): there are {n} rows")
    arr = arr.astype(np.int64)
    if arr.min() < -n or arr.max() >= n:
        raise IndexError(f"a position of {what} lies outside [{-n}, {n}): there are {n} rows")
    return np.where(arr < 0, arr + n, arr)


def checked_pairs(left, right, n_left: int, n_right: int):
    """(left, right) as positions; lists of different lengths: ValueError."""
    left, right = pair_positions(left, n_left, "left"), pair_positions(right, n_right, "right")
    if len(left) != len(right):
        raise ValueError(f"left names {len(left)} rows and right {len(right)}: a pair needs one of each")
    return left, right


def pair_similarities(master: pd.Series, left, right, duplicates: Optional[pd.Series] = None, **kwargs) -> np.ndarray:
    """The similarity of ``master[left[p]]`` and ``master[right[p]]`` -- with ``duplicates``: ``duplicates[right[p]]`` -- for
    every p: a numpy array of ``tfidf_matrix_dtype``, one entry a pair, in the order given.  The vectoriser is fitted as
    ``match_strings(master, duplicates, **kwargs)`` fits it, and every pair that call reports has the same bits here (the
    diagonal of a self-join apart, which the frames set to 1).  ``left`` / ``right``: positions (not labels), negative ones
    count from the end.  A ``Corpus`` answers the same question without fitting again (``Corpus.pair_similarities``)."""
    grouper = StringGrouper(master, duplicates=duplicates, **kwargs)          # the reference's validation of data and options
    n_right = len(master) if duplicates is None else len(duplicates)
    left, right = checked_pairs(left, right, len(master), n_right)
    if len(left) == 0:
        return np.zeros(0, grouper._config.tfidf_matrix_dtype)
    eng = _engine_mod.get_engine()
    if not hasattr(eng, "pairs_dot"):
        raise NotImplementedError(f"the engine {getattr(eng, 'name', type(eng).__name__)!r} scores no pairs")
    A, B = grouper._tfidf_on_engine()
    try:
        return eng.pairs_dot(A, B, left, right)
    finally:
        for m in {id(A): A, id(B): B}.values():
            csr = getattr(m, "csr", None)
            if csr is not None:
                csr.free()
