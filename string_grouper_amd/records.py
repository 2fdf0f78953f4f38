"""Record matching: several fields a record, one combined similarity.

``match_records`` is the module-level form of ``Corpus.match_records`` (string_grouper_amd/corpus.py): it fits one corpus a
field on its inputs, as ``match_strings`` fits its vectoriser, calls and closes them.  A service that matches against the same
records again keeps the corpora instead."""
from __future__ import annotations

from typing import Optional

import pandas as pd

from .corpus import Corpus


def match_records(fields, duplicates=None, master_id: Optional[pd.Series] = None, duplicates_id: Optional[pd.Series] = None,
                  weights=None, candidates=None, candidate_fields=(0,), field_min_similarity=None,
                  field_similarities=False, empty_fields="zero", **kwargs) -> pd.DataFrame:
    """``fields``: a list of 2 to 8 equally long Series, one a field of the records; the first finds the candidates --
    with ``candidate_fields`` (positions in ``fields``, 0 among them) the union of several fields' matches does.
    ``field_min_similarity``: None or one floor a field (a number or None), in the order of ``fields``.
    ``field_similarities=True``: a column ``similarity_k`` a field in the frame, k the position in ``fields``.
    ``empty_fields``: ``"zero"`` (the default) or ``"skip"``: a field that is empty for a pair -- a string with no n-gram its
    field knows, on either side -- takes no part in that pair and its weight is shared among the others.
    ``duplicates``: None or as many Series.  Everything else as in ``Corpus.match_records``; vectoriser options in
    ``kwargs`` (``ngram_size``, ``tfidf_matrix_dtype`` ...) apply to every field."""
    if isinstance(fields, pd.Series) or not isinstance(fields, (list, tuple)) or len(fields) < 2:
        raise TypeError("fields must be a list of at least two pandas.Series, one for every field of the records")
    if len({len(f) for f in fields}) != 1:
        raise ValueError("the fields differ in length: row p of every Series must be record p")
    corpora = []
    try:
        for k, series in enumerate(fields):
            corpora.append(Corpus(series, master_id=master_id if k == 0 else None, **kwargs))
        return corpora[0].match_records(corpora[1:], duplicates=duplicates, duplicates_id=duplicates_id, weights=weights,
                                        candidates=candidates, candidate_fields=candidate_fields,
                                        field_min_similarity=field_min_similarity, field_similarities=field_similarities,
                                        empty_fields=empty_fields, **kwargs)
    finally:
        for c in corpora:
            c.close()
