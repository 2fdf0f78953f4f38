"""Record matching: what one call of ``Corpus.match_records`` / ``group_similar_records`` asks of the engine, as one value.

``checked_record_call`` turns the caller's options into a ``RecordCall`` -- every check, message and default of them in one
place -- and ``RecordCall`` holds the invariants the device calls rest on, so that a description made by hand is checked
where the corpus's is.  ``Corpus`` hands it to ``CorpusEngine.corpus_records`` as it is."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

MAX_RECORD_FIELDS = 7                         # further fields of a record call (include/sg_hip.h: sg_topn_rescore)
MAX_RECORD_CANDIDATES = 2048                  # candidates a record: the stride sg_topn_rescore and sg_topn_union take


@dataclass(frozen=True)
class RecordCall:
    """One record call.  ``weights``: one a field, the corpus's first; ``candidate_fields``: the fields whose multiplies find
    the candidates, ``(0,)`` for the corpus alone; ``candidates``: ``(max_n_matches, min_similarity)`` a candidate field;
    ``floors``: None or one entry a field, each None or a number, not all None; ``field_scores``: a score column a field;
    ``skip_empty``: a field empty for a pair takes no part in it."""
    weights: Tuple[float, ...]
    candidate_fields: Tuple[int, ...]
    candidates: Tuple[Tuple[int, float], ...]
    floors: Optional[Tuple[Optional[float], ...]] = None
    field_scores: bool = False
    skip_empty: bool = False

    def __post_init__(self):
        floors = None if self.floors is None else tuple(None if m is None else float(m) for m in self.floors)
        for name, value in (("weights", tuple(map(float, self.weights))), ("candidate_fields", tuple(map(int, self.candidate_fields))),
                            ("candidates", tuple((int(k), float(m)) for k, m in self.candidates)), ("floors", floors),
                            ("field_scores", bool(self.field_scores)), ("skip_empty", bool(self.skip_empty))):
            object.__setattr__(self, name, value)         # (frozen: normalised once, here)
        n, fields = self.n_fields, self.candidate_fields
        if not 2 <= n <= MAX_RECORD_FIELDS + 1 or not all(np.isfinite(self.weights)):
            raise ValueError(f"{n} weights: 2 to {MAX_RECORD_FIELDS + 1} fields, a finite weight each, are expected")
        if 0 not in fields or any(a >= b for a, b in zip(fields, fields[1:])) or fields[-1] >= n:
            raise ValueError(f"candidate_fields={fields}: distinct ascending positions below {n}, 0 among them, are expected")
        if len(self.candidates) != len(fields) or any(k < 1 for k, _ in self.candidates):
            raise ValueError(f"candidates={self.candidates}: one (max_n_matches >= 1, min_similarity) a candidate field is expected")
        if self.all_candidates > MAX_RECORD_CANDIDATES:
            raise ValueError(f"the candidate fields' max_n_matches exceed {MAX_RECORD_CANDIDATES} together")
        if self.floors is not None and (len(self.floors) != n or all(m is None for m in self.floors)
                                        or not all(np.isfinite(m) for m in self.floors if m is not None)):
            raise ValueError(f"floors={self.floors}: None, or one finite floor or None a field, not all None, is expected")

    @property
    def n_fields(self) -> int:
        return len(self.weights)

    @property
    def union(self) -> bool:
        return self.candidate_fields != (0,)

    @property
    def all_candidates(self) -> int:
        return sum(k for k, _ in self.candidates)

    @property
    def needs(self) -> frozenset:
        """The options of this call beyond the original one (an engine's ``RECORD_OPTIONS`` must hold them)."""
        used = dict(union=self.union, floors=self.floors is not None, field_scores=self.field_scores, skip_empty=self.skip_empty)
        return frozenset(name for name, on in used.items() if on)


def checked_record_call(configs, n_right: int, weights, candidates, candidate_fields=(0,), field_min_similarity=None,
                        field_similarities=False, empty_fields="zero") -> RecordCall:
    """The options of a record call, checked, as a ``RecordCall``.  ``configs``: every field's ``StringGrouperConfig``, the
    corpus's first (they fill what a ``candidates`` dict leaves out); ``n_right``: what ``max_n_matches=None`` takes."""
    n_others = len(configs) - 1
    # weights: one a field, this corpus's first; used as given
    if weights is None:
        weights = [1.0 / (n_others + 1)] * (n_others + 1)
    else:
        try:
            weights = [float(w) for w in weights]
        except (TypeError, ValueError):
            raise TypeError("weights must be numbers, one for every field (this corpus's first)")
        if len(weights) != n_others + 1:
            raise ValueError(f"{len(weights)} weights for {n_others + 1} fields: one a field is expected, this corpus's first")
        if not all(np.isfinite(w) and w > 0 for w in weights):
            raise ValueError("weights must be finite and greater than 0")
    # candidate_fields: the fields whose multiplies find the candidates (0: this corpus, k: others[k - 1])
    if isinstance(candidate_fields, (str, bytes)) or not hasattr(candidate_fields, "__iter__"):
        raise TypeError("candidate_fields must be a sequence of field positions (0: this corpus, k: others[k - 1])")
    candidate_fields = tuple(candidate_fields)
    if not all(isinstance(f, (int, np.integer)) and not isinstance(f, (bool, np.bool_)) for f in candidate_fields):
        raise TypeError("candidate_fields must be a sequence of field positions (0: this corpus, k: others[k - 1])")
    candidate_fields = tuple(int(f) for f in candidate_fields)
    if not all(0 <= f <= n_others for f in candidate_fields):
        raise ValueError(f"candidate_fields={candidate_fields}: positions between 0 and {n_others} are expected for "
                         f"{n_others + 1} fields")
    if 0 not in candidate_fields or any(a >= b for a, b in zip(candidate_fields, candidate_fields[1:])):
        raise ValueError(f"candidate_fields={candidate_fields}: distinct positions in ascending order, 0 (this corpus) among "
                         f"them, are expected")
    # field_min_similarity: one floor a field, this corpus's first; None -- the whole or an entry -- is no floor
    floors = None
    if field_min_similarity is not None:
        if isinstance(field_min_similarity, (str, bytes)) or not hasattr(field_min_similarity, "__len__"):
            raise TypeError("field_min_similarity must be a sequence, one entry for every field (this corpus's first): a "
                            "number or None")
        floors = list(field_min_similarity)
        if len(floors) != n_others + 1:
            raise ValueError(f"{len(floors)} entries of field_min_similarity for {n_others + 1} fields: one a field is "
                             f"expected, this corpus's first")
        for k, m in enumerate(floors):
            if isinstance(m, (bool, np.bool_)):
                raise TypeError(f"field_min_similarity[{k}]={m!r}: a number or None is expected, not a bool")
            if m is None:
                continue
            if not isinstance(m, (int, float, np.integer, np.floating)) or not np.isfinite(m):
                raise ValueError(f"field_min_similarity[{k}]={m!r}: a finite real number or None is expected")
            floors[k] = float(m)
        if all(m is None for m in floors):               # no floor anywhere: the call it always was
            floors = None
    # field_similarities: a column a field in the frame
    if not isinstance(field_similarities, (bool, np.bool_)):
        raise TypeError(f"field_similarities={field_similarities!r}: True or False is expected")
    # empty_fields: "zero" -- the call as it always was -- or "skip"
    if not isinstance(empty_fields, str):
        raise TypeError(f"empty_fields={empty_fields!r}: 'zero' or 'skip' is expected")
    if empty_fields not in ("zero", "skip"):
        raise ValueError(f"empty_fields={empty_fields!r}: 'zero' or 'skip' is expected")
    # candidates: the two options of a candidate field's multiply -- one dict for every candidate field, or one a field
    candidates = {} if candidates is None else candidates
    if isinstance(candidates, list) and all(isinstance(c, dict) for c in candidates):
        if len(candidates) != len(candidate_fields):
            raise ValueError(f"{len(candidates)} candidates dicts for {len(candidate_fields)} candidate fields: one a "
                             f"candidate field (or one for all) is expected")
    else:
        candidates = [candidates] * len(candidate_fields)
    cand = []
    for f, options_f in zip(candidate_fields, candidates):
        if not isinstance(options_f, dict) or set(options_f) - {"min_similarity", "max_n_matches"}:
            raise TypeError("candidates takes min_similarity and max_n_matches only, as a dict")
        config = configs[f]                              # a field's own corpus fills what the dict leaves out
        cand_threshold = float(options_f.get("min_similarity", config.min_similarity))
        cand_top_n = options_f.get("max_n_matches", config.max_n_matches)
        if cand_top_n is None:
            cand_top_n = n_right
        if isinstance(cand_top_n, (bool, np.bool_)) or not isinstance(cand_top_n, (int, np.integer)) or cand_top_n < 1:
            if n_right > 0:
                raise ValueError(f"candidates: max_n_matches={cand_top_n!r}: a whole number of at least 1 is expected")
            cand_top_n = 1
        if cand_top_n > MAX_RECORD_CANDIDATES:
            raise ValueError(f"candidates: max_n_matches={cand_top_n} exceeds the {MAX_RECORD_CANDIDATES} candidates a record "
                             f"that can be rescored: set candidates=dict(max_n_matches=...) to at most that")
        cand.append((int(cand_top_n), cand_threshold))
    if sum(k for k, _ in cand) > MAX_RECORD_CANDIDATES:
        raise ValueError(f"candidates: the max_n_matches of the candidate fields {list(candidate_fields)} "
                         f"({' + '.join(str(k) for k, _ in cand)}) exceed together the {MAX_RECORD_CANDIDATES} candidates a "
                         f"record that can be united and rescored")
    return RecordCall(weights, candidate_fields, cand, floors, field_similarities, empty_fields == "skip")
