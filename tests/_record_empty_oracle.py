"""Record matching with empty fields left out, for the tests: the COMPOSED ROUTE that ``match_records(empty_fields="skip")``
replaces -- ``match_strings`` at the candidate options (one a candidate field, united in pandas), ``pair_similarities`` a field,
which strings are empty from the nnz of the rows ``corpus.vectorizer.transform`` gives, then the statement in numpy and pandas:
the sums over the fields that are not empty, ``(c * wt) / wp``, the floors on the fields that are not empty, ``>``, the order
and the cut.  For the CPU and the GPU tests alike.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import pandas as pd
import scipy.sparse as sp

from string_grouper_amd.string_grouper import StringGrouper
from tests._record_union_oracle import _grouper, _per_field


# ------------------------------------------------------------------------------------------ the composed route
def _is_empty(corpus, series):
    """For every string of ``series``: has it no n-gram that the corpus knows?"""
    return np.diff(sp.csr_matrix(corpus.vectorizer.transform(series)).indptr) == 0


def skip_pairs(corpus, others, weights, candidates, min_similarity, max_n_matches, floors=None, duplicates=None,
               candidate_fields=(0,)):
    """(left positions, right positions, similarity of every surviving pair in the list's order, the fields' scores of those
    pairs, [field][pair] is the field empty for it): what a caller without ``empty_fields`` would have to do."""
    T = np.dtype(corpus._config.tfidf_matrix_dtype).type
    corpora = [corpus] + list(others)
    found = []
    for f, cand in zip(candidate_fields, _per_field(candidates, len(candidate_fields))):
        c = corpora[f]
        kw = dict(force_symmetries=False, **cand)
        if duplicates is None:
            frame, right_labels = c.match_strings(c.master, **kw), c.master.index
        else:
            frame, right_labels = c.match_strings(c.master, duplicates[f], **kw), duplicates[f].index
        found.append(pd.DataFrame({"left": pd.Index(c.master.index).get_indexer(frame["left_index"]),
                                   "right": pd.Index(right_labels).get_indexer(frame["right_index"])}))
    pairs = pd.concat(found, ignore_index=True).drop_duplicates(ignore_index=True)
    lp, rp = pairs["left"].to_numpy(np.int64), pairs["right"].to_numpy(np.int64)
    assert (lp >= 0).all() and (rp >= 0).all()
    scores = [c.pair_similarities(lp, rp) if duplicates is None else c.pair_similarities(lp, rp, duplicates=duplicates[k])
              for k, c in enumerate(corpora)]
    empty = []
    for k, c in enumerate(corpora):
        left = _is_empty(c, c.master)
        right = left if duplicates is None else _is_empty(c, duplicates[k])
        empty.append(left[lp] | right[rp])
    W = [T(w) for w in weights]
    acc, wp, wt = np.zeros(len(lp), T), np.zeros(len(lp), T), np.zeros(len(lp), T)
    with np.errstate(all="ignore"):
        for f in range(len(W)):
            acc = np.where(empty[f], acc, acc + W[f] * scores[f]).astype(T)
            wp = np.where(empty[f], wp, wp + W[f]).astype(T)
            wt = wt + W[f]
        some = np.logical_or.reduce(empty)
        scaled = np.where(wp > 0, (acc * wt) / wp, T(np.nan)).astype(T)
    sim = np.where(some, scaled, acc).astype(T)
    assert sim.dtype == T
    passed = np.ones(len(lp), bool)
    for f, m in enumerate(floors or []):
        if m is not None:
            passed &= empty[f] | (scores[f] > T(m))                             # a floor on an empty field is not held
    keep = np.flatnonzero(passed & (sim > T(min_similarity)))
    order = keep[np.lexsort((rp[keep], -sim[keep], lp[keep]))]                  # by record, similarity descending, right position
    rank = np.arange(len(order)) - np.searchsorted(lp[order], lp[order], side="left")
    order = order[rank < max_n_matches]
    if T == np.float32:                                                         # a float32 list comes back with rows by column
        order = order[np.lexsort((rp[order], lp[order]))]
    return lp[order], rp[order], sim[order], [s[order] for s in scores], [e[order] for e in empty]


def composed_route_skip(corpus, others, weights, candidates, min_similarity, max_n_matches, floors=None, duplicates=None,
                        duplicates_id=None, candidate_fields=(0,), field_similarities=False):
    """The frame ``match_records(..., empty_fields="skip", force_symmetries=False)`` must equal."""
    lp, rp, sim, scores, _ = skip_pairs(corpus, others, weights, candidates, min_similarity, max_n_matches, floors, duplicates,
                                        candidate_fields)
    g = _grouper(corpus, lp, rp, sim, min_similarity, max_n_matches, duplicates, duplicates_id)
    g._matches_list = pd.DataFrame({"master_side": lp, "dupe_side": rp, "similarity": sim.astype(np.float64)})
    g.is_build = True
    frame = g.get_matches()
    if field_similarities:
        at = list(frame.columns).index("similarity") + 1
        for k, s in enumerate(scores):
            frame.insert(at + k, f"similarity_{k}", s.astype(np.float64))
    return frame


def composed_groups_skip(corpus, others, weights, candidates, min_similarity, max_n_matches, floors=None, candidate_fields=(0,),
                         **kwargs):
    """``group_similar_strings`` fed with the list of the composed route: StringGrouper's own host steps (diagonal := 1,
    symmetrised) and its own ``get_groups``."""
    lp, rp, sim, _, _ = skip_pairs(corpus, others, weights, candidates, min_similarity, max_n_matches, floors, None, candidate_fields)
    n = len(corpus.master)
    m = sp.coo_matrix((sim.astype(np.float64), (lp, rp)), shape=(n, n))
    g = _grouper(corpus, lp, rp, sim, min_similarity, max_n_matches, **kwargs)
    g._matches_list = g._get_matches_list(StringGrouper._symmetrize_matrix(StringGrouper._fix_diagonal(m)))
    g.is_build = True
    return g.get_groups()
