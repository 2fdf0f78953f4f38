"""Record matching with candidates from several fields, for the tests: the COMPOSED UNION ROUTE that ``candidate_fields``
replaces -- ``match_strings`` a candidate field at its candidate options, the union of the position pairs in pandas,
``pair_similarities`` on every field (the primary included), then ``combined_pairs``' chain of tests/_record_oracle.py -- numpy's
weighted sum, ``>``, the order and the cut.  The diagonal of a self-join is a pair like any other, as in ``combined_pairs``.
TEST INFRASTRUCTURE ONLY."""
import numpy as np
import pandas as pd
import scipy.sparse as sp

from string_grouper_amd.string_grouper import StringGrouper


# ------------------------------------------------------------------------------------------ the composed union route
def _per_field(candidates, n):
    return list(candidates) if isinstance(candidates, list) else [candidates] * n


def union_pairs(corpus, others, weights, candidates, candidate_fields, min_similarity, max_n_matches, duplicates=None):
    """(left positions, right positions, combined similarity) of the surviving pairs, in the list's order: what a caller without
    ``candidate_fields`` does today."""
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
        lp = pd.Index(c.master.index).get_indexer(frame["left_index"])
        rp = pd.Index(right_labels).get_indexer(frame["right_index"])
        assert (lp >= 0).all() and (rp >= 0).all()
        found.append(pd.DataFrame({"left": lp, "right": rp}))
    pairs = pd.concat(found, ignore_index=True).drop_duplicates(ignore_index=True)        # the union, in pandas
    lp, rp = pairs["left"].to_numpy(np.int64), pairs["right"].to_numpy(np.int64)
    scores = [c.pair_similarities(lp, rp) if duplicates is None else c.pair_similarities(lp, rp, duplicates=duplicates[k])
              for k, c in enumerate(corpora)]                                             # every field, the primary included
    W = [T(w) for w in weights]
    acc = np.zeros(len(lp), T)
    for f in range(len(W)):
        acc = acc + W[f] * scores[f]
    assert acc.dtype == T
    keep = np.flatnonzero(acc > T(min_similarity))
    order = keep[np.lexsort((rp[keep], -acc[keep], lp[keep]))]                            # by record, combined descending, right position
    rank = np.arange(len(order)) - np.searchsorted(lp[order], lp[order], side="left")
    order = order[rank < max_n_matches]
    if T == np.float32:                                                                   # a float32 list comes back with rows by column
        order = order[np.lexsort((rp[order], lp[order]))]
    return lp[order], rp[order], acc[order], len(found[0]), len(pairs)


def _grouper(corpus, lp, rp, acc, min_similarity, max_n_matches, duplicates=None, duplicates_id=None, **kwargs):
    """StringGrouper's own frames over a list made elsewhere."""
    g = StringGrouper(corpus.master, None if duplicates is None else duplicates[0], corpus.master_id, duplicates_id,
                      min_similarity=min_similarity, max_n_matches=max_n_matches, **kwargs)
    g._true_max_n_matches = int(np.bincount(lp, minlength=len(corpus.master)).max()) if len(lp) else 0
    return g


def composed_union_route(corpus, others, weights, candidates, candidate_fields, min_similarity, max_n_matches, duplicates=None,
                         duplicates_id=None):
    """The frame ``match_records(..., candidate_fields=..., force_symmetries=False)`` must equal."""
    lp, rp, acc, _, _ = union_pairs(corpus, others, weights, candidates, candidate_fields, min_similarity, max_n_matches, duplicates)
    g = _grouper(corpus, lp, rp, acc, min_similarity, max_n_matches, duplicates, duplicates_id)
    g._matches_list = pd.DataFrame({"master_side": lp, "dupe_side": rp, "similarity": acc.astype(np.float64)})
    g.is_build = True
    return g.get_matches()


def composed_union_groups(corpus, others, weights, candidates, candidate_fields, min_similarity, max_n_matches, **kwargs):
    """``group_similar_strings`` fed with the combined list: StringGrouper's own host steps (diagonal := 1, symmetrised) and
    its own ``get_groups`` over the list of the composed union route."""
    lp, rp, acc, _, _ = union_pairs(corpus, others, weights, candidates, candidate_fields, min_similarity, max_n_matches)
    n = len(corpus.master)
    m = sp.coo_matrix((acc.astype(np.float64), (lp, rp)), shape=(n, n))
    g = _grouper(corpus, lp, rp, acc, min_similarity, max_n_matches, **kwargs)
    g._matches_list = g._get_matches_list(StringGrouper._symmetrize_matrix(StringGrouper._fix_diagonal(m)))
    g.is_build = True
    return g.get_groups()
