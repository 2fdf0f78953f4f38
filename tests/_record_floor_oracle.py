"""Record matching with per-field floors for the tests: the COMPOSED ROUTE with floors -- ``combined_pairs``' steps of
tests/_record_oracle.py with the floor mask between the sum and the filter -- that ``match_records(field_min_similarity=...)``
replaces, for the CPU and the GPU tests alike.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import pandas as pd
import scipy.sparse as sp

from string_grouper_amd.string_grouper import StringGrouper


def combined_pairs_floors(corpus, others, weights, candidates, min_similarity, max_n_matches, floors, duplicates=None,
                          duplicates_id=None):
    """``combined_pairs`` of tests/_record_oracle.py with the floors: (frame of match_strings at the candidate options, the
    keep-and-order index into it, the combined similarity of every row, left and right positions, the fields' scores)."""
    T = np.dtype(corpus._config.tfidf_matrix_dtype).type
    kw = dict(force_symmetries=False, **candidates)
    master = corpus.master
    if duplicates is None:
        frame = corpus.match_strings(master, master_id=corpus.master_id, **kw)
        right_labels = master.index
    else:
        frame = corpus.match_strings(master, duplicates[0], corpus.master_id, duplicates_id, **kw)
        right_labels = duplicates[0].index
    lp = pd.Index(master.index).get_indexer(frame["left_index"])
    rp = pd.Index(right_labels).get_indexer(frame["right_index"])
    assert (lp >= 0).all() and (rp >= 0).all()
    scores = [frame["similarity"].to_numpy().astype(T)]                       # widened from T: the cast back is exact
    for k, o in enumerate(others):
        scores.append(o.pair_similarities(lp, rp) if duplicates is None else o.pair_similarities(lp, rp, duplicates=duplicates[k + 1]))
    W = [T(w) for w in weights]
    acc = np.zeros(len(frame), T)
    for f in range(len(W)):
        acc = acc + W[f] * scores[f]
    assert acc.dtype == T
    passed = np.ones(len(frame), bool)                                        # the mask: between the sum and the filter
    for s, m in zip(scores, floors or [None] * len(scores)):
        if m is not None:
            passed &= s > T(m)
    keep = np.flatnonzero(passed & (acc > T(min_similarity)))
    order = keep[np.lexsort((rp[keep], -acc[keep], lp[keep]))]                # by record, combined descending, right position
    rank = np.arange(len(order)) - np.searchsorted(lp[order], lp[order], side="left")
    order = order[rank < max_n_matches]
    if T == np.float32:                                                       # a float32 list comes back with rows by column
        order = order[np.lexsort((rp[order], lp[order]))]
    return frame, order, acc, lp, rp, scores


def composed_route_floors(corpus, others, weights, candidates, min_similarity, max_n_matches, floors, duplicates=None,
                          duplicates_id=None):
    """The frame ``match_records(..., field_min_similarity=floors, force_symmetries=False)`` must equal."""
    frame, order, acc, _, _, _ = combined_pairs_floors(corpus, others, weights, candidates, min_similarity, max_n_matches, floors,
                                                       duplicates, duplicates_id)
    out = frame.iloc[order].reset_index(drop=True)
    out["similarity"] = acc[order].astype(np.float64)
    return out


def composed_groups_floors(corpus, others, weights, candidates, min_similarity, max_n_matches, floors, **kwargs):
    """``composed_groups`` of tests/_record_oracle.py over the list of the composed route with floors."""
    frame, order, acc, lp, rp, _ = combined_pairs_floors(corpus, others, weights, candidates, min_similarity, max_n_matches, floors)
    n = len(corpus.master)
    m = sp.coo_matrix((acc[order].astype(np.float64), (lp[order], rp[order])), shape=(n, n))
    g = StringGrouper(corpus.master, master_id=corpus.master_id, min_similarity=min_similarity, max_n_matches=max_n_matches,
                      **kwargs)
    g._true_max_n_matches = int(np.bincount(lp[order], minlength=n).max())
    g._matches_list = g._get_matches_list(StringGrouper._symmetrize_matrix(StringGrouper._fix_diagonal(m)))
    g.is_build = True
    return g.get_groups()


def composed_union_route_floors(corpus, others, weights, candidates, candidate_fields, min_similarity, max_n_matches, floors,
                                duplicates=None, duplicates_id=None):
    """``composed_union_route`` of tests/_record_union_oracle.py with the floors: the candidate fields' match_strings frames
    united in pandas, every field's ``pair_similarities``, the sum, the floor mask, the filter, the order and the cut."""
    from tests._record_union_oracle import _grouper, _per_field
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
    W = [T(w) for w in weights]
    acc = np.zeros(len(lp), T)
    for f in range(len(W)):
        acc = acc + W[f] * scores[f]
    passed = np.ones(len(lp), bool)
    for s, m in zip(scores, floors):
        if m is not None:
            passed &= s > T(m)
    keep = np.flatnonzero(passed & (acc > T(min_similarity)))
    order = keep[np.lexsort((rp[keep], -acc[keep], lp[keep]))]
    rank = np.arange(len(order)) - np.searchsorted(lp[order], lp[order], side="left")
    order = order[rank < max_n_matches]
    if T == np.float32:
        order = order[np.lexsort((rp[order], lp[order]))]
    g = _grouper(corpus, lp[order], rp[order], acc[order], min_similarity, max_n_matches, duplicates, duplicates_id)
    g._matches_list = pd.DataFrame({"master_side": lp[order], "dupe_side": rp[order], "similarity": acc[order].astype(np.float64)})
    g.is_build = True
    return g.get_matches()
