"""Record matching for the tests: the corpus engine double that scores named pairs (tests/_pair_oracle.py) with the engine method
of ``Corpus.match_records``, computed by ``ref_rescore`` (tests/_rescore_cases.py) on the double's scipy matrices, and the
COMPOSED ROUTE -- ``match_strings`` at the candidate options, ``pair_similarities`` a further corpus, the numpy chain, ``>``, the
order and the cut in pandas -- that ``match_records`` replaces, for the CPU and the GPU tests alike.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import pandas as pd
import scipy.sparse as sp

from string_grouper_amd.string_grouper import StringGrouper
from tests._pair_oracle import PairCorpusOracleEngine
from tests._rescore_cases import Case, Field, ref_rescore


class RecordCorpusOracleEngine(PairCorpusOracleEngine):
    name = "oracle-corpus-records"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.record_calls = []                # (candidate rows, further fields) of every call that reached the engine

    def corpus_fit(self, *args, **kwargs):
        state = super().corpus_fit(*args, **kwargs)
        state.stats.update(record_calls=0)
        return state

    def corpus_records_topn(self, state, others, B, B_fields, weights, cand_top_n, cand_threshold, top_n, threshold,
                            self_join_fix):
        A = state.matrix
        self_join = B_fields is None
        cand = sp.csr_matrix(self.topn_multiply(A, B, cand_top_n, cand_threshold))      # rows by score descending, then column
        T = A.dtype.type
        R, N = cand.shape
        stride = max(min(int(cand_top_n), N), 1)
        counts = np.diff(cand.indptr).astype(np.int32)
        cols, vals = np.zeros((R, stride), np.int32), np.zeros((R, stride), T)
        for r in range(R):
            cols[r, :counts[r]] = cand.indices[cand.indptr[r]:cand.indptr[r + 1]]
            vals[r, :counts[r]] = cand.data[cand.indptr[r]:cand.indptr[r + 1]]
        fields = []
        for k, o in enumerate(others):
            left = sp.csr_matrix(o.matrix.m)
            left.sort_indices()
            right = left if self_join else sp.csr_matrix(B_fields[k].m)
            right.sort_indices()
            fields.append(Field(left, right, weights[k + 1], None, None))
        self.record_calls.append((R, len(fields)))
        for st in [state] + list(others):
            st.stats["record_calls"] += 1
        out_c, out_v, out_n = ref_rescore(Case(cols, vals, counts, N, weights[0], fields, threshold, top_n))
        true_max = int(out_n.max()) if R else 0
        mask = np.arange(out_c.shape[1])[None, :] < out_n[:, None]
        rows = np.repeat(np.arange(R, dtype=np.int64), out_n)
        cc, vv = out_c[mask].astype(np.int64), out_v[mask]
        if self_join_fix:                     # diagonal := 1, symmetrised, rows by column (StringGrouper's own two steps)
            m = StringGrouper._symmetrize_matrix(StringGrouper._fix_diagonal(sp.coo_matrix((vv, (rows, cc)), shape=(R, N))))
            rows = np.repeat(np.arange(R, dtype=np.int64), np.diff(m.indptr))
            return rows, m.indices.astype(np.int64), m.data.astype(T), true_max
        if T == np.float32:                   # the reference's up-cast re-sorts a float32 result's rows by column
            order = np.lexsort((cc, rows))
            cc, vv = cc[order], vv[order]
        return rows, cc, vv, true_max


# ------------------------------------------------------------------------------------------ the composed route
def combined_pairs(corpus, others, weights, candidates, min_similarity, max_n_matches, duplicates=None, duplicates_id=None):
    """(frame of match_strings at the candidate options with force_symmetries=False, keep-and-order index into it, combined
    similarity of every row of it): what a caller without ``match_records`` does today."""
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
    keep = np.flatnonzero(acc > T(min_similarity))
    order = keep[np.lexsort((rp[keep], -acc[keep], lp[keep]))]                # by record, combined descending, right position
    rank = np.arange(len(order)) - np.searchsorted(lp[order], lp[order], side="left")
    order = order[rank < max_n_matches]
    if T == np.float32:                                                       # a float32 list comes back with rows by column
        order = order[np.lexsort((rp[order], lp[order]))]
    return frame, order, acc, lp, rp


def composed_route(corpus, others, weights, candidates, min_similarity, max_n_matches, duplicates=None, duplicates_id=None):
    """The frame ``match_records(..., force_symmetries=False)`` must equal."""
    frame, order, acc, _, _ = combined_pairs(corpus, others, weights, candidates, min_similarity, max_n_matches, duplicates,
                                             duplicates_id)
    out = frame.iloc[order].reset_index(drop=True)
    out["similarity"] = acc[order].astype(np.float64)
    return out


def composed_groups(corpus, others, weights, candidates, min_similarity, max_n_matches, **kwargs):
    """``group_similar_strings`` fed with the combined list: StringGrouper's own host steps (diagonal := 1, symmetrised) and
    its own ``get_groups`` over the list of the composed route."""
    frame, order, acc, lp, rp = combined_pairs(corpus, others, weights, candidates, min_similarity, max_n_matches)
    n = len(corpus.master)
    m = sp.coo_matrix((acc[order].astype(np.float64), (lp[order], rp[order])), shape=(n, n))
    g = StringGrouper(corpus.master, master_id=corpus.master_id, min_similarity=min_similarity, max_n_matches=max_n_matches,
                      **kwargs)
    g._true_max_n_matches = int(np.bincount(lp[order], minlength=n).max())
    g._matches_list = g._get_matches_list(StringGrouper._symmetrize_matrix(StringGrouper._fix_diagonal(m)))
    g.is_build = True
    return g.get_groups()
