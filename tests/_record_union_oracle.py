"""Record matching with candidates from several fields, for the tests: the engine double of tests/_record_oracle.py with the
engine method behind ``candidate_fields`` -- built from ``topn_multiply``, ``ref_union`` (tests/_union_cases.py) and
``ref_rescore`` (tests/_rescore_cases.py) on the double's scipy matrices -- and the COMPOSED UNION ROUTE that the call replaces:
``match_strings`` a candidate field at its candidate options, the union of the position pairs in pandas, ``pair_similarities`` on
every field (the primary included), then ``combined_pairs``' chain -- numpy's weighted sum, ``>``, the order and the cut.  The
diagonal of a self-join is a pair like any other, as in ``combined_pairs``.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import pandas as pd
import scipy.sparse as sp

from string_grouper_amd.string_grouper import StringGrouper
from tests._record_oracle import RecordCorpusOracleEngine
from tests._rescore_cases import Case, Field, ref_rescore
from tests._union_cases import Part, UnionCase, ref_union


def _sorted(m):
    m = sp.csr_matrix(m)
    m.sort_indices()
    return m


class RecordUnionOracleEngine(RecordCorpusOracleEngine):
    name = "oracle-corpus-records-union"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.union_calls = []                 # (candidate fields, candidates before the union, after it) of every call

    def corpus_fit(self, *args, **kwargs):
        state = super().corpus_fit(*args, **kwargs)
        state.stats.update(record_union_calls=0)
        return state

    def corpus_records_union_topn(self, state, others, B, B_fields, weights, candidate_fields, cands, top_n, threshold,
                                  self_join_fix, keep_on_device=False):
        states = [state] + list(others)
        self_join = B_fields is None
        T = state.matrix.dtype.type
        parts = []
        for f, (cand_top_n, cand_threshold) in zip(candidate_fields, cands):
            A_f = states[f].matrix
            B_f = A_f if self_join else (B if f == 0 else B_fields[f - 1])
            cand = sp.csr_matrix(self.topn_multiply(A_f, B_f, cand_top_n, cand_threshold))
            R, N = cand.shape
            stride = max(min(int(cand_top_n), N), 1)
            counts = np.diff(cand.indptr).astype(np.int32)
            cols, vals = np.zeros((R, stride), np.int32), np.zeros((R, stride), T)
            for r in range(R):
                cols[r, :counts[r]] = cand.indices[cand.indptr[r]:cand.indptr[r + 1]]
                vals[r, :counts[r]] = cand.data[cand.indptr[r]:cand.indptr[r + 1]]
            parts.append(Part(cols, vals, counts))
        left = _sorted(state.matrix.m)
        u_cols, u_vals, u_counts = ref_union(UnionCase(parts, N, Field(left, left if self_join else _sorted(B.m), 1.0, None, None)))
        fields = []
        for k, o in enumerate(others):
            left = _sorted(o.matrix.m)
            fields.append(Field(left, left if self_join else _sorted(B_fields[k].m), weights[k + 1], None, None))
        self.union_calls.append((tuple(candidate_fields), int(sum(p.counts.sum() for p in parts)), int(u_counts.sum())))
        for st in states:
            st.stats["record_calls"] += 1
        for f in candidate_fields:
            states[f].stats["record_union_calls"] += 1
        out_c, out_v, out_n = ref_rescore(Case(u_cols, u_vals, u_counts, N, weights[0], fields, threshold, top_n))
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
