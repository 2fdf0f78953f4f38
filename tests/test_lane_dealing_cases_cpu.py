"""CPU test: the matrices of tests/_lane_dealing_cases.py are what tests/test_lane_dealing_gpu.py takes them for -- list
lengths on the right side of the bar from which a term is frequent, rows of exactly the widths the dealing's corners need,
a list that lies in both super-tiles, wide rows whose prefix terms sit in both halves, unit norms, and planted
near-duplicates that the port finds above the threshold with no list cut."""
import numpy as np

from tests import _lane_dealing_cases as L


def test_the_cases_are_what_they_claim():
    for dtype in L.DTYPES:
        A = L.rare(dtype)
        df, nnz = L.list_lengths(A), np.diff(A.indptr)
        assert A.shape[0] == 4000 and L.frequent_from(A) == 20 and df.max() == 19
        assert {1, 2, 63, 64} <= set(nnz.tolist()) and nnz.max() == 64
        A = L.skewed(dtype)
        df, nnz = L.list_lengths(A), np.diff(A.indptr)
        assert A.shape[0] == 40000 > 32768 and L.frequent_from(A) == 200 and df.max() == 199
        per_row = [np.sort(df[A.indices[A.indptr[i]:A.indptr[i + 1]]]).tolist() for i in range(0, 40000, 7)]
        assert [2] * 10 + [199] in per_row and [12] * 9 in per_row
        long_lists = np.flatnonzero(df == 199)
        rows_of = A.tocsc()
        first = rows_of.indices[rows_of.indptr[long_lists[0]]:rows_of.indptr[long_lists[0] + 1]]
        assert first.min() < 32768 <= first.max()            # the list lies in both super-tiles
        A = L.wide(dtype)
        df, nnz = L.list_lengths(A), np.diff(A.indptr)
        assert A.shape[0] == 4000 and L.frequent_from(A) == 20
        wide_rows = np.flatnonzero(nnz > 64)
        assert len(wide_rows) == 600 and nnz.max() == 128 and nnz[wide_rows].min() == 65
        seen = set()
        for i in wide_rows:
            d = df[A.indices[A.indptr[i]:A.indptr[i + 1]]]
            v = A.data[A.indptr[i]:A.indptr[i + 1]].astype(np.float64)
            rare_terms = d < 20
            assert 60 <= rare_terms.sum() <= 64 and (v[~rare_terms] ** 2).sum() < 0.4      # the frequent part fits the suffix
            assert rare_terms[:64].any() and rare_terms[64:].any()                         # prefix terms in both halves
            seen.add(int(rare_terms.sum()))
        assert seen == {60, 61, 62, 63, 64}
        for case in L.CASES:
            A = L.matrix(case, dtype)
            n2 = np.asarray(A.astype(np.float64).multiply(A.astype(np.float64)).sum(axis=1)).ravel()
            assert np.abs(n2 - 1.0).max() < 1e-6
            C = L.port(case, dtype)
            assert (np.diff(C.indptr) >= 2).mean() > 0.9 and np.diff(C.indptr).max() < L.TOP_N      # near-duplicates found, nothing cut
