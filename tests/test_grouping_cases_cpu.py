"""The inputs of tests/test_grouping_paths_gpu.py are what they claim to be (numpy and the port alone)."""
import numpy as np
import pytest

from oracle import port as P
from tests import _grouping_cases as G

DTYPES = [np.float32, np.float64]


def _well_formed(A):
    assert (np.asarray(A.multiply(A).sum(axis=1)).ravel() <= 1.0).all()          # the index build groups such a matrix
    inside = np.ones(A.nnz, bool)                       # entries that are not the first of their row: columns ascend
    inside[A.indptr[:-1][np.diff(A.indptr) > 0]] = False
    assert (np.diff(A.indices.astype(np.int64))[inside[1:]] > 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sizes_has_every_size_class_of_the_member_sort_and_the_odd_groups(dtype):
    A = G.sizes(dtype)
    assert A.dtype == dtype and A.shape[0] == 25767
    _well_formed(A)
    assert np.asarray(A.multiply(A).sum(axis=1)).max() == 1.0
    gid, n_groups = G.expected_gid(A)
    members, size = G.expected_members(gid)
    assert n_groups == 311 and sorted(size[size > 1]) == sorted(G.SIZES + [2, 2, G.WIDE[0], G.N_EMPTY]) and (size == 1).sum() == 300
    assert (size > G.SORT_LDS).sum() == 2 and (size == G.SORT_LDS).sum() == 1 and (size == 33).sum() == 1 and (size == 32).sum() == 1
    # rows are not in arrival order: no group of several members is a run of consecutive rows
    first = np.concatenate([[0], np.cumsum(size)[:-1]])
    assert all(np.ptp(members[first[g]:first[g] + size[g]]) >= size[g] for g in np.flatnonzero(size > 1))
    lens = np.diff(A.indptr)
    assert (lens == G.WIDE[1]).sum() == G.WIDE[0] and (lens == 0).sum() == G.N_EMPTY
    # the near-copy of the first hub: same columns, one value one ulp lower
    starts = A.indptr[:-1][lens == 2]
    on_first = starts[A.indices[starts] == 0]
    assert len(on_first) == 4 and {A.data[s:s + 2].tobytes() for s in on_first} == {
        np.array([0.5, 0.5], dtype).tobytes(), np.array([0.5, np.nextafter(dtype(0.5), dtype(0))], dtype).tobytes()}


@pytest.mark.parametrize("dtype", DTYPES)
def test_sizes_has_rows_in_which_groups_of_several_members_tie_and_most_rows_are_full(dtype):
    A = G.sizes(dtype)
    gid, _ = G.expected_gid(A)
    size = np.bincount(gid)
    want = P.sp_matmul_topn_port(A, A.T, G.TOP_N, G.THRESHOLD, True, 8)
    found = np.diff(want.indptr)
    assert (found == G.TOP_N).sum() == 25450 >= 0.9 * A.shape[0]
    # result rows that hold more than one group (a handful: hubs on other columns score 0)
    g_of_entry = gid[want.indices]
    g_first = np.repeat(g_of_entry[np.minimum(want.indptr[:-1], want.nnz - 1)], found)
    mixed = np.unique(np.repeat(np.arange(A.shape[0]), found)[g_of_entry != g_first])
    assert 0 < len(mixed) < 20
    tied_rows = 0
    for r in mixed:
        cols, vals = want.indices[want.indptr[r]:want.indptr[r + 1]], want.data[want.indptr[r]:want.indptr[r + 1]]
        for v in np.unique(vals):
            groups = np.unique(gid[cols[vals == v]])
            if len(groups) > 1 and (size[groups] > 1).sum() > 1:
                tied_rows += 1
                break
    assert tied_rows >= 2          # (the two rows that are the first hub's first entry alone: 0.25 against three groups of 2)


@pytest.mark.parametrize("n_hubs", [G.LARGE_MAX, G.LARGE_MAX + 1])
def test_hubs_have_28_and_29_groups_above_the_lds_sort(n_hubs):
    A = G.hubs(n_hubs, np.float32)
    _well_formed(A)
    gid, n_groups = G.expected_gid(A)
    size = np.bincount(gid)
    assert (size > G.SORT_LDS).sum() == n_hubs and n_groups == n_hubs + 44
    if n_hubs == 29:
        assert A.shape[0] == 237649 and n_groups == 73
    A64 = G.hubs(n_hubs, np.float64)
    assert A64.dtype == np.float64 and np.array_equal(A64.data, A.data) and np.array_equal(A64.indices, A.indices)


def test_barely_sits_on_either_side_of_the_bar_and_not_on_it():
    for n_groups, alone, pairs in ((9701, 9402, 299), (9699, 9398, 301)):
        A = G.barely(n_groups, np.float32)
        _well_formed(A)
        gid, n = G.expected_gid(A)
        size = np.bincount(gid)
        assert A.shape[0] == 10000 and n == n_groups and (size == 1).sum() == alone and (size == 2).sum() == pairs
        assert n_groups != 0.97 * A.shape[0]
    assert 9699 < 0.97 * 10000 < 9701


def test_tiny():
    for which, want in (("two_same", [0, 0]), ("three_two_same", [0, 1, 0]), ("three_distinct", [0, 1, 2])):
        for dtype in DTYPES:
            A = G.tiny(which, dtype)
            _well_formed(A)
            assert list(G.expected_gid(A)[0]) == want
