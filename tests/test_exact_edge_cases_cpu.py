"""The constructed inputs of the exact multiply (tests/_exact_edge_cases.py) bite, shown without a GPU: for every
(family, dtype, tile size, permutation on / off)

  - the census -- a plain count of segment lengths, segments per chunk, ballot masks, hit positions, counts between launches,
    tie blocks -- finds every edge the family owns at that tile size (``expected``), and names what is missing otherwise;
  - the multiply restated in numpy equals the oracle's port bit for bit on the whole schedule: indptr, indices, data;
  - every wrong reference of the family (``flaws_of``) changes the answer of at least one multiply of the schedule -- the
    test says which --, and equal scores ordered by POSITION change nothing while the index is in row order;
  - the rows built for it differ in bits between ascending and descending summation in float32 and in float64.

Nothing is skipped or waived at run time: an edge a tile size cannot hold is absent from ``expected`` / ``flaws_of`` for that
tile size, with the reason next to it."""
import numpy as np
import pytest

from tests import _exact_edge_cases as E

CASES = [(f, d, t, p) for f in E.FAMILIES for d in E.DTYPES for t in E.TILES for p in (False, True)]
CASES += [("selfjoin", d, t, p) for d in E.DTYPES for t in E.SELF_TILES for p in (False, True)]
IDS = [f"{f}-{np.dtype(d).name}-{t}-{'permuted' if p else 'row-order'}" for f, d, t, p in CASES]


@pytest.mark.parametrize("family,dtype,tile_cols,permute", CASES, ids=IDS)
def test_the_census_finds_every_edge(family, dtype, tile_cols, permute):
    case = E.build(family, dtype, tile_cols, permute)
    assert case.n == 2 * tile_cols + 104 and case.B.shape == (case.n, case.n_terms) and case.A.shape[1] == case.n_terms
    if permute:      # the caller's matrix is the design permuted by the library's rule
        assert sorted(case.pos_of.tolist()) == list(range(case.n)) and case.pos_of[1] != 1
        assert np.array_equal(case.orig_of[case.pos_of], np.arange(case.n))
    found = E.census(case)
    miss = E.missing(found, E.expected(family, dtype, tile_cols, permute), permute)
    assert not miss, f"{family}: the inputs do not reach: {miss}"
    # the products the kernel will make: the sum of the list lengths over the left entries, counted a second way
    lengths = np.diff(case.lists.ptr)
    if family == "selfjoin":      # (A is B: the sum of the squared list lengths, and every row is cosine-like)
        assert found["macs"] == int(lengths[case.A.indices].sum()) and case.A is case.B
        return
    assert found["macs"] == int(lengths[case.A.indices].sum()) == int((abs(case.A).sign() @ abs(case.B.T).sign()).sum())


@pytest.mark.parametrize("family,dtype,tile_cols,permute", CASES, ids=IDS)
def test_the_reference_is_the_port_and_every_wrong_reference_is_caught(family, dtype, tile_cols, permute):
    case = E.build(family, dtype, tile_cols, permute)
    kw = dict(tile_cols=tile_cols, pos_of=case.pos_of, lists=case.lists, cache={})
    left, names = case.A, case.row_names
    if family == "selfjoin":      # the numpy reference on the club and hub members and a few other rows; the port on the same
        from oracle import port as P
        left, names = case.B[case.probe], [case.row_names[j] for j in case.probe]
        kw["left_pos"] = (case.pos_of if permute else np.arange(case.n))[case.probe]
    right = {}
    for top_n, thr, sort in case.schedule:
        right[(top_n, thr, sort)] = E.reference(left, case.B, top_n, thr, sort, dtype, **kw)
        want = E.port(case, top_n, thr, sort) if family != "selfjoin" else P.sp_matmul_topn_port(left, case.B.T, top_n, thr, sort, 4)
        assert E.same(right[(top_n, thr, sort)], want), f"the reference is not the port at top_n={top_n} thr={thr} sort={sort}"
    if family == "state":      # the list carried through the launches as the kernel carries it gives the same rows
        for group in (1, 2):
            for i in range(case.A.shape[0]):
                cols, vals = case.A.indices[case.A.indptr[i]:case.A.indptr[i + 1]], case.A.data[case.A.indptr[i]:case.A.indptr[i + 1]]
                acc, touched = E.accumulate(cols, vals, case.lists, dtype)
                for top_n in (64, 65, 129, case.n):
                    a, b = E.select(acc, touched, case.lists, top_n, 0.0), E.select(acc, touched, case.lists, top_n, 0.0, None, group, [])
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    caught = {}
    for flaw in E.flaws_of(family, dtype, tile_cols):
        group = 1 if E.FLAWS[flaw][0] == "state" else 0          # (a launch a tile: the state flaws need launches to show)
        for key, good in right.items():
            bad = E.reference(left, case.B, *key, dtype, flaw, group=group, **kw)
            if not E.same(bad, good):
                rows = np.flatnonzero([not E.same(bad[i], good[i]) for i in range(good.shape[0])])
                caught[flaw] = (key, names[rows[0]])
                break
        if flaw == "ties-by-position" and not permute:
            assert flaw not in caught, f"position order changed the answer of an index in row order: {caught[flaw]}"
        else:
            assert flaw in caught, f"{family}: no multiply of the schedule notices: {E.FLAWS[flaw][1]}"
    print({f: f"top_n={k[0]} thr={k[1]} sort={k[2]}: {row}" for f, (k, row) in caught.items()})


@pytest.mark.parametrize("dtype", E.DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_order_of_the_sum_shows_in_the_bits(dtype):
    case = E.build("batches", dtype, 1024, True)
    rows = case.edges["order of the sum"]
    assert len(rows) == 4 and any(np.any(np.diff(case.A.indices[case.A.indptr[i]:case.A.indptr[i + 1]]) < 0) for i in rows), \
        "no left row is stored in descending column order"
    for i in rows:
        cols, vals = case.A.indices[case.A.indptr[i]:case.A.indptr[i + 1]], case.A.data[case.A.indptr[i]:case.A.indptr[i + 1]]
        up, _ = E.accumulate(cols, vals, case.lists, dtype)
        down, _ = E.accumulate(cols, vals, case.lists, dtype, "descending-sum")
        assert np.allclose(up, down, rtol=1e-4) and not np.array_equal(up, down), case.row_names[i]
