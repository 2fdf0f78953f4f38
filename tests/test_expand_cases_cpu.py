"""The constructed inputs of the expansion of grouped results (tests/_expand_cases.py) bite, shown without a GPU:

  - the census -- the kernels' queueing rule restated, run lengths, where every cut falls, queued rows per call -- finds every
    edge a stride can hold, at every stride, and names what is missing otherwise;
  - the model of the two kernels (``expand_row``) without a wrong turn is the statement (``ref_expand``), and the statement
    is ``NumpyOps.expand_rows`` of tests/_numpy_ops.py on one group of every kind;
  - ``ref_expand`` of the port's result over the REPRESENTATIVES equals the port on ALL rows: every one-sided case at top_n
    1, 2, 10, 64, 65 and 128, the repeated left rows, and the self-product of the layout whose groups score against each other;
  - every wrong reference changes an answer, and the test says on which case -- but for the one turn that provably cannot
    (``HARMLESS``, with the reason next to it), which must change none."""
import numpy as np
import pytest

from oracle import port as P
from tests import _expand_cases as X
from tests._numpy_ops import NumpyOps

DT = lambda d: np.dtype(d).name


@pytest.mark.parametrize("S", X.STRIDES)
@pytest.mark.parametrize("dtype", X.DTYPES, ids=DT)
def test_the_census_finds_every_edge(dtype, S):
    L = X.layout(dtype)
    assert L.n == 4025 and L.n_groups == 2169 > 2 * X.TILE and int(L.size[L.size > 1].sum()) >= 2200
    assert sorted(int(z) for z in L.size[L.size > 3]) == sorted(s for _, s in X.SPECIAL)
    g = lambda name: int(L.group_of_type[L.t[name]])
    assert list(L.rows_of(g("first"))) == list(range(10)) and list(L.rows_of(g("last"))) == list(range(L.n - 11, L.n))
    assert list(L.rows_of(g("alt_a"))) == list(range(10, 22, 2)) and list(L.rows_of(g("alt_b"))) == list(range(11, 22, 2))
    spread = L.rows_of(g("h1000"))
    assert len(np.unique(L.gid[spread[0]:spread[-1]])) > 2000, "the hub's members do not interleave with the other groups'"
    cs = X.case(dtype, S)
    assert cs.cols.shape == (L.n_groups, S) and cs.counts.max() == (S if S > 1 else 1)
    for c, v in cs.rows:       # as the multiply leaves a row: score descending, then group ascending
        assert all(v[e] > v[e + 1] or (v[e] == v[e + 1] and c[e] < c[e + 1]) for e in range(len(c) - 1))
    found = X.census(cs)
    print(f"stride {S}: {len(cs.kinds)} kinds, runs of {found['run_lengths']}, queued rows per call {found['queued_rows']}, "
          f"kept {found['kept_rows']}")


@pytest.mark.parametrize("S", X.STRIDES)
@pytest.mark.parametrize("dtype", X.DTYPES, ids=DT)
def test_the_model_without_a_wrong_turn_is_the_statement(dtype, S):
    cs = X.case(dtype, S)
    L = cs.L
    want = X.ref_expand(L, None, cs.cols, cs.vals, cs.counts, S)
    assert want[0].shape == (L.n, S)
    assert X.same(X.wrong_expand(L, None, cs.cols, cs.vals, cs.counts, S, None), want), f"stride {S}: expand_row is not ref_expand"
    for which, rows in cs.row_lists.items():
        if rows is not None:
            part = X.ref_expand(L, rows, cs.cols, cs.vals, cs.counts, S)
            assert X.same(part, tuple(a[rows] for a in want)), f"stride {S}, rows {which}"

    class Index:
        gid, members = L.gid, [list(L.rows_of(g)) for g in range(L.n_groups)]

    rows = np.array([L.rows_of(np.flatnonzero(cs.kind_of_group == k)[0])[-1] for k in range(len(cs.kinds))])
    assert X.same(NumpyOps.expand_rows(Index, rows, cs.cols, cs.vals, cs.counts), tuple(a[rows] for a in want)), \
        f"stride {S}: ref_expand is not NumpyOps.expand_rows"


def _port_fixed(A, B, top_n, thr, stride):
    return X.fixed(P.sp_matmul_topn_port(A, B.T, top_n, thr, True, 4), stride)


@pytest.mark.parametrize("top_n", X.TOP_NS)
@pytest.mark.parametrize("dtype", X.DTYPES, ids=DT)
def test_the_statement_on_the_representatives_is_the_port_on_all_rows(dtype, top_n):
    L = X.layout(dtype)
    A, names = X.left_matrix(dtype)
    assert len(names) > 100
    for left, what in ((A, names), X.repeated(A, names)):
        groups = _port_fixed(left, L.U, top_n, X.THRESHOLD, min(top_n, L.n_groups))
        got = X.ref_expand(L, None, *groups, min(top_n, L.n), left=True)
        want = _port_fixed(left, L.A, top_n, X.THRESHOLD, min(top_n, L.n))
        bad = [what[i] for i in range(len(what)) if not X.same(tuple(a[i:i + 1] for a in got), tuple(a[i:i + 1] for a in want))]
        assert not bad, f"top_n {top_n}: the statement is not the port on {bad[:5]}"
        assert want[2].max() == min(top_n, L.n) and (top_n == 1 or (want[2] < top_n).any())   # rows that are cut, rows that are not
    V = X.variant(dtype)
    assert V.n_groups == 70 < V.n and V.size.max() == 4
    groups = _port_fixed(V.U, V.U, top_n, X.VARIANT_THRESHOLD, min(top_n, V.n_groups))
    assert groups[2].max() == min(top_n, 70)
    got = X.ref_expand(V, None, *groups, min(top_n, V.n))
    assert X.same(got, _port_fixed(V.A, V.A, top_n, X.VARIANT_THRESHOLD, min(top_n, V.n))), f"top_n {top_n}: the variant's self-product"


@pytest.mark.parametrize("dtype", X.DTYPES, ids=DT)
def test_every_wrong_reference_changes_an_answer(dtype):
    caught = {}
    for flaw in X.FLAWS:
        if flaw in ("stride-cut-at-groups", "range-from-lo"):
            continue
        for S in X.STRIDES:
            cs = X.case(dtype, S)
            for name, (c, v) in zip(cs.names, cs.rows):
                good, bad = X.expand_row(cs.L, c, v, S), X.expand_row(cs.L, c, v, S, flaw)
                if len(good[0]) != len(bad[0]) or not np.array_equal(good[0], bad[0]) or good[1].tobytes() != bad[1].tobytes():
                    caught.setdefault(flaw, []).append(f"{name} at stride {S}")
    # the stride cut at the number of groups: where there are fewer groups than top_n asks columns for
    V = X.variant(dtype)
    for top_n in X.TOP_NS:
        groups = _port_fixed(V.U, V.U, top_n, X.VARIANT_THRESHOLD, min(top_n, V.n_groups))
        good = X.ref_expand(V, None, *groups, min(top_n, V.n))
        assert X.same(X.wrong_expand(V, None, *groups, min(top_n, V.n), None), good)
        if not X.same(X.wrong_expand(V, None, *groups, min(top_n, V.n), "stride-cut-at-groups"), good):
            caught.setdefault("stride-cut-at-groups", []).append(f"the variant's self-product at top_n {top_n}")
    # a share's positions counted from the wrong end: the rows of rank r of `world` over the permuted and the row-order index
    L = X.layout(dtype)
    for pos_of, how in ((NumpyOps.permutation(L.n_groups)[1], "permuted"), (None, "row order")):
        for world in (2, 3, 8):
            shares = [X.range_rows(L, pos_of, 0, L.n_groups - r, world) for r in range(world)]
            assert np.array_equal(np.sort(np.concatenate(shares)), np.arange(L.n)), "the shares of one world are disjoint and cover every row"
            for r in range(world):
                if not np.array_equal(X.range_rows(L, pos_of, 0, L.n_groups - r, world, from_lo=True), shares[r]):
                    caught.setdefault("range-from-lo", []).append(f"rank {r} of {world}, {how}")
    for flaw, what in X.FLAWS.items():
        if flaw in X.HARMLESS:
            assert flaw not in caught, f"'{what}' cannot change an answer on sorted rows (tests/_expand_cases.py), yet did: {caught[flaw][:3]}"
        else:
            assert flaw in caught, f"no case notices the wrong turn '{flaw}': {what}"
    print({flaw: f"{len(c)} cases, first: {c[0]}" for flaw, c in caught.items()})
