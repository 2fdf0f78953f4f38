"""The constructed inputs of the self-join merge (tests/_merge_cases.py) bite, shown without a GPU:

  - every case holds the conditions under which the contract has one answer (``check_case``, run when a case is built) and
    says which path of pairs_select_kernel each of its rows takes; the census finds every path, every end of the rank path,
    every stride, every batch boundary in every order of arrival and every cut of the wide path, and names what is missing;
  - the register paths restated batch by batch (``ref_merge(..., batched=True)``) give the contract's answer on every case;
  - the contract is ``NumpyOps.selfjoin_merge`` of tests/_numpy_ops.py where that is defined (no repeats);
  - one multiset of records in three orders has one answer;
  - every wrong reference changes the answer of a case it is expected to, and the test says of which."""
import numpy as np
import pytest
import torch

from tests import _merge_cases as M
from tests._numpy_ops import HostTopN, NumpyOps, SelfJoinPart

DT = lambda d: np.dtype(d).name


def _rows(dtype, only=lambda name: True):
    for name in M.CASES:
        if only(name):
            cs = M.case(name, dtype)
            for r in cs.rows:
                yield cs, r


@pytest.mark.parametrize("dtype", M.DTYPES, ids=DT)
def test_the_census_finds_every_path_boundary_and_cut(dtype):
    missing = []
    rows = list(_rows(dtype))
    for name in M.CASES:
        cs = M.case(name, dtype)
        M.check_case(cs)
        assert cs.cols.shape[0] <= 300 or name.startswith("permuted"), name
        assert len(cs.pairs) <= 4000, f"{name}: {len(cs.pairs)} records"
    # the three paths, and every stride on the paths that can have it
    seen = {(r.path, cs.stride) for cs, r in rows}
    missing += [f"path {p} at stride {S}" for p, strides in (("rank", M.NARROW_STRIDES + M.WIDE_STRIDES), ("narrow", M.NARROW_STRIDES),
                                                              ("wide", M.WIDE_STRIDES)) for S in strides if (p, S) not in seen]
    # the end of the rank path: own + mirrored = 1, 63, 64, 65, 66 with none, one and a full stride of own entries
    seen = {(r.own + r.mirrored, "none" if r.own == 0 else "full" if r.own == cs.stride else "one" if r.own == 1 else "") for cs, r in rows
            if r.path != "outside"} | {(r.own + r.mirrored, "one") for cs, r in rows if r.own == 1 and r.path != "outside"}
    missing += [f"m = {m} with {own} own" for m in M.BOUNDARY_M for own in ("none", "one", "full") if (m, own) not in seen and not (m == 1 and own != "none")]
    assert {r.path for cs, r in rows if r.own + r.mirrored == 64 and r.path != "outside"} == {"rank"}
    assert {r.path for cs, r in rows if r.own + r.mirrored == 65 and r.path != "outside"} == {"narrow", "wide"}
    # batches of the register paths: every length, in every order of arrival, behind own entries
    seen = {(r.path, r.mirrored, r.arrival) for cs, r in rows if r.own > 0}
    missing += [f"{p}: {L} records arriving {a}" for p in ("narrow", "wide") for L in M.BATCH_LENGTHS for a in M.ARRIVALS if (p, L, a) not in seen]
    # the wide path: own lists of 0, 64, 65 and 128 at the cuts 65, 100 and 128
    seen = {(r.own, cs.stride) for cs, r in rows if r.path == "wide"}
    missing += [f"wide: {own} own at the cut {S}" for own in M.WIDE_OWN for S in M.WIDE_CUTS if own <= S and (own, S) not in seen]
    # membership: every step inside the rows, rows just outside the share named by records, every result size
    for step in M.STEPS:
        cs = M.case(f"membership-{step}", dtype)
        assert cs.step == step and cs.lo > 0 and cs.hi < cs.cols.shape[0]
        outside = {r.row for r in cs.rows if r.path == "outside"}
        assert {cs.lo - 1, cs.hi} <= outside and (step == 1) == (cs.hi - 2 not in outside), f"membership-{step}"
        assert {r.path for r in cs.rows} >= {"rank", "outside", "wide" if cs.stride > 64 else "narrow"}, f"membership-{step}"
    assert sorted(M.case(f"rows-{n}", dtype).cols.shape[0] for n in M.SIZES) == sorted(M.SIZES)
    assert all(len(M.case(f"rows-{n}", dtype).rows) == n for n in M.SIZES), "a row of a size case has no record"
    empty, none = M.case("nothing-empty-share", dtype), M.case("nothing-no-records", dtype)
    assert empty.lo == empty.hi and len(empty.pairs) > 0 and len(none.pairs) == 0 and none.hi > none.lo
    for cs in (empty, none):
        assert M.same(M.want(cs.name, dtype), (cs.cols, cs.vals, cs.counts)), f"{cs.name}: something changes"
    # positions: a real permutation, rows of the share and rows just outside it BY POSITION, all paths a stride can have
    for S in M.PERMUTED_STRIDES:
        cs = M.case(f"permuted-{S}", dtype)
        n = cs.cols.shape[0]
        assert n == M.PERMUTED_ROWS > 2 * 4096 and cs.step == 3 and not np.array_equal(cs.pos_of, np.arange(n))
        by_pos = {int(cs.pos_of[r.row]): r.path for r in cs.rows}
        assert all(by_pos[p] == "outside" for p in (cs.lo - 1, cs.hi, cs.hi - 2)) and by_pos[cs.hi - 1] != "outside" and by_pos[cs.lo] != "outside"
        assert {r.path for r in cs.rows} == {"rank", "outside", "wide" if S > 64 else "narrow"}
        assert any(M.is_member(r.row, cs.lo, cs.hi, cs.step) != (r.path != "outside") for r in cs.rows)
    assert not missing, f"{DT(dtype)}: no row for {missing}"
    print(f"{DT(dtype)}: {len(M.CASES)} cases, {len(rows)} rows named by records: "
          f"{ {p: sum(r.path == p for _, r in rows) for p in ('rank', 'narrow', 'wide', 'outside')} }")


@pytest.mark.parametrize("dtype", M.DTYPES, ids=DT)
def test_the_register_paths_restated_give_the_contracts_answer(dtype):
    """own entries first, records in batches of 64 held against the bar read before the batch, repeats refused by column,
    lists of 64 or 128: a bar that is only ever too low and a list that loses nothing that could stay change no answer"""
    for name in M.CASES:
        assert M.same(M.ref_case(M.case(name, dtype), batched=True), M.want(name, dtype)), f"{name}: the batches differ from the contract"


@pytest.mark.parametrize("dtype", M.DTYPES, ids=DT)
def test_the_contract_is_the_numpy_restatement_of_the_ranks(dtype):
    """NumpyOps.selfjoin_merge (what the multi-rank tests hold distributed.HipOps to) on the cases without repeats -- it
    does not define them -- in row order and over the library's permutation"""
    done = 0
    for name in M.CASES:
        cs = M.case(name, dtype)
        if name.startswith(("repeats", "nothing-no")):
            continue
        ops = NumpyOps(dtype)
        ops.permuted = cs.pos_of is not None
        part = SelfJoinPart(HostTopN(cs.cols.copy(), cs.vals.copy(), cs.counts.copy(), cs.n_cols),
                            torch.from_numpy(cs.pairs.reshape(-1).copy()), cs.words, None)
        block = ops.selfjoin_merge(part, part.pairs, cs.lo, cs.hi, cs.step)
        assert M.same(block.res.to_host(), M.want(name, dtype)), name
        done += 1
    assert done == len(M.CASES) - len(M.REPEAT_STRIDES) - 1


@pytest.mark.parametrize("dtype", M.DTYPES, ids=DT)
def test_one_multiset_of_records_has_one_answer(dtype):
    for S in M.ARRIVAL_STRIDES:
        cases = [M.case(f"arrival-{S}-{order}", dtype) for order in M.ORDERS]
        assert all(np.array_equal(np.sort(c.pairs.view(f"V{4 * c.words}").ravel()), np.sort(cases[0].pairs.view(f"V{4 * c.words}").ravel()))
                   for c in cases), "the three lists are not one multiset"
        assert not np.array_equal(cases[0].pairs, cases[1].pairs) and not np.array_equal(cases[0].pairs, cases[2].pairs)
        for c in cases[1:]:
            assert M.same(M.want(c.name, dtype), M.want(cases[0].name, dtype)), c.name


# the case each wrong reference must be caught by, at least
EXPECTED = {
    "bits-order": "ties-10",
    "arrival-ties": "ties-64",
    "repeats-counted": "repeats-10",
    "cut-at-stride-1": "boundaries-1",
    "wide-cut-at-64": "batches-65",
    "bar-drops-equal": "ties-100",
    "no-residue": "membership-3",
    "membership-on-j": "permuted-10",
    "outside-rewritten": "membership-1",
}


@pytest.mark.parametrize("dtype", M.DTYPES, ids=DT)
def test_every_wrong_reference_changes_an_answer(dtype):
    assert set(EXPECTED) == set(M.FLAWS)
    caught = {}
    for flaw in M.FLAWS:
        for name in M.CASES:
            if not M.same(M.ref_case(M.case(name, dtype), flaw), M.want(name, dtype)):
                caught.setdefault(flaw, []).append(name)
    for flaw, what in M.FLAWS.items():
        assert EXPECTED[flaw] in caught.get(flaw, []), f"'{flaw}' ({what}) is not noticed by {EXPECTED[flaw]}; noticed by {caught.get(flaw)}"
    # both zeros' signs come out: the row that holds them keeps a -0.0 and a +0.0
    for S in M.TIE_STRIDES:
        cs, (cols, vals, counts) = M.case(f"ties-{S}", dtype), M.want(f"ties-{S}", dtype)
        for r in cs.rows:
            if "0.0" in r.what:
                kept = vals[r.row, :counts[r.row]]
                zeros = kept[kept == 0]
                assert len(zeros) == min(3, S) and np.signbit(zeros).any() and not np.signbit(zeros).all(), f"ties-{S} row {r.row}"
    print({flaw: f"{len(c)} cases, first: {c[0]}" for flaw, c in caught.items()})
