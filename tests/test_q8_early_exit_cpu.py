"""The second filter's early exit (sg_spgemm_pruned.hip: q8_passes) and the rest norms K3 stores for it (sg_postings.hip:
q8_rest_word), restated in float32 in the kernel's order (tests/_q8_early_cases.py) on top of tests/test_prune_model.py's
q8_quantise / q8_bar / q8_bound.  Two claims:
  1  a pair the oracle keeps is rejected at NO boundary (with claim 2 this is implied by test_prune_model's "every match
     passes"; it is checked on its own because it is the one that would lose a match);
  2  a lane that leaves early would have failed the final test: early rejection implies q8_bound < q8_bar -- so the set that
     passes, the statistics and the results are what they were.
And that it bites: most pairs that are no match leave before their last unit."""
import numpy as np
import pytest

from oracle import oracle as O
from string_grouper_amd.synth import synth_names
from tests import _q8_early_cases as Q
from tests import _threshold_cases as T
from tests import test_prune_model as M

f32 = np.float32


def check_pair(a_idx, a_val, b_idx, b_val, thr, norm_up):
    """Claim 2 on one pair; -> (the unit the lane leaves behind or None, units of the record)."""
    bq = M.q8_quantise(b_val, norm_up)
    u, ub_then = Q.early_exit(a_idx, a_val, b_idx, bq, thr, norm_up)
    if u is not None:
        final = M.q8_bound(a_idx, a_val, b_idx, bq)
        assert final < M.q8_bar(thr, norm_up), (u, float(ub_then), float(final))
        assert ub_then <= final
    return u, (len(b_idx) + 7) >> 2 if len(b_idx) <= M.Q8_MAX_ENTRIES else 1


@pytest.mark.parametrize("n", [4, 8, 16, 17, 24, 60, 61])
def test_rest_norms_are_upper_bounds_rounded_up_in_integers(n):
    """Rows of exactly n entries (4: one unit, 8: two, 16 / 17: either side of a unit, 24: the last boundary's first entry,
    60: the longest record, 61: no copy): every field is the least integer at or above the root, 255 where that is 255 or more
    (a row of full-scale values) or the row has no copy, 0 where the record ends at the boundary."""
    rng = np.random.default_rng(n)
    for trial in range(50):
        bq = rng.integers(1, 256, n) if trial % 2 else np.clip(rng.integers(1, 40, n) * (1 + 5 * (trial % 3)), 1, 255)
        fields = Q.rest_fields(bq)
        for u, r in zip(Q.REST_UNITS, fields):
            s = int((bq[4 * u:].astype(np.int64) ** 2).sum())
            if n > M.Q8_MAX_ENTRIES or s > 254 * 254:
                assert r == Q.REST_UNKNOWN
            else:
                assert r * r >= s and (r == 0 or (r - 1) * (r - 1) < s), (u, r, s)
                assert (r == 0) == (n <= 4 * u)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("thr,scale", [pytest.param(0.5, None, id="0.5"), pytest.param(0.8, None, id="0.8"),
                                       pytest.param(0.95, None, id="0.95")] +
                         [pytest.param(t, sc, id=f"{t}-scale{sc}") for sc, t in M.OFF_NORM])
def test_early_exit_on_the_hub_list(dtype, thr, scale):
    """tests/test_prune_model.py's hub list of 4 000 names, on and off the unit norm: claim 1 on every match of the sampled
    rows, claim 2 on those and on twenty random columns per row.  Of the random pairs whose record has a unit behind a
    boundary to save (four units and more) more than half must leave early -- with nothing in common, equal values and
    ||a|| = ||b|| = norm_up a record of n entries leaves behind unit u as soon as (n - 4 u) / n < thr^2, which at 0.8 is the
    first boundary for n < 22 and the second for n < 33: nearly all of a name list; at 0.5 it takes (n - 4 u) / n < 0.25."""
    names = list(synth_names(4000, 321))
    for k in range(60):
        names[50 * k] = "NORTHERN LIGHTS HOLDING CO" + ("" if k % 3 else " " + "ABC"[k % 3])
    m, _ = M._scaled_names(None, scale, dtype, names=names)
    norm_up = M._norm_up(m)
    C = O.sp_matmul_topn(m, m.T.tocsr(), 100000, thr, sort=True)
    rng = np.random.default_rng(7)
    rows = np.unique(np.concatenate([rng.integers(0, m.shape[0], 300), np.arange(0, 3000, 50)]))
    kept = 0
    for i in rows:
        ai, av = Q.row(m, i)
        for j in C.indices[C.indptr[i]:C.indptr[i + 1]]:
            u, _ = check_pair(ai, av, *Q.row(m, j), dtype(thr), norm_up)
            assert u is None, (i, j, u)
            kept += 1
    assert kept > len(rows)
    could = left = 0
    for i in rows[:200]:
        ai, av = Q.row(m, i)
        for j in rng.integers(0, m.shape[0], 20):
            if j in C.indices[C.indptr[i]:C.indptr[i + 1]]:
                continue
            u, units = check_pair(ai, av, *Q.row(m, j), dtype(thr), norm_up)
            could += units >= 4
            left += u is not None
    print(f"thr {thr} scale {scale} {np.dtype(dtype).name}: {left} of {could} random non-matching pairs with four units and more "
          f"leave before their last unit ({100.0 * left / could:.1f} %)")
    assert left > 0.5 * could


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_early_exit_at_the_threshold_plus_and_minus_one_ulp(dtype):
    """tests/test_prune_model.py's tightest construction -- a near-copy of b on the shared terms, 8-bit-exact values every
    other trial, the threshold ONE ULP under the pair's exact score (a match: never rejected early) and one ulp above it
    (no match: whatever happens early must agree with the final test) -- with candidates of exactly 4, 8, 16, 17, 24, 60 and
    61 entries and left rows of the candidate's terms, of 64 and of 128 terms."""
    rng = np.random.default_rng(11)
    n_terms = 5000
    checked = 0
    for trial in range(420):
        n_b = (4, 8, 16, 17, 24, 60, 61)[trial % 7]
        n_a = int(rng.choice([n_b, 64, 128]))
        b_idx = np.sort(rng.choice(n_terms, n_b, replace=False))
        extra = np.setdiff1d(rng.choice(n_terms, n_a, replace=False), b_idx)[: max(n_a - n_b, 0)]
        a_idx = np.sort(np.concatenate([b_idx, extra]))
        norm_up = np.nextafter(f32(f32(1.0) * f32(1.000001)), f32(2))
        if (trial // 7) % 2:
            q = rng.integers(1, 40, n_b).astype(np.float64)
            b_val = q / np.sqrt((q * q).sum())
            b_val = np.maximum(np.round(b_val * 255 / float(norm_up)), 1.0) * float(norm_up) / 255.0
        else:
            b_val = rng.random(n_b) + 0.05
            b_val /= np.sqrt((b_val * b_val).sum())
        b_val = b_val.astype(dtype)
        a_val = np.zeros(len(a_idx))
        pos = np.searchsorted(a_idx, b_idx)
        a_val[pos] = b_val * (0.9 + 0.2 * rng.random(n_b))
        others = np.setdiff1d(np.arange(len(a_idx)), pos)
        a_val[others] = 0.02 * rng.random(len(others))
        a_val = (a_val / np.sqrt((a_val * a_val).sum())).astype(dtype)
        s = M.exact_score(a_idx, a_val, b_idx, b_val, dtype)
        if not 0.45 < float(s) < 1.0:
            continue
        u, _ = check_pair(a_idx, a_val, b_idx, b_val, np.nextafter(s, dtype(0)), norm_up)
        assert u is None, (trial, float(s), u)
        check_pair(a_idx, a_val, b_idx, b_val, np.nextafter(s, dtype(2)), norm_up)
        # ... and far above the score, where the lane does leave: the same implication
        check_pair(a_idx, a_val, b_idx, b_val, dtype(min(0.999, float(s) * 1.3)), norm_up)
        checked += 1
    assert checked > 300


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_switch_leaves_no_check_that_can_fire(dtype):
    """SG_Q8_EARLY=0 stores 255 in every field: the reader takes it for "unknown" whatever the rest of the test says -- also
    for a left row of norm 1/2, where  ub + ||a|| * 255  alone would be under the bar."""
    m, anchors = Q.built(dtype)
    norm_up = Q.norm_up_of(m)
    ai, av = Q.row(m, anchors[-1])                      # a row of norm 1/2
    for j in range(0, 400):
        bi, bv = Q.row(m, j)
        u, _ = Q.early_exit(ai, av, bi, M.q8_quantise(bv, norm_up), dtype(0.8), norm_up, fields=(Q.REST_UNKNOWN,) * 4)
        assert u is None


def test_built_matrix_holds_the_cases():
    """What tests/test_q8_early_exit_gpu.py runs is in the matrix: by the restated first filter, the candidates of one left
    row alone leave at each boundary and at none; the ordinary left rows' candidates have every number of entries from 1 to
    60 between them and include rows beyond 60 (no copy); the wide left rows (65 .. 128 terms) and those of norm 1/2 have
    candidates that leave early too (the latter at the lower threshold); claim 2 holds on every one of them."""
    m, anchors = Q.built(np.float32)
    nnz = np.diff(m.indptr)
    assert m.shape[0] > 2 * T.TILE_ROWS
    found = Q.built_candidates(np.float32, Q.THRESHOLDS[0])
    one = found[anchors[0]]
    assert {u for _, _, u in one} == {None, *Q.REST_UNITS}
    assert {n for i in anchors[:6] for _, n, _ in found[i]} >= set(range(1, 61)) and any(n > 60 for _, n, _ in one)
    wide = [i for i in anchors if nnz[i] > 64]
    assert len(wide) == 4 and all(65 <= nnz[i] <= 128 and {u for _, _, u in found[i]} >= set(Q.REST_UNITS) for i in wide)
    half = [i for i in anchors if abs(float(np.sqrt((Q.row(m, i)[1].astype(np.float64) ** 2).sum())) - 0.5) < 1e-3]
    low = Q.built_candidates(np.float32, Q.THRESHOLDS[1])
    assert len(half) == 2 and all(len({u for _, _, u in low[i]} - {None}) >= 2 for i in half)
    norm_up = Q.norm_up_of(m)
    for thr, table in zip(Q.THRESHOLDS, (found, low)):
        for i, cands in table.items():
            for j, _, u in cands:
                assert check_pair(*Q.row(m, i), *Q.row(m, j), f32(thr), norm_up)[0] == u
