"""What the second filter of the pruned multiply saves when a lane stops reading a candidate's 8-bit record as soon as the
rest of the record cannot lift the bound over the bar (sg_spgemm_pruned.hip: q8_passes; the rest norms: sg_postings.hip).
CPU model in the manner of k4p_second_filter_model.py: the first filter's candidates from tests/test_prune_model.py's
restatement (self-join form, every row indexed), the second filter's arithmetic in float64.  A call of the survivor routine
is up to 64 candidates of one row; its lanes run in lockstep, so a call costs the MAXIMUM of its lanes' iterations.
Printed per variant: 16-byte units read per candidate (header included, and the unit a lane has requested before its check)
and entry-unit iterations per call.  Variants: now; the weak bound (A_rest = ||a||) and the full one (A_rest = sqrt(||a||^2 -
sum of the matched a_k^2)) for every set of boundaries given; a check behind every unit (the bound of the idea).
python scripts/k4p_q8_early_exit_model.py [names=20000] [rows=1500] [boundaries=1,2,3,4 ...]"""
import math
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import test_prune_model as T  # noqa: E402
from oracle import oracle as O  # noqa: E402
from string_grouper_amd.synth import synth_names  # noqa: E402

f32 = np.float32
n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
n_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 1500
sets = [tuple(int(x) for x in s.split(",")) for s in sys.argv[3:]] or [(1, 2, 3, 4), (2, 3, 4, 6)]
every = max(1, n // n_rows)
names = synth_names(n, 1234)
(m,), _, _ = O.tfidf_sklearn(names, [names], dtype=np.float32)
m = m.tocsr()
m.sort_indices()
mt = m.T.tocsr()
mt.sort_indices()
norm_up = np.nextafter(f32(np.sqrt(f32(np.asarray(m.multiply(m).sum(axis=1)).max())) * f32(1.000001)), f32(2))
thr, delta, freq = 0.8, 0.03, 0.005
freq_min = max(1, int(freq * n))
fq, bq, post = T.quantise_right_stream(m, mt, freq_min, norm_up, tile=4096)
bar = float(T.q8_bar(f32(thr), norm_up))
bar_lo = bar * (1.0 - 2e-5)
rng = np.random.default_rng(5)
t0 = time.time()
md = m.data.astype(np.float64)
q8 = T.q8_quantise(m.data, norm_up)            # every row's 8-bit values, as K3 writes them

EVERY = tuple(range(1, 16))
variants = [("now", None, None)] + [(f"{kind} {','.join(map(str, s))}", kind, s) for s in sets for kind in ("weak", "full")] + \
           [("full, every unit", "full", EVERY)]
units_read = {v[0]: 0 for v in variants}
call_iters = {v[0]: 0 for v in variants}
candidates = calls = rows = passed = 0


def lane(a, na2, j, kind, bounds):
    """(units read, entry-unit iterations, passes) of one candidate."""
    lo, hi = m.indptr[j], m.indptr[j + 1]
    cnt = hi - lo
    if cnt > T.Q8_MAX_ENTRIES:
        return 1, 0, True
    units = (cnt + 7) >> 2
    ks, qs = m.indices[lo:hi].tolist(), q8[lo:hi].tolist()
    ub = matched = 0.0
    for u in range(1, units):
        for e in range(4 * u - 4, min(4 * u, cnt)):
            av = a.get(ks[e], 0.0)
            ub += av * qs[e]
            matched += av * av
        if bounds is not None and u in bounds and u + 1 < units:
            r = math.isqrt(sum(q * q for q in qs[4 * u:]) - 1) + 1 if qs[4 * u:] else 0      # the root rounded UP, as stored
            a_rest = math.sqrt(max(na2 * (1 + 2e-5) - (matched if kind == "full" else 0.0), 0.0))
            if r < 255 and ub + a_rest * r < bar_lo:
                return min(u + 2, units), u, False
    return units, units - 1, ub >= bar


for i in range(0, n, every):
    lo, hi = m.indptr[i], m.indptr[i + 1]
    rec, _ = T.records_of_row_stream(m.indices[lo:hi], m.data[lo:hi], mt.indptr, mt.indices, bq, fq, post, thr, delta,
                                     norm_up, freq_min, rng, tile=4096)
    if rec is None:
        continue
    rows += 1
    uni = np.unique(rec[rec <= i])             # self-join form: the pairs j <= i are row i's
    a = dict(zip(m.indices[lo:hi].tolist(), md[lo:hi].tolist()))
    na2 = float((md[lo:hi] ** 2).sum())
    candidates += len(uni)
    calls += (len(uni) + 63) // 64
    for name, kind, bounds in variants:
        per = [lane(a, na2, int(j), kind, bounds) for j in uni]
        units_read[name] += sum(p[0] for p in per)
        for c in range(0, len(per), 64):
            call_iters[name] += max(p[1] for p in per[c:c + 64])
        if kind is None:
            passed += sum(p[2] for p in per)
        else:
            assert sum(p[2] for p in per) == sum(lane(a, na2, int(j), None, None)[2] for j in uni)      # the pass set is the same

print(f"{rows} rows of {n} names (threshold {thr}): {candidates} candidates in {calls} calls "
      f"({candidates / max(calls, 1):.1f} lanes a call), {passed} pass   [{time.time() - t0:.0f} s]")
base = call_iters["now"]
for name, _, _ in variants:
    print(f"  {name:24s} units read per candidate {units_read[name] / max(candidates, 1):5.2f}   "
          f"iterations per call {call_iters[name] / max(calls, 1):5.2f} ({100.0 * (call_iters[name] - base) / max(base, 1):+.0f} %)")
