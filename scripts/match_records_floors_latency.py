"""What a floor on ONE field costs through Corpus.match_records(field_min_similarity=...) (decided on the device:
the floors of sg_topn_rescore) against the composed route it replaces, and what the call WITHOUT the option costs on this build, in one
session.  The set-up is scripts/match_records_latency.py's: three SynthNames fields arranged by a seeded coin, fp32, candidates at
0.6 / top 50, final 0.8 / top 20, weights 0.5 / 0.3 / 0.2, force_symmetries=False on every route.

  plain      names.match_records([addresses, cities], ...) without the option: the kernels it always ran.  --plain-only stops
             here and runs on a checkout without the option too, so the same lines come from this build and from its parent.
  composed   names.match_strings at the candidate options, a pair_similarities call a further field, then numpy and pandas: the
             weighed sum, THE FLOOR MASK, the filter, the order, the cut, the frame of the survivors
  new        names.match_records([addresses, cities], field_min_similarity=[None, 0.6, None], ...): the same frame
  rescore    Context.topn_rescore on the SAME candidates (the names' self-join at the candidate options, kept on the device) with
             and without the floors, alternating: the call ends with its one read-back, so its wall time is the kernels' time
  columns    names.match_records(..., field_similarities=True): the frame with a column a field (sg_matchlist_field_scores on the
             list while it lies on the device) against the plain call plus one pair_similarities a field on its frame -- the
             same frame, the same bar

One round that only warms up, then --rounds rounds alternating.  bar: the new call's slowest run below the composed route's
fastest.  Every GPU step runs under a time limit of its own, one process a size (the machines are shared: nothing is started on a
card after a fault or a time limit).  As recorded in profiles/match_records_floors_latency.log:
  timeout -k 10 300 python scripts/match_records_floors_latency.py --records 663000
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- \
      python scripts/match_records_floors_latency.py --records 663000 --trace-run [--plain-only]  &&  python scripts/kstats.py <dir>/.../t_kernel_stats.csv 60
--trace-run: one warming call, then one call without and one with the floor, nothing else -- for a run of its own under a kernel
trace: both instantiations of rescore_score_kernel side by side, and (with --plain-only, on this build and on its parent) the
kernels of the unchanged path.
python scripts/match_records_floors_latency.py [--records 663000] [--rounds 3] [--floor 0.6] [--plain-only] [--trace-run]"""
import argparse
import json
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import string_grouper_amd as sga  # noqa: E402
import string_grouper_amd.engine as E  # noqa: E402
from match_records_latency import CAND, FINAL, W, arranged, timed  # noqa: E402
from string_grouper_amd import _native as N  # noqa: E402
from string_grouper_amd.synth import synth_names  # noqa: E402


def composed(names, others, floors):
    T = np.float32
    frame = names.match_strings(names.master, force_symmetries=False, **CAND)
    lp, rp = frame.left_index.to_numpy(), frame.right_index.to_numpy()        # (a RangeIndex: labels are positions)
    scores = [frame.similarity.to_numpy().astype(T)] + [o.pair_similarities(lp, rp) for o in others]
    acc = np.zeros(len(frame), T)
    for w, s in zip(W, scores):
        acc = acc + T(w) * s
    passed = acc > T(FINAL["min_similarity"])
    for s, m in zip(scores, floors):
        if m is not None:
            passed &= s > T(m)
    keep = np.flatnonzero(passed)
    order = keep[np.lexsort((rp[keep], -acc[keep], lp[keep]))]
    rank = np.arange(len(order)) - np.searchsorted(lp[order], lp[order], side="left")
    order = order[rank < FINAL["max_n_matches"]]
    order = order[np.lexsort((rp[order], lp[order]))]                         # a float32 list comes back with rows by column
    out = frame.iloc[order].reset_index(drop=True)
    out["similarity"] = acc[order].astype(np.float64)
    return out, len(frame)


def plain_plus_pairs(plain, corpora):
    """The route to per-field columns without the option: the plain call, then one pair_similarities a field on its frame."""
    frame = plain()
    lp, rp = frame.left_index.to_numpy(), frame.right_index.to_numpy()        # (a RangeIndex: labels are positions)
    at = list(frame.columns).index("similarity") + 1
    for k, c in enumerate(corpora):
        frame.insert(at + k, f"similarity_{k}", c.pair_similarities(lp, rp).astype(np.float64))
    return frame


def rescore_times(eng, ctx, corpora, floors, rounds):
    """topn_rescore on the same candidates, without and with the floors."""
    states = [c._live() for c in corpora]
    A = states[0].matrix
    plain_ms, floors_ms, kept = [], [], []
    with N.Scope() as s:
        cand = s.own(eng._topn_device(A, A, CAND["max_n_matches"], CAND["min_similarity"]))
        fields = []
        for st, w in zip(states[1:], W[1:]):
            rows = st.physical()
            fields.append((rows, rows, w, st.dead_dev, st.dead_dev))
        for rnd in range(-1, rounds):
            for into, fl in ((plain_ms, None), (floors_ms, floors)):
                res, ms = timed(lambda: ctx.topn_rescore(cand, W[0], fields, FINAL["min_similarity"], FINAL["max_n_matches"], floors=fl))
                if rnd >= 0:
                    into.append(ms)
                if rnd == 0:
                    kept.append(int(res.counts().sum()))
                res.free()
    return plain_ms, floors_ms, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="663000", help="one size a process, each under its own time limit (see above)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--floor", type=float, default=0.6, help="the floor on the address")
    ap.add_argument("--plain-only", action="store_true", help="only the call without the option (runs on the parent commit too)")
    ap.add_argument("--trace-run", action="store_true", help="one warming call, then one call without and one with the floor (for a kernel trace)")
    a = ap.parse_args()
    ctx = N.default_context(0)
    eng = E.HipEngine(ctx)
    E.set_engine(eng)
    rng = np.random.default_rng(7)
    floors = [None, a.floor, None]
    for n in [int(x) for x in a.records.split(",")]:
        kw = dict(tfidf_matrix_dtype=np.float32)
        names = sga.Corpus(pd.Series(synth_names(n, 1234)), **kw)
        frame = names.match_strings(names.master, force_symmetries=False, **CAND)
        off = frame[frame.left_index > frame.right_index]
        partner = np.full(n, -1, np.int64)
        first = off.groupby("left_index").right_index.min()
        partner[first.index.to_numpy()] = first.to_numpy()
        del frame, off, first
        addresses = sga.Corpus(arranged(pd.Series(synth_names(n, 1235, perturb_frac=0.0)), partner, rng), **kw)
        cities = sga.Corpus(arranged(pd.Series(synth_names(n, 1236, perturb_frac=0.0)), partner, rng), **kw)
        others = [addresses, cities]

        def plain():
            return names.match_records(others, weights=W, candidates=CAND, force_symmetries=False, **FINAL)

        def new():
            return names.match_records(others, weights=W, candidates=CAND, force_symmetries=False, field_min_similarity=floors, **FINAL)

        def columns():
            return names.match_records(others, weights=W, candidates=CAND, force_symmetries=False, field_similarities=True, **FINAL)

        if a.trace_run:
            plain()
            got, t_plain = timed(plain)
            kept, t_new = (got, 0.0) if a.plain_only else timed(new)
            print(json.dumps({"records": n, "trace_run": True, "plain_ms": round(t_plain, 1), "new_ms": round(t_new, 1),
                              "survivors_without_and_with": [len(got), len(kept)]}), flush=True)
            for c in (names, addresses, cities):
                c.close()
            continue
        plain_ms = []
        for rnd in range(-1, 2 * a.rounds if a.plain_only else a.rounds):
            got, t = timed(plain)
            if rnd >= 0:
                plain_ms.append(t)
        print(json.dumps({"records": n, "plain_ms": [round(x, 1) for x in plain_ms], "plain_median_ms": round(float(np.median(plain_ms)), 1),
                          "plain_survivors": len(got)}), flush=True)
        if not a.plain_only:
            new_ms, composed_ms, want, n_cand = [], [], None, 0
            for rnd in range(-1, a.rounds):                                   # round -1 warms both routes up at this size
                got, t_new = timed(new)
                (want, n_cand), t_old = timed(lambda: composed(names, others, floors))
                if rnd >= 0:
                    new_ms.append(t_new)
                    composed_ms.append(t_old)
                print(json.dumps({"records": n, "round": rnd, "new_ms": round(t_new, 1), "composed_ms": round(t_old, 1),
                                  "survivors": len(got)}), flush=True)
            try:
                pd.testing.assert_frame_equal(got, want)
                equal = True
            except AssertionError as e:
                equal = False
                print(json.dumps({"frames_differ": str(e)[:400]}), flush=True)
            r_plain, r_floors, kept = rescore_times(eng, ctx, [names] + others, floors, a.rounds)
            print(json.dumps({"summary": {
                "records": n, "floors": floors, "candidates": n_cand, "survivors": len(got), "frames_equal": equal,
                "new_ms": [round(x, 1) for x in new_ms], "composed_ms": [round(x, 1) for x in composed_ms],
                "bar_new_slowest_below_composed_fastest": bool(max(new_ms) < min(composed_ms)),
                "composed_fastest_over_new_slowest": round(min(composed_ms) / max(new_ms), 2),
                "rescore_ms_without_floors": [round(x, 2) for x in r_plain], "rescore_ms_with_floors": [round(x, 2) for x in r_floors],
                "rescore_kept_without_and_with": kept}}), flush=True)
            if not equal:
                raise SystemExit("match_records with floors does not reproduce the composed route's frame")
            # field columns: field_similarities=True against the plain call plus one pair_similarities a field
            col_ms, pairs_ms = [], []
            for rnd in range(-1, a.rounds):
                got, t_new = timed(columns)
                want, t_old = timed(lambda: plain_plus_pairs(plain, [names] + others))
                if rnd >= 0:
                    col_ms.append(t_new)
                    pairs_ms.append(t_old)
                print(json.dumps({"records": n, "round": rnd, "field_columns_ms": round(t_new, 1), "plain_plus_pairs_ms": round(t_old, 1),
                                  "rows": len(got)}), flush=True)
            try:
                pd.testing.assert_frame_equal(got, want)
                equal = True
            except AssertionError as e:
                equal = False
                print(json.dumps({"frames_differ": str(e)[:400]}), flush=True)
            print(json.dumps({"summary_field_columns": {
                "records": n, "rows": len(got), "frames_equal": equal, "field_columns_ms": [round(x, 1) for x in col_ms],
                "plain_plus_pairs_ms": [round(x, 1) for x in pairs_ms],
                "bar_new_slowest_below_composed_fastest": bool(max(col_ms) < min(pairs_ms)),
                "composed_fastest_over_new_slowest": round(min(pairs_ms) / max(col_ms), 2),
                "field_scores_ms_of_the_last_call": round(1e3 * eng.timings.get("field_scores_s", 0.0), 2)}}), flush=True)
            if not equal:
                raise SystemExit("field_similarities does not reproduce the plain call plus pair_similarities")
        for c in (names, addresses, cities):
            st = c.stats
            print(json.dumps({"records": n, "stats": {k: st.get(k) for k in ("tokenisations", "record_calls", "record_floor_calls", "pair_calls",
                                                                            "compactions", "index_builds")}}), flush=True)
            c.close()
        ctx.trim()


if __name__ == "__main__":
    main()
