"""What matching RECORDS of three fields costs through Corpus.match_records (candidates rescored on the device: sg_topn_rescore)
against the composed route it replaces, in one session:

  composed   names.match_strings at the candidate options (the frame of EVERY candidate comes down), then
             addresses.pair_similarities and cities.pair_similarities over its positions (two position lists up and the scores
             down, a field), then numpy and pandas: the weighed sum in float32, the filter, the order by record, combined
             similarity descending and right position, the cut, the frame of the survivors
  new        names.match_records([addresses, cities], ...): the same frame, only the survivors come down

Records: SynthNames lists of three seeds, fp32; the second and third field are arranged so that name candidates agree on them --
a seeded coin a record decides whether it takes the field of the first record its name is a candidate of (with a number behind
it) or keeps its own; the share of the candidates that ends up above 0.6 on a further field is printed (0.27-0.29 in the
recorded runs).  Candidates at 0.6 / top 50, final 0.8 / top 20, force_symmetries=False on both routes (the
frames are then comparable row by row).  One round that only warms up, then --rounds rounds alternating between the two.

  new_ms, composed_ms (and its split: match_strings, the pair calls, the host tail) per round
  candidates, survivors; frames_equal (assert_frame_equal of the last round's two frames)
  bar        the new call's slowest run below the composed route's fastest
  gathered_bytes_per_candidate  what the scoring kernel has to read for a candidate and field, from the rows' lengths: 2 x 16 B
             of row pointers and (4 + 4) B an entry of either row; plus 4 + 4 B of column and score once and 2 x 4 B of c a field

--trace-run: one new call and one addresses.pair_similarities over the same candidates, nothing else -- for a run of its own
under rocprofv3 --kernel-trace --stats (scripts/kstats.py prints the kernels' times): rescore_score_kernel and
rescore_select_short_kernel beside pairs_dot_kernel.
Every GPU step runs under a time limit of its own, one process a size, and a step that fails ends the session (the machines are
shared: nothing is started on a card after a fault or a time limit).  As recorded in profiles/match_records_latency.log:
  timeout -k 10 200 python scripts/match_records_latency.py --records 663000
  timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- \
      python scripts/match_records_latency.py --records 663000 --trace-run        &&  python scripts/kstats.py <dir>/.../t_kernel_stats.csv 40
  timeout -k 10 660 python scripts/match_records_latency.py --records 5000000
python scripts/match_records_latency.py [--records 663000] [--rounds 3] [--trace-run]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import string_grouper_amd as sga  # noqa: E402
import string_grouper_amd.engine as E  # noqa: E402
from string_grouper_amd import _native as N  # noqa: E402
from string_grouper_amd.synth import synth_names  # noqa: E402

W = [0.5, 0.3, 0.2]
CAND = dict(min_similarity=0.6, max_n_matches=50)
FINAL = dict(min_similarity=0.8, max_n_matches=20)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def arranged(base: pd.Series, partner: np.ndarray, rng) -> pd.Series:
    """A record with a partner takes the partner's value (a number behind it) when its coin says so."""
    take = np.flatnonzero((partner >= 0) & (rng.random(len(base)) < 0.5))
    out = base.copy()
    out.iloc[take] = (base.iloc[partner[take]].to_numpy() + " " + pd.Series(1 + take % 9).astype(str)).to_numpy()
    return out


def composed(names, others, split):
    T = np.float32
    frame, t0 = timed(lambda: names.match_strings(names.master, force_symmetries=False, **CAND))
    lp, rp = frame.left_index.to_numpy(), frame.right_index.to_numpy()        # (a RangeIndex: labels are positions)
    scores, t1 = timed(lambda: [frame.similarity.to_numpy().astype(T)] + [o.pair_similarities(lp, rp) for o in others])

    def tail():
        acc = np.zeros(len(frame), T)
        for w, s in zip(W, scores):
            acc = acc + T(w) * s
        keep = np.flatnonzero(acc > T(FINAL["min_similarity"]))
        order = keep[np.lexsort((rp[keep], -acc[keep], lp[keep]))]
        rank = np.arange(len(order)) - np.searchsorted(lp[order], lp[order], side="left")
        order = order[rank < FINAL["max_n_matches"]]
        order = order[np.lexsort((rp[order], lp[order]))]                     # a float32 list comes back with rows by column
        out = frame.iloc[order].reset_index(drop=True)
        out["similarity"] = acc[order].astype(np.float64)
        return out
    out, t2 = timed(tail)
    split.update(match_strings_ms=round(t0, 1), pair_calls_ms=round(t1, 1), host_tail_ms=round(t2, 1), candidates=len(frame))
    return out, lp, rp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="663000", help="one size a process, each under its own time limit (see above)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-run", action="store_true", help="one new call and one pair call over the same candidates (for a kernel trace)")
    a = ap.parse_args()
    ctx = N.default_context(0)
    E.set_engine(E.HipEngine(ctx))
    rng = np.random.default_rng(7)
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

        def new():
            return names.match_records(others, weights=W, candidates=CAND, force_symmetries=False, **FINAL)

        if a.trace_run:
            split = {}
            _, lp, rp = composed(names, others, split)                        # (also warms the index up)
            got, t_new = timed(new)
            _, t_pairs = timed(lambda: addresses.pair_similarities(lp, rp))
            print(json.dumps({"records": n, "trace_run": True, "candidates": len(lp), "survivors": len(got), "new_ms": round(t_new, 1),
                              "one_field_pair_call_ms": round(t_pairs, 1)}), flush=True)
        else:
            new_ms, composed_ms, got, want, split = [], [], None, None, {}
            for rnd in range(-1, a.rounds):                                   # round -1 warms both routes up at this size
                got, t_new = timed(new)
                split = {}
                (want, lp, rp), t_old = timed(lambda: composed(names, others, split))
                if rnd >= 0:
                    new_ms.append(t_new)
                    composed_ms.append(t_old)
                print(json.dumps({"records": n, "round": rnd, "new_ms": round(t_new, 1), "composed_ms": round(t_old, 1), **split,
                                  "survivors": len(got)}), flush=True)
            try:
                pd.testing.assert_frame_equal(got, want)
                equal = True
            except AssertionError as e:
                equal = False
                print(json.dumps({"frames_differ": str(e)[:400]}), flush=True)
            per_field = []
            for o in others:
                lengths = np.diff(o._state.physical().to_scipy().indptr)
                per_field.append(round(float((lengths[lp].sum() + lengths[rp].sum()) * 8 / len(lp) + 2 * 16 + 2 * 4), 1))
            agree = [float(np.mean(o.pair_similarities(lp[:200000], rp[:200000]) > 0.6)) for o in others]
            print(json.dumps({"summary": {
                "records": n, "candidates": len(lp), "survivors": len(got), "frames_equal": equal,
                "new_ms": [round(x, 1) for x in new_ms], "composed_ms": [round(x, 1) for x in composed_ms],
                "bar_new_slowest_below_composed_fastest": bool(max(new_ms) < min(composed_ms)),
                "composed_fastest_over_new_slowest": round(min(composed_ms) / max(new_ms), 2),
                "gathered_bytes_per_candidate_by_field": per_field, "plus_bytes_per_candidate_once": 8,
                "share_of_the_first_200k_candidates_above_0.6_by_field": [round(x, 3) for x in agree]}}), flush=True)
            if not equal:
                raise SystemExit("match_records does not reproduce the composed route's frame")
        for c in (names, addresses, cities):
            st = c.stats
            print(json.dumps({"records": n, "stats": {k: st[k] for k in ("tokenisations", "record_calls", "pair_calls", "compactions", "index_builds")}}),
                  flush=True)
            c.close()
        ctx.trim()


if __name__ == "__main__":
    main()
