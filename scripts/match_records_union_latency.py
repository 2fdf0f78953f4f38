"""What matching RECORDS of three fields costs with candidates from TWO fields -- Corpus.match_records(candidate_fields=(0, 1)):
the names' and the addresses' multiplies united on the device (sg_topn_union), the union rescored (sg_topn_rescore) -- against
the composed union route it replaces, in one session:

  composed   names.match_strings and addresses.match_strings at the candidate options (two frames of EVERY candidate come down),
             the union of their position pairs in pandas, pair_similarities on all three corpora over the union (two position
             lists up and the scores down, a field), then numpy and pandas: the weighed sum in float32, the filter, the order by
             record, combined similarity descending and right position, the cut, the frame of the survivors
  new        names.match_records([addresses, cities], candidate_fields=(0, 1), ...): the same frame, only the survivors come down

Records, options and rounds as in scripts/match_records_latency.py (whose arrangement of the fields by one seeded coin this
script imports): fp32, candidates at 0.6 / top 50 on name and address, final 0.8 / top 20, force_symmetries=False on both routes;
one round that only warms up, then --rounds rounds alternating between the two.

  new_ms, composed_ms (and its split: the two match_strings, the union in pandas, the pair calls, the host tail) per round
  candidates before the union (the two frames' rows) and after it, survivors; frames_equal (assert_frame_equal, last round)
  bar        the new call's slowest run below the composed route's fastest
  new_split  one further new call taken apart, a wait after every step: the two multiplies, the union, the rescoring, the match
             list (K6 and its download)

--trace-run: one new call, nothing else -- for a run of its own under rocprofv3 --kernel-trace --stats (scripts/kstats.py prints
the kernels' times): union_short_kernel, union_block_kernel, union_fill_kernel and union_copy_kernel beside rescore_score_kernel.
Every GPU step runs under a time limit of its own, one process a size, and a step that fails ends the session (the machines are
shared: nothing is started on a card after a fault or a time limit).  As recorded in profiles/match_records_union_latency.log:
  timeout -k 10 300 python scripts/match_records_union_latency.py --records 663000
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- \
      python scripts/match_records_union_latency.py --records 663000 --trace-run   &&  python scripts/kstats.py <dir>/.../t_kernel_stats.csv 40
  timeout -k 10 900 python scripts/match_records_union_latency.py --records 5000000
python scripts/match_records_union_latency.py [--records 663000] [--rounds 3] [--trace-run]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import string_grouper_amd as sga  # noqa: E402
import string_grouper_amd.engine as E  # noqa: E402
from match_records_latency import CAND, FINAL, W, arranged, timed  # noqa: E402
from string_grouper_amd import _native as N  # noqa: E402
from string_grouper_amd.synth import synth_names  # noqa: E402

FIELDS = (0, 1)


def composed(corpora, split):
    T = np.float32
    names = corpora[0]
    frames, t0 = timed(lambda: [corpora[f].match_strings(corpora[f].master, force_symmetries=False, **CAND) for f in FIELDS])

    def unite():                                                              # (a RangeIndex: labels are positions)
        pairs = pd.concat([f[["left_index", "right_index"]] for f in frames], ignore_index=True).drop_duplicates(ignore_index=True)
        return pairs.left_index.to_numpy(), pairs.right_index.to_numpy()
    (lp, rp), t1 = timed(unite)
    scores, t2 = timed(lambda: [c.pair_similarities(lp, rp) for c in corpora])

    def tail():
        acc = np.zeros(len(lp), T)
        for w, s in zip(W, scores):
            acc = acc + T(w) * s
        keep = np.flatnonzero(acc > T(FINAL["min_similarity"]))
        order = keep[np.lexsort((rp[keep], -acc[keep], lp[keep]))]
        rank = np.arange(len(order)) - np.searchsorted(lp[order], lp[order], side="left")
        order = order[rank < FINAL["max_n_matches"]]
        order = order[np.lexsort((rp[order], lp[order]))]                     # a float32 list comes back with rows by column
        master = names.master
        left, right = master.iloc[lp[order]], master.iloc[rp[order]]
        return pd.DataFrame({"left_index": left.index.to_numpy(), f"left_{master.name}": left.to_numpy(),
                             "similarity": acc[order].astype(np.float64), f"right_{master.name}": right.to_numpy(),
                             "right_index": right.index.to_numpy()})
    out, t3 = timed(tail)
    split.update(match_strings_ms=round(t0, 1), union_in_pandas_ms=round(t1, 1), pair_calls_ms=round(t2, 1), host_tail_ms=round(t3, 1),
                 candidates_before_union=int(sum(len(f) for f in frames)), candidates=len(lp))
    return out


def new_split(eng, ctx, corpora):
    """One new call taken apart, a wait after every step (the stages of CorpusEngine.corpus_records with candidate_fields)."""
    states = [c._live() for c in corpora]
    out = {}

    def step(name, fn):
        t0 = time.perf_counter()
        res = fn()
        ctx.sync()
        out[name + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        return res

    with N.Scope() as s:
        parts = [s.own(step(f"multiply_field_{f}", lambda f=f: eng._topn_device(states[f].matrix, states[f].matrix, CAND["max_n_matches"],
                                                                                CAND["min_similarity"]))) for f in FIELDS]
        rows = states[0].physical()
        cand = s.own(step("union", lambda: ctx.topn_union(parts, (rows, rows, states[0].dead_dev, states[0].dead_dev))))
        out["union_stride"] = cand.dims()[1]
        fields = [(o.physical(), o.physical(), w, o.dead_dev, o.dead_dev) for o, w in zip(states[1:], W[1:])]
        res = s.own(step("rescore", lambda: ctx.topn_rescore(cand, W[0], fields, FINAL["min_similarity"], FINAL["max_n_matches"])))
        step("match_list_k6_and_download", lambda: eng._match_list_from_topn(res, np.float32, states[0].matrix.shape[0], False, False,
                                                                             time.perf_counter()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="663000", help="one size a process, each under its own time limit (see above)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-run", action="store_true", help="one new call, nothing else (for a kernel trace)")
    a = ap.parse_args()
    ctx = N.default_context(0)
    eng = E.HipEngine(ctx)
    E.set_engine(eng)
    rng = np.random.default_rng(7)
    for n in [int(x) for x in a.records.split(",")]:
        kw = dict(tfidf_matrix_dtype=np.float32)
        names = sga.Corpus(pd.Series(synth_names(n, 1234), name="name"), **kw)
        frame = names.match_strings(names.master, force_symmetries=False, **CAND)
        off = frame[frame.left_index > frame.right_index]
        partner = np.full(n, -1, np.int64)
        first = off.groupby("left_index").right_index.min()
        partner[first.index.to_numpy()] = first.to_numpy()
        del frame, off, first
        addresses = sga.Corpus(arranged(pd.Series(synth_names(n, 1235, perturb_frac=0.0)), partner, rng), **kw)
        cities = sga.Corpus(arranged(pd.Series(synth_names(n, 1236, perturb_frac=0.0)), partner, rng), **kw)
        corpora = [names, addresses, cities]

        def new():
            return names.match_records([addresses, cities], weights=W, candidates=CAND, candidate_fields=FIELDS,
                                       force_symmetries=False, **FINAL)

        if a.trace_run:
            new()                                                             # (builds the two indexes)
            got, t_new = timed(new)
            print(json.dumps({"records": n, "trace_run": True, "survivors": len(got), "new_ms": round(t_new, 1)}), flush=True)
        else:
            new_ms, composed_ms, got, want, split = [], [], None, None, {}
            for rnd in range(-1, a.rounds):                                   # round -1 warms both routes up at this size
                got, t_new = timed(new)
                split = {}
                want, t_old = timed(lambda: composed(corpora, split))
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
            print(json.dumps({"summary": {
                "records": n, "candidates_before_union": split["candidates_before_union"], "candidates": split["candidates"],
                "survivors": len(got), "frames_equal": equal,
                "new_ms": [round(x, 1) for x in new_ms], "composed_ms": [round(x, 1) for x in composed_ms],
                "bar_new_slowest_below_composed_fastest": bool(max(new_ms) < min(composed_ms)),
                "composed_fastest_over_new_slowest": round(min(composed_ms) / max(new_ms), 2),
                "new_split": new_split(eng, ctx, corpora)}}), flush=True)
            if not equal:
                raise SystemExit("match_records(candidate_fields=(0, 1)) does not reproduce the composed union route's frame")
        for c in corpora:
            st = c.stats
            print(json.dumps({"records": n, "stats": {k: st[k] for k in ("tokenisations", "record_calls", "record_union_calls", "pair_calls",
                                                                         "compactions", "index_builds")}}), flush=True)
            c.close()
        ctx.trim()


if __name__ == "__main__":
    main()
