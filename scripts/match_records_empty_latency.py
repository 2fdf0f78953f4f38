"""What leaving a record's empty fields out costs through Corpus.match_records(empty_fields="skip") (decided on the device:
skip_empty of sg_topn_rescore) against the composed route it replaces, in one session.  The set-up is
scripts/match_records_latency.py's: three SynthNames fields arranged by a seeded coin, fp32, candidates at 0.6 / top 50, final
0.8 / top 20, weights 0.5 / 0.3 / 0.2, force_symmetries=False on every route -- and a fifth of the addresses set to "".

  plain      names.match_records([addresses, cities], ...) without the option, on the same records: the survivors it finds
  composed   names.match_strings at the candidate options, a pair_similarities call a further field, which strings are empty
             from the nnz of the rows corpus.vectorizer.transform gives, then numpy and pandas: the sums over the fields that are
             not empty, (c * wt) / wp, the filter, the order, the cut, the frame of the survivors
  new        names.match_records([addresses, cities], empty_fields="skip", ...): the same frame
  rescore    Context.topn_rescore on the SAME candidates (the names' self-join at the candidate options, kept on the device) with
             and without skip_empty, alternating: the call ends with its one read-back, so its wall time is the kernels' time

One round that only warms up, then --rounds rounds alternating.  bar: the new call's slowest run below the composed route's
fastest.  The call WITHOUT the option on this build against its parent is scripts/match_records_floors_latency.py --plain-only,
which runs on both.  Every GPU step runs under a time limit of its own, one process a size (the machines are shared: nothing is
started on a card after a fault or a time limit).  As recorded in profiles/match_records_empty_latency.log:
  timeout -k 10 400 python scripts/match_records_empty_latency.py --records 663000
python scripts/match_records_empty_latency.py [--records 663000] [--rounds 3] [--blank 0.2]"""
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


def composed(names, others):
    T = np.float32
    frame = names.match_strings(names.master, force_symmetries=False, **CAND)
    lp, rp = frame.left_index.to_numpy(), frame.right_index.to_numpy()        # (a RangeIndex: labels are positions)
    corpora = [names] + list(others)
    scores = [frame.similarity.to_numpy().astype(T)] + [o.pair_similarities(lp, rp) for o in others]
    acc, wp, wt = np.zeros(len(frame), T), np.zeros(len(frame), T), T(0)
    some = np.zeros(len(frame), bool)
    for c, w, s in zip(corpora, W, scores):
        blank = np.diff(c.vectorizer.transform(c.master).indptr) == 0
        empty = blank[lp] | blank[rp]
        acc = np.where(empty, acc, acc + T(w) * s).astype(T)
        wp = np.where(empty, wp, wp + T(w)).astype(T)
        wt = T(wt + T(w))
        some |= empty
    with np.errstate(all="ignore"):
        sim = np.where(some, np.where(wp > 0, (acc * wt) / wp, T(np.nan)), acc).astype(T)
    keep = np.flatnonzero(sim > T(FINAL["min_similarity"]))
    order = keep[np.lexsort((rp[keep], -sim[keep], lp[keep]))]
    rank = np.arange(len(order)) - np.searchsorted(lp[order], lp[order], side="left")
    order = order[rank < FINAL["max_n_matches"]]
    order = order[np.lexsort((rp[order], lp[order]))]                         # a float32 list comes back with rows by column
    out = frame.iloc[order].reset_index(drop=True)
    out["similarity"] = sim[order].astype(np.float64)
    return out, len(frame)


def rescore_times(eng, ctx, corpora, rounds):
    """topn_rescore on the same candidates, without and with skip_empty."""
    states = [c._live() for c in corpora]
    A = states[0].matrix
    plain_ms, skip_ms, kept = [], [], []
    with N.Scope() as s:
        cand = s.own(eng._topn_device(A, A, CAND["max_n_matches"], CAND["min_similarity"]))
        fields = []
        for st, w in zip(states[1:], W[1:]):
            rows = st.physical()
            fields.append((rows, rows, w, st.dead_dev, st.dead_dev))
        rows = states[0].physical()
        primary = (rows, rows, states[0].dead_dev, states[0].dead_dev)
        for rnd in range(-1, rounds):
            for into, kw in ((plain_ms, {}), (skip_ms, dict(skip_empty=True, primary=primary))):
                res, ms = timed(lambda: ctx.topn_rescore(cand, W[0], fields, FINAL["min_similarity"], FINAL["max_n_matches"], **kw))
                if rnd >= 0:
                    into.append(ms)
                if rnd == 0:
                    kept.append(int(res.counts().sum()))
                res.free()
    return plain_ms, skip_ms, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="663000", help="one size a process, each under its own time limit (see above)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blank", type=float, default=0.2, help="the share of the addresses set to \"\"")
    a = ap.parse_args()
    ctx = N.default_context(0)
    eng = E.HipEngine(ctx)
    E.set_engine(eng)
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
        address = arranged(pd.Series(synth_names(n, 1235, perturb_frac=0.0)), partner, rng)
        address = pd.Series(np.where(np.random.default_rng(8).random(n) < a.blank, "", address.to_numpy(object)))
        addresses = sga.Corpus(address, **kw)
        cities = sga.Corpus(arranged(pd.Series(synth_names(n, 1236, perturb_frac=0.0)), partner, rng), **kw)
        others = [addresses, cities]

        def plain():
            return names.match_records(others, weights=W, candidates=CAND, force_symmetries=False, **FINAL)

        def new():
            return names.match_records(others, weights=W, candidates=CAND, force_symmetries=False, empty_fields="skip", **FINAL)

        plain_ms = []
        for rnd in range(-1, a.rounds):
            without, t = timed(plain)
            if rnd >= 0:
                plain_ms.append(t)
        new_ms, composed_ms, want, n_cand = [], [], None, 0
        for rnd in range(-1, a.rounds):                                       # round -1 warms both routes up at this size
            got, t_new = timed(new)
            (want, n_cand), t_old = timed(lambda: composed(names, others))
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
        r_plain, r_skip, kept = rescore_times(eng, ctx, [names] + others, a.rounds)
        print(json.dumps({"summary": {
            "records": n, "blank_addresses": int((address == "").sum()), "candidates": n_cand,
            "survivors_without_and_with": [len(without), len(got)], "frames_equal": equal,
            "plain_ms": [round(x, 1) for x in plain_ms], "new_ms": [round(x, 1) for x in new_ms],
            "composed_ms": [round(x, 1) for x in composed_ms],
            "bar_new_slowest_below_composed_fastest": bool(max(new_ms) < min(composed_ms)),
            "composed_fastest_over_new_slowest": round(min(composed_ms) / max(new_ms), 2),
            "rescore_ms_without_skip": [round(x, 2) for x in r_plain], "rescore_ms_with_skip": [round(x, 2) for x in r_skip],
            "rescore_kept_without_and_with": kept}}), flush=True)
        if not equal:
            raise SystemExit("match_records with empty_fields='skip' does not reproduce the composed route's frame")
        for c in (names, addresses, cities):
            st = c.stats
            print(json.dumps({"records": n, "stats": {k: st.get(k) for k in ("tokenisations", "record_calls", "record_skip_empty_calls",
                                                                            "pair_calls", "compactions", "index_builds")}}), flush=True)
            c.close()
        ctx.trim()


if __name__ == "__main__":
    main()
