"""What scoring NAMED pairs of a resident corpus costs (string_grouper_amd.Corpus.pair_similarities) against the only other
route to the same question: corpus.compute_pairwise_similarities(master.iloc[left], master.iloc[right]), which gathers both sides
into two new Series, vectorises every string of them again and multiplies row i with row i (K9).  Per corpus size (fp32), the
pairs are those of match_strings(corpus.master) at --min-similarity (about 2 M at 663 k names; at most --max-pairs of them, a
seeded sample in the frame's order, so that the old route's two Series fit the host at 5 M names), and 1 000 of them.  The two
routes alternate in one session, --rounds times after one round that only warms up:

  new_ms     corpus.pair_similarities(left, right): two index lists up, one launch, the scores back (the call waits for them)
  old_ms     the two gathers + compute_pairwise_similarities
  bar        the new call's slowest run below the old route's fastest
  pairs_per_s, gathered_bytes (what the kernel has to read and write for these pairs, from the rows' lengths: 16 B of row
             pointers and (4 + 4) B an entry for either row, 8 B of positions, 4 B of score) -- over a kernel time these give its
             share of the 8 TB/s peak; the kernel's time alone comes from a run of --new-only under
             rocprofv3 --kernel-trace --stats (scripts/kstats.py prints it)
  checked    the new scores are, bit for bit, the similarities of the frame (diagonal apart: the frames set it to 1); how many of
             the old route's scores differ from them in the last bits (K9 sums in numpy's order)

One JSON line per round, then one summary per pair count.
python scripts/pair_similarities_latency.py [--corpora 663000,5000000] [--rounds 3] [--new-only]"""
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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def gathered_bytes(lengths, left, right) -> int:
    entries = int(lengths[left].sum() + lengths[right].sum())
    return entries * 8 + len(left) * (2 * 16 + 8 + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", default="663000,5000000")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-similarity", type=float, default=0.8)
    ap.add_argument("--max-pairs", type=int, default=2_500_000)
    ap.add_argument("--new-only", action="store_true", help="the new call alone (for a kernel trace)")
    a = ap.parse_args()
    ctx = N.default_context(0)
    E.set_engine(E.HipEngine(ctx))
    rng = np.random.default_rng(7)
    for n_corpus in [int(x) for x in a.corpora.split(",")]:
        master = pd.Series(synth_names(n_corpus, 1234))
        corpus = sga.Corpus(master, tfidf_matrix_dtype=np.float32, min_similarity=a.min_similarity)
        frame = corpus.match_strings(corpus.master)
        left, right = frame.left_index.to_numpy(), frame.right_index.to_numpy()
        frame_sims = frame.similarity.to_numpy()
        n_frame = len(left)
        del frame
        if n_frame > a.max_pairs:
            keep = np.sort(rng.choice(n_frame, a.max_pairs, replace=False))
            left, right, frame_sims = left[keep], right[keep], frame_sims[keep]
        few = np.sort(rng.choice(len(left), 1000, replace=False))
        lengths = np.diff(corpus._state.physical().to_scipy().indptr)
        print(json.dumps({"corpus": n_corpus, "frame_pairs": n_frame, "pairs": len(left), "mean_row_entries": round(float(lengths.mean()), 2)}),
              flush=True)
        for what, (l, r, sims) in (("all", (left, right, frame_sims)), ("1000", (left[few], right[few], frame_sims[few]))):
            new_ms, old_ms, new, old = [], [], None, None
            for rnd in range(-1, a.rounds):                    # round -1 warms both routes up at this size
                new, t_new = timed(lambda: corpus.pair_similarities(l, r))
                row = {"corpus": n_corpus, "pairs": len(l), "round": rnd, "new_ms": round(t_new, 3)}
                if not a.new_only:
                    old, t_old = timed(lambda: corpus.compute_pairwise_similarities(master.iloc[l], master.iloc[r]).to_numpy())
                    row["old_ms"] = round(t_old, 3)
                if rnd >= 0:
                    new_ms.append(t_new)
                    if not a.new_only:
                        old_ms.append(t_old)
                print(json.dumps(row), flush=True)
            off = l != r
            same = np.array_equal(new[off].astype(np.float64).view(np.uint64), sims[off].view(np.uint64))
            summary = {"corpus": n_corpus, "pairs": len(l), "what": what, "new_ms": [round(x, 3) for x in new_ms],
                       "checked_bit_for_bit_against_the_frame": bool(same), "off_diagonal": int(off.sum()),
                       "pairs_per_s_at_the_slowest_new": round(len(l) / (max(new_ms) * 1e-3)),
                       "gathered_bytes": gathered_bytes(lengths, l, r)}
            if not a.new_only:
                summary.update(old_ms=[round(x, 3) for x in old_ms], bar_new_slowest_below_old_fastest=bool(max(new_ms) < min(old_ms)),
                               old_fastest_over_new_slowest=round(min(old_ms) / max(new_ms), 1),
                               old_scores_that_differ_in_bits=int(np.count_nonzero(old.view(np.uint32) != new.view(np.uint32))),
                               old_max_abs_difference=float(np.max(np.abs(old.astype(np.float64) - new.astype(np.float64)))))
            print(json.dumps({"summary": summary}), flush=True)
            if not same:
                raise SystemExit("pair_similarities does not reproduce the frame's similarities")
        st = corpus.stats
        print(json.dumps({"corpus": n_corpus, "stats": {k: st[k] for k in ("tokenisations", "pair_calls", "pairs_scored", "compactions")}}),
              flush=True)
        corpus.close()
        ctx.trim()


if __name__ == "__main__":
    main()
