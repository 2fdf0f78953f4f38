"""Latency of one call on a resident corpus (string_grouper_amd.Corpus) against the module-level function, which refits on
master + batch every call.  For every corpus size and batch size: match_strings(corpus, batch) on the forward path (the
corpus rows against an index of the batch), on the reverse path (the batch against the corpus's resident index, turned
round by sg_topn_transpose_select), what the automatic rule picks, and sga.match_strings(corpus, batch).  Wall-clock of
the whole call (frames included): the best of `reps` after one warm-up call.  One JSON line per (corpus, batch).
python scripts/corpus_latency.py [--corpora 663000,5000000] [--batches 1,100,1000,10000,100000] [--reps 3]"""
import argparse
import json
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, ".")
import string_grouper_amd as sga  # noqa: E402
import string_grouper_amd.engine as E  # noqa: E402
from string_grouper_amd import _native as N  # noqa: E402
from string_grouper_amd.synth import synth_names  # noqa: E402


def best_of(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", default="663000,5000000")
    ap.add_argument("--batches", default="1,100,1000,10000,100000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--module-reps", type=int, default=1)
    ap.add_argument("--min-similarity", type=float, default=0.8)
    a = ap.parse_args()
    ctx = N.default_context(0)
    E.set_engine(E.HipEngine(ctx))
    kw = dict(min_similarity=a.min_similarity, tfidf_matrix_dtype=np.float32)
    for n_corpus in [int(x) for x in a.corpora.split(",")]:
        names = synth_names(n_corpus, 1234)
        corpus = pd.Series(names)
        t0 = time.perf_counter()
        cp = sga.Corpus(corpus, **kw)
        build_s = time.perf_counter() - t0
        for n_batch in [int(x) for x in a.batches.split(",")]:
            batch = pd.Series(synth_names(n_batch, 77 + n_batch, perturb_of=names[:200_000], perturb_frac=0.5))
            row = {"corpus": n_corpus, "batch": n_batch, "corpus_build_s": round(build_s, 4)}
            for label, mode in (("forward_s", "0"), ("reverse_s", "1")):
                ctx.set_option("SG_CORPUS_REVERSE", mode)
                row[label] = round(best_of(lambda: cp.match_strings(corpus, batch), a.reps), 5)
            ctx.set_option("SG_CORPUS_REVERSE", None)
            before = cp.stats
            cp.match_strings(corpus, batch)
            after = cp.stats
            row["auto_pick"] = "reverse" if after["reverse"] > before["reverse"] else "forward"
            row["reverse_fallbacks"] = after["reverse_fallbacks"]
            row["module_level_s"] = round(best_of(lambda: sga.match_strings(corpus, batch, **kw), a.module_reps), 5)
            faster = "reverse" if row["reverse_s"] < row["forward_s"] else "forward"
            picked, other = row[row["auto_pick"] + "_s"], min(row["forward_s"], row["reverse_s"])
            row["faster"] = faster
            row["pick_within_10pct"] = bool(picked <= 1.10 * other)
            print(json.dumps(row), flush=True)
        cp.close()
        ctx.trim()


if __name__ == "__main__":
    main()
