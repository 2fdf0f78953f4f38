"""What refreshing the idf of a resident corpus costs (string_grouper_amd.Corpus.refit_idf) against the only other way to an idf
that follows the list: close() + Corpus(corpus.master), which prepares, tokenises, fits, weights and indexes every string again.
Per corpus size, `--rounds` times in one session, the two alternating: 1 000 rows are appended and 100 removed (neither folded
in: the refit compacts), then

  refit_ms                     corpus.refit_idf(), device work waited for, and its parts:
    rows_ms                      the live rows in one matrix (sg_csr_concat + sg_csr_select_rows: the compaction)
    counts_ms                    entries per column (sg_csr_column_counts; one synchronisation)
    host_idf_ms                  numpy's idf of the counts
    reweigh_ms                   sg_vec_reweigh (the upload of the idf, the kernel, one synchronisation)
  refit_first_query_ms         the one-name match_strings(corpus.master, name) that follows: it builds the new rows' index
  query_ms                     the same query again
  rebuild_ms                   close() + Corpus(corpus.master) on the same list
  rebuild_first_query_ms       its first query (the index build)

One JSON line per round, then one with the medians.
python scripts/corpus_refit_idf_latency.py [--corpora 663000,5000000] [--rounds 3]"""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, ".")
import string_grouper_amd as sga  # noqa: E402
import string_grouper_amd.engine as E  # noqa: E402
from string_grouper_amd import _native as N  # noqa: E402
from string_grouper_amd.synth import synth_names  # noqa: E402

APPENDED, REMOVED = 1000, 100


def ms(fn, ctx):
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", default="663000,5000000")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-similarity", type=float, default=0.8)
    a = ap.parse_args()
    ctx = N.default_context(0)
    eng = E.HipEngine(ctx)
    E.set_engine(eng)
    eng.CORPUS_COMPACT_SHARE = float("inf")          # the appended and the removed rows are pending when the refit comes
    eng.CORPUS_MAX_DEAD = 10 ** 9
    kw = dict(min_similarity=a.min_similarity, tfidf_matrix_dtype=np.float32)
    rng = np.random.default_rng(7)
    for n_corpus in [int(x) for x in a.corpora.split(",")]:
        pool = synth_names(n_corpus + a.rounds * APPENDED, 1234)
        names = synth_names(8 * a.rounds + 8, 4321, perturb_of=pool[:200_000], perturb_frac=0.5)
        at = 0

        def query(cp):
            nonlocal at
            at += 1
            name = pd.Series(names[at - 1:at])
            return ms(lambda: cp.match_strings(cp.master, name), ctx)

        cp = sga.Corpus(pd.Series(pool[:n_corpus]), **kw)
        query(cp)
        rounds = []
        for r in range(a.rounds):
            cp.append(pd.Series(pool[n_corpus + r * APPENDED:n_corpus + (r + 1) * APPENDED]))
            cp.remove(np.sort(rng.choice(len(cp.master), REMOVED, replace=False)))
            query(cp)
            row = {"corpus": n_corpus, "round": r, "rows": len(cp.master)}
            row["refit_ms"] = round(ms(cp.refit_idf, ctx), 3)
            row.update({k[len("refit_"):-2] + "_ms": round(v * 1e3, 3) for k, v in eng.timings.items() if k.startswith("refit_")})
            row["refit_first_query_ms"] = round(query(cp), 3)
            row["query_ms"] = round(min(query(cp) for _ in range(3)), 3)
            current = cp.master

            def rebuild():
                nonlocal cp
                cp.close()
                cp = sga.Corpus(current, **kw)
            row["rebuild_ms"] = round(ms(rebuild, ctx), 3)
            row["rebuild_first_query_ms"] = round(query(cp), 3)
            st = cp.stats
            row["tokenisations_of_the_rebuilt"] = st["tokenisations"]
            rounds.append(row)
            print(json.dumps(row), flush=True)
        keys = [k for k in rounds[0] if k.endswith("_ms")]
        med = {k: round(statistics.median(r[k] for r in rounds), 3) for k in keys}
        med["corpus"] = n_corpus
        med["rebuild_over_refit"] = round((med["rebuild_ms"] + med["rebuild_first_query_ms"]) /
                                          (med["refit_ms"] + med["refit_first_query_ms"]), 2)
        print(json.dumps({"medians": med}), flush=True)
        cp.close()
        ctx.trim()


if __name__ == "__main__":
    main()
