"""What growing a resident corpus costs (string_grouper_amd.Corpus.append), and the measurement behind
engine.HipEngine.CORPUS_COMPACT_SHARE.  Per corpus size, with automatic compaction switched off, the delta segment is grown to
about 0, 1/64, 1/16, 1/8 and 1/4 of the base segment's rows; at every level:

  append_<k>_ms           one append of k rows (1, 32, 1 000; 100 000 while the delta is being grown), device work waited for
  first_query_<k>_ms      the one-name match_strings(corpus.master, name) that follows it (joins the Series, rebuilds the
                          delta's index, runs the reverse path against both indexes)
  query_delta_ms          the same query again: two indexes, nothing to rebuild
  step_ms                 mean of `--run` steps (append one row, match one name): what a living master list pays per record
  compact_ms, first_query_compacted_ms, query_compacted_ms
                          compact(), the query that rebuilds the one index, and the steady query on ONE index over the same rows
                          (query_delta_ms beside query_compacted_ms: what the second index costs a query)

and before all that the only way to add a row without append: close() + Corpus(pd.concat([master, new])) + the same first
query (rebuild_and_query_ms).  The share: a compaction every S * base rows costs (compact + index rebuild) / (S * base) per
appended row, and a step costs the more the larger the delta is; model_step_ms[S] = mean step_ms over the levels up to S
(trapezoid) + that amortised compaction.  One JSON line per level, then one with the model.
python scripts/corpus_append_latency.py [--corpora 663000,5000000] [--run 1000] [--reps 3]"""
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

SHARES = (0.0, 1 / 64, 1 / 16, 1 / 8, 1 / 4)
CHUNK = 100_000


def ms(fn, ctx):
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", default="663000,5000000")
    ap.add_argument("--run", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-similarity", type=float, default=0.8)
    a = ap.parse_args()
    ctx = N.default_context(0)
    eng = E.HipEngine(ctx)
    E.set_engine(eng)
    eng.CORPUS_COMPACT_SHARE = float("inf")          # compaction only where this script asks for it
    kw = dict(min_similarity=a.min_similarity, tfidf_matrix_dtype=np.float32)
    for n_corpus in [int(x) for x in a.corpora.split(",")]:
        pool = synth_names(n_corpus + int(n_corpus * sum(SHARES)) + 2 * CHUNK, 1234)
        master, extra, used = pd.Series(pool[:n_corpus]), pool[n_corpus:], 0
        n_singles = len(SHARES) * (2 * a.run + 1040 * a.reps + 60) + 100
        singles = synth_names(n_singles, 4321, perturb_of=pool[:200_000], perturb_frac=0.5)
        at = 0

        def take(k):
            nonlocal at
            at += k
            return pd.Series(singles[at - k:at])

        def query(cp):
            name = take(1)
            return ms(lambda: cp.match_strings(cp.master, name), ctx)

        cp = sga.Corpus(master, **kw)
        query(cp)
        # the parent's only way to add a row
        rebuild = []
        for _ in range(2):
            one, name = take(1), take(1)

            def rebuild_and_query():
                nonlocal cp
                cp.close()
                cp = sga.Corpus(pd.concat([master, one]), **kw)
                cp.match_strings(cp.master, name)
            rebuild.append(ms(rebuild_and_query, ctx))
        cp.close()
        cp = sga.Corpus(master, **kw)
        query(cp)
        levels = []
        for share in SHARES:
            row = {"corpus": n_corpus, "share": round(share, 5), "rebuild_and_query_ms": round(min(rebuild), 2)}
            big = []
            while share > 0 and delta_rows(cp) < share * n_corpus:
                k = int(min(CHUNK, max(share * n_corpus - delta_rows(cp), 1)))
                chunk = pd.Series(extra[used:used + k])
                assert len(chunk) == k, "the pool of names is used up"
                used += k
                t = ms(lambda: cp.append(chunk), ctx)
                q = query(cp)
                if k == CHUNK:
                    big.append((t, q))
            if big:
                row["append_100000_ms"] = round(statistics.median(t for t, _ in big), 2)
                row["first_query_100000_ms"] = round(statistics.median(q for _, q in big), 2)
            for k in (1, 32, 1000):
                ts, qs = [], []
                for _ in range(a.reps):
                    batch = take(k)
                    ts.append(ms(lambda: cp.append(batch), ctx))
                    qs.append(query(cp))
                row[f"append_{k}_ms"] = round(statistics.median(ts), 3)
                row[f"first_query_{k}_ms"] = round(statistics.median(qs), 3)
            row["query_delta_ms"] = round(min(query(cp) for _ in range(a.reps + 2)), 3)
            t0 = time.perf_counter()
            for _ in range(a.run):
                cp.append(take(1))
                cp.match_strings(cp.master, take(1))
            ctx.sync()
            row["step_ms"] = round((time.perf_counter() - t0) * 1e3 / a.run, 3)
            st = cp.stats
            row["base_rows"], row["delta_rows"] = len(cp.master) - delta_rows(cp), delta_rows(cp)
            row["compact_ms"] = round(ms(cp.compact, ctx), 2)
            row["first_query_compacted_ms"] = round(query(cp), 2)
            row["query_compacted_ms"] = round(min(query(cp) for _ in range(a.reps + 2)), 3)
            row["base_index_builds"], row["index_builds"] = cp.stats["base_index_builds"], cp.stats["index_builds"]
            row["reverse"], row["forward"] = cp.stats["reverse"] - st["reverse"], cp.stats["forward"] - st["forward"]
            levels.append(row)
            print(json.dumps(row), flush=True)
        cp.close()
        ctx.trim()
        # the model: per step, the mean step over the delta's life plus the compaction spread over the rows between two
        model = {}
        for i, share in enumerate(SHARES[1:], start=1):
            steps = [r["step_ms"] for r in levels[:i + 1]]
            at_s = [r["delta_rows"] / r["base_rows"] for r in levels[:i + 1]]
            area = sum((at_s[j + 1] - at_s[j]) * (steps[j] + steps[j + 1]) / 2 for j in range(i))
            mean_step = area / (at_s[i] - at_s[0])
            fold = levels[i]["compact_ms"] + levels[i]["first_query_compacted_ms"] - levels[i]["query_compacted_ms"]
            model[f"1/{round(1 / share)}"] = {"mean_step_ms": round(mean_step, 3),
                                              "compaction_per_row_ms": round(fold / (share * n_corpus), 5),
                                              "model_step_ms": round(mean_step + fold / (share * n_corpus), 3)}
        best = min(model, key=lambda k: model[k]["model_step_ms"])
        print(json.dumps({"corpus": n_corpus, "model": model, "cheapest_share": best,
                          "append_and_query_vs_rebuild": round(levels[0]["rebuild_and_query_ms"] /
                                                               (levels[0]["append_1_ms"] + levels[0]["first_query_1_ms"]), 1)}),
              flush=True)


def delta_rows(cp):
    state = cp._live()
    return state.delta.n_rows if state.delta is not None else 0


if __name__ == "__main__":
    main()
