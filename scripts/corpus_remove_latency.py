"""What forgetting rows of a resident corpus costs (string_grouper_amd.Corpus.remove), and the measurement behind
engine.HipEngine.CORPUS_MAX_DEAD.  Per corpus size (fp32, min_similarity 0.8, device work waited for):

  rebuild_and_query_ms    the only way to drop a row without remove: close() + Corpus(master[keep]) + a one-name query
  then, with automatic compaction switched off, at dead_rows = 0, 8, 32, 64, 128 one JSON line with
  remove_1_ms             one remove of one row, split into remove_1_engine_ms (the dead list: merged, uploaded) and
                          remove_1_host_ms (the Series copied without the row -- follows the corpus, not the batch)
  query_1_ms              match_strings(corpus.master, one name): the reverse path against the index, dead columns filtered
  query_1000_ms           match_strings(1 000 names, corpus.master): the resident index asked for top_n + dead_rows
  and at the last level
  compact_ms, first_query_compacted_ms, query_compacted_ms
                          compact(), the query that rebuilds the index, the steady query on the clean segment
  then per cap (CORPUS_MAX_DEAD = 8, 32, 64, 128), `--rounds` times over, one line with
  step_ms                 mean of `--run` steps of a living list: remove one row, append one row, match one name
                          (compactions by the cap and by append's share rule included; step_host_ms: the Series' part, which
                          no cap touches; step_device_ms: the rest)

python scripts/corpus_remove_latency.py [--corpora 663000,5000000] [--run 400] [--reps 5] [--rounds 2]"""
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

LEVELS = (0, 8, 32, 64, 128)
CAPS = (8, 32, 64, 128)


def ms(fn, ctx):
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", default="663000,5000000")
    ap.add_argument("--run", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--min-similarity", type=float, default=0.8)
    a = ap.parse_args()
    ctx = N.default_context(0)
    eng = E.HipEngine(ctx)
    E.set_engine(eng)
    default_cap = eng.CORPUS_MAX_DEAD
    kw = dict(min_similarity=a.min_similarity, tfidf_matrix_dtype=np.float32)
    # the engine's share of a remove, timed where it happens (device work waited for)
    engine_ms = [0.0]
    inner = eng.corpus_remove

    def timed_remove(state, positions):
        engine_ms[0] += ms(lambda: inner(state, positions), ctx)
    eng.corpus_remove = timed_remove
    rng = np.random.default_rng(5)
    for n_corpus in [int(x) for x in a.corpora.split(",")]:
        pool = synth_names(n_corpus, 1234)
        master = pd.Series(pool)
        n_singles = 20 * a.reps + a.rounds * len(CAPS) * (2 * a.run + 1) + 400
        singles = synth_names(n_singles, 4321, perturb_of=pool[:200_000], perturb_frac=0.5)
        batch = pd.Series(synth_names(1000, 987, perturb_of=pool[:200_000], perturb_frac=0.5))
        at = 0

        def take(k):
            nonlocal at
            at += k
            return pd.Series(singles[at - k:at])

        def query(cp):
            name = take(1)
            return ms(lambda: cp.match_strings(cp.master, name), ctx)

        def query_batch(cp):
            return ms(lambda: cp.match_strings(batch, cp.master), ctx)

        def remove_one(cp):
            """(total, engine part, host part) of one remove of one random row"""
            row = int(rng.integers(0, len(cp.master)))
            engine_ms[0] = 0.0
            total = ms(lambda: cp.remove(row), ctx)
            return total, engine_ms[0], total - engine_ms[0]

        cp = sga.Corpus(master, **kw)
        query(cp)
        # the parent's only way to drop a row
        rebuild = []
        for _ in range(2):
            row, name = int(rng.integers(0, n_corpus)), take(1)
            keep = np.ones(n_corpus, bool)
            keep[row] = False

            def rebuild_and_query():
                nonlocal cp
                cp.close()
                cp = sga.Corpus(master[keep], **kw)
                cp.match_strings(cp.master, name)
            rebuild.append(ms(rebuild_and_query, ctx))
        cp.close()
        cp = sga.Corpus(master, **kw)
        query(cp)
        query_batch(cp)
        eng.CORPUS_MAX_DEAD = 1 << 30                     # compaction only where this script asks for it
        for level in LEVELS:
            row = {"corpus": n_corpus, "dead_rows": level, "rebuild_and_query_ms": round(min(rebuild), 2)}
            parts = []
            if level == 0:                               # measured on a clean corpus, each one folded in again
                for _ in range(a.reps):
                    parts.append(remove_one(cp))
                    cp.compact()
                query(cp)
                query_batch(cp)
            else:
                bulk = level - cp.stats["dead_rows"] - a.reps
                if bulk > 0:
                    cp.remove(rng.choice(len(cp.master), bulk, replace=False))
                while cp.stats["dead_rows"] < level:
                    parts.append(remove_one(cp))
            assert cp.stats["dead_rows"] == level, cp.stats
            row["remove_1_ms"] = round(statistics.median(p[0] for p in parts), 3)
            row["remove_1_engine_ms"] = round(statistics.median(p[1] for p in parts), 3)
            row["remove_1_host_ms"] = round(statistics.median(p[2] for p in parts), 3)
            row["query_1_ms"] = round(min(query(cp) for _ in range(a.reps + 2)), 3)
            row["query_1000_ms"] = round(min(query_batch(cp) for _ in range(a.reps)), 3)
            if level == LEVELS[-1]:
                row["compact_ms"] = round(ms(cp.compact, ctx), 2)
                row["first_query_compacted_ms"] = round(query(cp), 2)
                row["query_compacted_ms"] = round(min(query(cp) for _ in range(a.reps + 2)), 3)
            row["compactions"], row["base_index_builds"] = cp.stats["compactions"], cp.stats["base_index_builds"]
            print(json.dumps(row), flush=True)
        summary, device = {cap: [] for cap in CAPS}, {cap: [] for cap in CAPS}
        for rnd in range(a.rounds):                      # the caps in turn, more than once: what a step's jitter is
            for cap in CAPS:
                eng.CORPUS_MAX_DEAD = cap
                cp.compact()
                query(cp)
                st = cp.stats
                engine_ms[0] = 0.0
                host = 0.0
                t0 = time.perf_counter()
                for _ in range(a.run):
                    h0 = time.perf_counter()
                    e0 = engine_ms[0]
                    cp.remove(int(rng.integers(0, len(cp.master))))
                    host += (time.perf_counter() - h0) * 1e3 - (engine_ms[0] - e0)
                    cp.append(take(1))
                    cp.match_strings(cp.master, take(1))
                ctx.sync()
                step = (time.perf_counter() - t0) * 1e3 / a.run
                now = cp.stats
                summary[cap].append(round(step, 3))
                device[cap].append(round(step - host / a.run, 3))
                print(json.dumps({"corpus": n_corpus, "cap": cap, "round": rnd, "step_ms": round(step, 3),
                                  "step_host_ms": round(host / a.run, 3), "step_device_ms": device[cap][-1],
                                  "step_engine_remove_ms": round(engine_ms[0] / a.run, 3), "steps": a.run,
                                  "compactions": now["compactions"] - st["compactions"],
                                  "base_index_builds": now["base_index_builds"] - st["base_index_builds"],
                                  "reverse": now["reverse"] - st["reverse"], "forward": now["forward"] - st["forward"]}), flush=True)
        print(json.dumps({"corpus": n_corpus, "step_ms_by_cap": summary, "step_device_ms_by_cap": device,
                          "cheapest_cap_by_round": [min(CAPS, key=lambda c: summary[c][r]) for r in range(a.rounds)],
                          "default_cap": default_cap}), flush=True)
        cp.close()
        ctx.trim()


if __name__ == "__main__":
    main()
