"""What keeping the self-join of a resident corpus costs and saves (string_grouper_amd.Corpus.keep_self_join).  Per corpus size
(fp32, min_similarity 0.8, max_n_matches 20, device work waited for) two steps of a deduplication service are timed, each with
the result kept and without -- without is the path a corpus takes that never calls keep_self_join:

  append_group      append one row, then group_similar_strings(corpus.master)
  remove_append_group
                    remove one row, append one row, then group_similar_strings(corpus.master)

The two corpora (kept / not kept) live side by side and take the same changes; kept and not kept alternate inside every
round, `--rounds` rounds of `--run` steps each.  One JSON line per (step, kept, round):

  step_ms           mean wall time of a step
  engine_ms         its part inside the engine, every call followed by a synchronise: corpus_append / corpus_remove (with the
                    kept result's updates), the multiply or the served copy + the match list + its download (match_list) and
                    the group representatives (K8)
  append_ms, remove_ms, group_engine_ms
                    engine_ms by call
  host_ms           the rest: the Series joined or copied, the frames built by pandas
  and the counters of the kept result over the round (full multiplies, served calls, rows refilled).

The last line per size has the medians over the rounds and, at the end, whether the two corpora's groups are equal.

python scripts/corpus_selfjoin_latency.py [--corpora 663000,5000000] [--run 10] [--rounds 3]"""
import argparse
import functools
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

STEPS = ("append_group", "remove_append_group")
COUNTERS = ("self_join_full", "self_join_served", "self_join_append_updates", "self_join_remove_updates",
            "self_join_rows_refilled", "compactions", "base_index_builds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", default="663000,5000000")
    ap.add_argument("--run", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-similarity", type=float, default=0.8)
    ap.add_argument("--max-n-matches", type=int, default=20)
    a = ap.parse_args()
    ctx = N.default_context(0)
    eng = E.HipEngine(ctx)
    E.set_engine(eng)
    kw = dict(min_similarity=a.min_similarity, max_n_matches=a.max_n_matches, tfidf_matrix_dtype=np.float32)

    # the engine's part of a step, timed where it happens (device work waited for)
    spent = {"append": 0.0, "remove": 0.0, "group": 0.0}

    def timed(fn, what):
        @functools.wraps(fn)                      # (fit() looks at match_list's signature)
        def call(*args, **kwargs):
            t0 = time.perf_counter()
            out = fn(*args, **kwargs)
            ctx.sync()
            spent[what] += (time.perf_counter() - t0) * 1e3
            return out
        return call
    eng.corpus_append = timed(eng.corpus_append, "append")
    eng.corpus_remove = timed(eng.corpus_remove, "remove")
    eng.match_list = timed(eng.match_list, "group")
    E.DeviceMatchList.group_reps = timed(E.DeviceMatchList.group_reps, "group")

    for n_corpus in [int(x) for x in a.corpora.split(",")]:
        rng = np.random.default_rng(5)
        pool = synth_names(n_corpus, 1234)
        master = pd.Series(pool)
        n_singles = 2 * len(STEPS) * a.rounds * a.run + 64
        singles = synth_names(n_singles, 4321, perturb_of=pool[:200_000], perturb_frac=0.5)
        corpora = {True: sga.Corpus(master, **kw), False: sga.Corpus(master, **kw)}
        corpora[True].keep_self_join()
        at = 0

        def one_step(cp, step, name, row):
            if step == "remove_append_group":
                cp.remove(row)
            cp.append(pd.Series([name]))
            return cp.group_similar_strings(cp.master)

        # warm-up: the first multiply (kept: the one whole multiply it ever makes), every path of both steps once
        t0 = time.perf_counter()
        for kept, cp in corpora.items():
            cp.group_similar_strings(cp.master)
        ctx.sync()
        print(json.dumps({"corpus": n_corpus, "first_group_of_both_ms": round((time.perf_counter() - t0) * 1e3, 1)}), flush=True)
        for step in STEPS:
            row = int(rng.integers(0, len(corpora[True].master)))
            for kept, cp in corpora.items():
                one_step(cp, step, singles[at], row)
            at += 1
        ctx.sync()

        rows = {(s, k): [] for s in STEPS for k in (True, False)}
        for rnd in range(a.rounds):
            for step in STEPS:
                # the same changes for both corpora, so that they stay the same list
                changes = [(singles[at + i], int(rng.integers(0, len(corpora[True].master) - a.run))) for i in range(a.run)]
                at += a.run
                for kept in ((True, False) if rnd % 2 == 0 else (False, True)):
                    cp = corpora[kept]
                    before = cp.stats
                    for k in spent:
                        spent[k] = 0.0
                    ctx.sync()
                    t0 = time.perf_counter()
                    for name, row in changes:
                        one_step(cp, step, name, row)
                    ctx.sync()
                    step_ms = (time.perf_counter() - t0) * 1e3 / a.run
                    engine_ms = sum(spent.values()) / a.run
                    now = cp.stats
                    line = {"corpus": n_corpus, "step": step, "kept": kept, "round": rnd, "steps": a.run,
                            "step_ms": round(step_ms, 3), "engine_ms": round(engine_ms, 3),
                            "host_ms": round(step_ms - engine_ms, 3), "append_ms": round(spent["append"] / a.run, 3),
                            "remove_ms": round(spent["remove"] / a.run, 3), "group_engine_ms": round(spent["group"] / a.run, 3)}
                    line.update({c: now[c] - before[c] for c in COUNTERS})
                    rows[(step, kept)].append(line)
                    print(json.dumps(line), flush=True)
        groups = {kept: cp.group_similar_strings(cp.master) for kept, cp in corpora.items()}
        summary = {"corpus": n_corpus, "rows_now": len(corpora[True].master), "groups_equal": bool(groups[True].equals(groups[False]))}
        for step in STEPS:
            for kept in (True, False):
                tag = f"{step}_{'kept' if kept else 'not_kept'}"
                for field in ("step_ms", "engine_ms", "host_ms"):
                    summary[f"{tag}_{field}"] = round(statistics.median(r[field] for r in rows[(step, kept)]), 3)
        print(json.dumps(summary), flush=True)
        for cp in corpora.values():
            cp.close()
        ctx.trim()


if __name__ == "__main__":
    main()
