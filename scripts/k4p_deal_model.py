"""CPU model of how the pruned multiply (K4p, stream + self-join form) deals a wave's 64 lanes to the prefix terms of a
row, on the real index of the headline job: rounds per row, postings per round and idle lanes for
  * floor               G_t = 1 + floor((64 - np) * 0.999 * df_t / dsum)               (the rule until now: SG_DEAL=floor)
  * largest remainder   the spare lanes by quotient, the lanes left over to the largest remainders   (the kernel's rule,
                        string_grouper_amd/csrc/sg_k4_device.h; taken from the built library -- sg_debug_deal_lanes -- when
                        there is one, and restated here in integers either way: the two must agree)
  * per visit           the fewest rounds ANY dealing could need if the lanes were dealt again for every visit
                        (not buildable: a lane's stream runs across visits; the bound)
A visit is a super-tile of 32 768 positions; a lane reads four postings per round, so a visit takes
max(1, max_t ceil(cnt[t, visit] / (4 G_t))) rounds.  Index as the library builds it: one row per distinct string, rows in
position order (pos = j * M mod n), frequent from 0.5 % of the rows, suffix under beta = threshold - delta.

    python scripts/k4p_deal_model.py [rows=663000] [sample=1200] [threshold=0.8] [delta=0.03]
"""
import ctypes
import os
import sys
import time

import numpy as np
from sklearn.feature_extraction.text import TfidfVectorizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from string_grouper_amd.synth import synth_names  # noqa: E402

SUPER = 32768


def deal_floor(df):
    f32 = np.float32
    share = df.astype(f32) / f32(int(df.sum()))
    return 1 + np.floor(f32(64 - len(df)) * f32(0.999) * share).astype(np.int64)


def deal_largest_remainder(df):
    n, dsum, spare = len(df), int(df.sum()), 64 - len(df)
    G = 1 + spare * df // dsum
    rem = spare * df % dsum
    for t in np.lexsort((np.arange(n), -rem))[:64 - int(G.sum())]:
        G[t] += 1
    return G


def library_rule():
    path = os.path.join(ROOT, "string_grouper_amd", "libsg_hip.so")
    if not os.path.exists(path):
        return None
    fn = ctypes.CDLL(path).sg_debug_deal_lanes
    fn.restype = ctypes.c_int

    def call(df):
        d = np.ascontiguousarray(df, np.uint32)
        out = np.zeros(len(d), np.uint32)
        assert fn(ctypes.c_void_p(d.ctypes.data), ctypes.c_int(len(d)), ctypes.c_void_p(out.ctypes.data), ctypes.c_int(0)) == 0
        return out.astype(np.int64)
    return call


def fewest_rounds(cnt):
    """smallest r with sum_t ceil(cnt_t / (4 r)) <= 64 over the terms that have postings in the visit (the others: a lane each)"""
    idle_terms = int((cnt == 0).sum())
    c = cnt[cnt > 0]
    r = 1
    while int(np.ceil(c / (4.0 * r)).sum()) + idle_terms > 64:
        r += 1
    return r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 663000
    n_sample = int(sys.argv[2]) if len(sys.argv) > 2 else 1200
    thr = float(sys.argv[3]) if len(sys.argv) > 3 else 0.8
    delta = float(sys.argv[4]) if len(sys.argv) > 4 else 0.03
    t0 = time.time()
    names = sorted(set(synth_names(n, 1234)))           # identical strings are one index row
    n = len(names)
    m = TfidfVectorizer(analyzer="char", ngram_range=(3, 3), lowercase=True, dtype=np.float32).fit_transform(names).tocsr()
    m.sort_indices()
    mult = int(0.6180339887498949 * n) | 1
    while np.gcd(mult, n) != 1:
        mult += 2
    pos_of = (np.arange(n, dtype=np.int64) * mult) % n
    orig_of = np.empty(n, np.int64)
    orig_of[pos_of] = np.arange(n)
    m = m[orig_of]            # rows in position order
    mt = m.T.tocsr()
    mt.sort_indices()
    print(f"# {n} index rows, nnz {m.nnz}, {time.time() - t0:.1f} s", flush=True)
    df_all = np.diff(mt.indptr)
    freq_min = max(1, int(0.005 * n))
    norm_up = float(np.sqrt(np.asarray(m.multiply(m).sum(axis=1)).max())) * 1.000001
    budget = ((thr - delta) / norm_up) ** 2 * (1.0 - 1e-6)
    rows = np.sort(np.random.default_rng(7).choice(n, n_sample, replace=False))
    lib = library_rule()
    rules = {"floor": deal_floor, "largest remainder": deal_largest_remainder}
    tot = {name: dict(rounds=0, idle=0) for name in list(rules) + ["per visit (bound)"]}
    n_rows = postings = terms = visits = 0
    for i in rows:
        k = m.indices[m.indptr[i]:m.indptr[i + 1]]
        a = m.data[m.indptr[i]:m.indptr[i + 1]].astype(np.float64)
        if len(k) == 0 or len(k) > 64:
            continue
        df = df_all[k].astype(np.int64)
        order = np.lexsort((np.arange(len(k)), -df))
        cum = np.empty(len(k))
        cum[order] = np.cumsum((a * a * 1.00001)[order])
        in_p = ~((cum <= budget) & (df >= freq_min))
        if not in_p.any():
            continue
        dfp = df[in_p]
        n_visits = i // SUPER + 1
        cnt = np.zeros((len(dfp), n_visits), np.int64)      # postings of term t in visit v, columns up to the row's own tile's end
        for q, term in enumerate(k[in_p]):
            c = mt.indices[mt.indptr[term]:mt.indptr[term + 1]]
            cnt[q] = np.bincount(c[c < (i // 4096 + 1) * 4096] // SUPER, minlength=n_visits)
        n_rows += 1
        postings += int(cnt.sum())
        terms += len(dfp)
        visits += n_visits
        for name, rule in rules.items():
            G = rule(dfp)
            if name == "largest remainder":
                assert G.sum() == 64 and (lib is None or np.array_equal(G, lib(dfp))), (dfp, G)
            tot[name]["rounds"] += int(np.maximum(1, np.ceil(cnt / (4.0 * G[:, None])).max(axis=0)).sum())
            tot[name]["idle"] += 64 - int(G.sum())
        tot["per visit (bound)"]["rounds"] += sum(fewest_rounds(cnt[:, v]) for v in range(n_visits))
    print(f"rows sampled {n_rows}: {terms / n_rows:.1f} prefix terms, {visits / n_rows:.1f} visits, {postings / n_rows:.0f} postings a row"
          f"{'' if lib is not None else '   (no built library: the rule from its restatement alone)'}")
    print("dealing              | rounds / row | postings / round (fill) | idle lanes / row | rounds against floor")
    for name, r in tot.items():
        print(f"{name:20s} | {r['rounds'] / n_rows:12.2f} | {postings / r['rounds']:8.1f} ({postings / r['rounds'] / 256:.2f})        | "
              f"{r['idle'] / n_rows:16.2f} | {r['rounds'] / tot['floor']['rounds'] - 1:+.1%}")


if __name__ == "__main__":
    main()
