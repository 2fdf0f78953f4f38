"""The second filter's EARLY EXIT restated (sg_postings.hip: q8_rest_word; sg_spgemm_pruned.hip: q8_passes) and a matrix
built so that one left row's candidates leave their records at every stored boundary.  TEST INFRASTRUCTURE ONLY: numpy / scipy
and tests/test_prune_model.py's restatement of the two filters; no GPU and no library.

The restatement is float32 in the kernel's order where the kernel's order is defined (the fma chains over a record's entries)
and takes the value LEAST favourable to the claims where it is not: ||a||^2 is summed by the wave in an order that depends on
where the hash put the terms, so the model takes the smallest sum the kernel's error analysis allows (the exact sum less
1e-6 of it) times the kernel's 1.00002f, and the hardware root (one ulp) as the correctly rounded one less an ulp.  Both
make the model leave EARLIER than the kernel can: what it never rejects early, the kernel does not either."""
import functools
import math

import numpy as np
import scipy.sparse as sp

from tests import test_prune_model as M

f32 = np.float32
REST_UNITS = (2, 3, 4, 6)          # SG_Q8_REST_UNIT (sg_internal.h)
REST_UNKNOWN = 255


def rest_fields(bq):
    """The four bytes K3 stores for a record of 8-bit values `bq` (ascending term order): the least integer r with
    r * r >= sum of bq_e^2 over e >= 4 u, cut at 255 = unknown; all unknown for a row without a copy."""
    bq = [int(q) for q in bq]
    if len(bq) > M.Q8_MAX_ENTRIES:
        return (REST_UNKNOWN,) * 4
    out = []
    for u in REST_UNITS:
        s = sum(q * q for q in bq[4 * u:])
        r = math.isqrt(s)
        r += r * r < s
        out.append(min(r, REST_UNKNOWN))
    return tuple(out)


def _fma(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def early_exit(a_idx, a_val, b_idx, bq, thr, norm_up, fields=None):
    """-> (the unit behind which the lane stops reading, or None: it reads the record to its end; U as far as it got)."""
    n = len(b_idx)
    a32 = np.asarray(a_val).astype(f32)
    a = dict(zip(np.asarray(a_idx).tolist(), a32.tolist()))
    if n > M.Q8_MAX_ENTRIES:
        return None, f32(0)
    fields = rest_fields(bq) if fields is None else fields
    units = (n + 7) >> 2
    na2 = f32(f32(np.nextafter(f32((a32.astype(np.float64) ** 2).sum() * (1.0 - 1e-6)), f32(0))) * f32(1.00002))
    bar = M.q8_bar(thr, norm_up)
    bar_lo = f32(bar * f32(0.99998))
    ub = matched = f32(0)
    ks, qs = np.asarray(b_idx).tolist(), [int(q) for q in bq]
    for u in range(1, units):
        for e in range(4 * u - 4, min(4 * u, n)):
            av = a.get(ks[e], 0.0)
            ub = _fma(av, qs[e], ub)
        for e in range(4 * u - 4, min(4 * u, n)):
            av = a.get(ks[e], 0.0)
            matched = _fma(av, av, matched)
        if u in REST_UNITS and u + 1 < units:
            r8 = fields[REST_UNITS.index(u)]
            root = np.sqrt(np.maximum(f32(na2 - matched), f32(1e-30)), dtype=f32)
            a_rest = np.nextafter(root, f32(0))
            if r8 != REST_UNKNOWN and _fma(a_rest, r8, ub) < bar_lo:
                return u, ub
    return None, ub


def row(m, i):
    return m.indices[m.indptr[i]:m.indptr[i + 1]], m.data[m.indptr[i]:m.indptr[i + 1]]


# ---------------------------------------------------------------------------------------------------- the built matrix
# What makes a pair a candidate of the FIRST filter without being a match: the first filter knows a candidate's frequent terms
# (those in 0.5 % of the rows and more) only by their norm.  A left row that keeps much of its mass on frequent terms and a
# candidate that does the same on OTHER frequent terms, with one or two rare terms in common, is such a pair -- and the second
# filter, which looks the terms up, throws it out.  Where it can tell depends on how many entries the candidate has and where
# in the term order the common ones lie: candidates of 1 .. 60 entries (and a few beyond 60: no copy) with the common terms
# in front, in the middle or at the end leave at every boundary, or at none.
N_COLS = 20000
N_FREQUENT = 96            # terms 0, 200, 400 ... : spread over the term order
N_FILLER = 8600            # with the families: more than two tiles of 4096 index rows
ANCHORS = 12               # rows 0 .. 11 of the families: 6 of 24 .. 40 terms, 4 wide (65 .. 128), 2 of norm 1/2
PER_ANCHOR = 140
SEED = 17
THRESHOLDS = (0.8, 0.35)   # the second for the left rows of norm 1/2, whose scores end at 0.5


@functools.lru_cache(maxsize=None)
def built(dtype):
    """-> (matrix, anchor rows): the anchors are the left rows the cases are about."""
    rng = np.random.default_rng(SEED)
    frequent = np.arange(N_FREQUENT) * 200
    rare = np.setdiff1d(np.arange(N_COLS), frequent)
    rows = []

    def make(terms, weights, norm=1.0):
        terms, weights = np.asarray(terms), np.asarray(weights, np.float64)
        order = np.argsort(terms)
        assert len(np.unique(terms)) == len(terms)
        return terms[order], weights[order] / np.sqrt((weights ** 2).sum()) * norm

    anchors = []
    for a in range(ANCHORS):
        wide = 6 <= a < 10
        n_rare = int(rng.integers(70, 110)) if wide else int(rng.integers(8, 16))
        n_freq = int(rng.integers(12, 18))
        a_rare = rng.choice(rare, n_rare, replace=False)
        a_freq = rng.choice(frequent[:N_FREQUENT // 2], n_freq, replace=False)      # the anchors' frequent terms: the first half
        # squared mass 0.5 on the frequent terms (inside the first filter's budget (0.8 - delta)^2), 0.5 on the rare ones, a
        # few of which are heavy: one in common is worth 0.2 .. 0.35 of a score
        w_rare = rng.random(n_rare) * 0.3 + 0.05
        w_rare[:4] = 1.0
        w = np.concatenate([w_rare / np.sqrt((w_rare ** 2).sum()), np.full(n_freq, 1.0 / math.sqrt(n_freq))])
        anchors.append((a_rare, a_freq))
        rows.append(make(np.concatenate([a_rare, a_freq]), w, 0.5 if a >= 10 else 1.0))
    for a, (a_rare, a_freq) in enumerate(anchors):
        for c in range(PER_ANCHOR):
            n = 1 + (c * 7 + a) % 66                      # 1 .. 66 entries: every length of a record, and rows without a copy
            n_common = min(n, int(rng.integers(1, 4)))
            common = rng.choice(a_rare[:4], min(n_common, 4), replace=False)
            n_freq = min(n - len(common), int(rng.integers(6, 30)))
            other = frequent[N_FREQUENT // 2:] if c % 4 else frequent                # every fourth may share frequent terms too
            c_freq = rng.choice(other, n_freq, replace=False)
            private = rng.choice(np.setdiff1d(rare, a_rare), n - len(common) - n_freq, replace=False)
            w = np.concatenate([np.full(len(common), rng.random() * 0.5 + 0.3),
                                np.full(n_freq, 0.9 / math.sqrt(max(n_freq, 1))), rng.random(len(private)) * 0.2 + 0.02])
            rows.append(make(np.concatenate([common, c_freq, private]), w))
    for _ in range(N_FILLER):                                                        # what makes the frequent terms frequent
        n_freq = int(rng.integers(4, 10))
        terms = np.concatenate([rng.choice(frequent, n_freq, replace=False), rng.choice(rare, 16 - n_freq, replace=False)])
        rows.append(make(terms, rng.random(16) + 0.1))
    shuffle = rng.permutation(len(rows))
    where = np.argsort(shuffle)                           # row r of the list sits at where[r]
    rows = [rows[i] for i in shuffle]
    indptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(t) for t, _ in rows], out=indptr[1:])
    m = sp.csr_matrix((np.concatenate([v for _, v in rows]).astype(dtype), np.concatenate([t for t, _ in rows]).astype(np.int32), indptr),
                      shape=(len(rows), N_COLS))
    m.has_sorted_indices = True
    return m, tuple(int(x) for x in where[:ANCHORS])


def norm_up_of(m):
    return np.nextafter(f32(np.sqrt(f32(np.asarray(m.multiply(m).sum(axis=1)).max())) * f32(1.000001)), f32(2))


@functools.lru_cache(maxsize=None)
def built_candidates(dtype, thr=0.8, delta=0.03, freq=0.005):
    """{anchor: [(candidate j, its entries, the unit it leaves behind or None)]} by the restated first filter."""
    m, anchors = built(dtype)
    mt = m.T.tocsr()
    mt.sort_indices()
    norm_up = norm_up_of(m)
    freq_min = max(1, int(freq * m.shape[0]))
    fq, bq, post = M.quantise_right_stream(m, mt, freq_min, norm_up, tile=4096)
    rng = np.random.default_rng(5)
    out = {}
    for i in anchors:
        ai, av = row(m, i)
        # (a wide row, 65 .. 128 terms, is staged two terms a lane by a launch of its own: the rule restated here is the same)
        rec, _ = M.records_of_row_stream(ai, av.astype(f32), mt.indptr, mt.indices, bq, fq, post, thr, delta, norm_up, freq_min, rng, tile=4096)
        if rec is None:
            continue
        found = []
        for j in np.unique(rec):
            if j == i:
                continue
            bi, bv = row(m, int(j))
            u, _ = early_exit(ai, av, bi, M.q8_quantise(bv, norm_up), m.dtype.type(thr), norm_up)
            found.append((int(j), len(bi), u))
        out[i] = found
    return out
