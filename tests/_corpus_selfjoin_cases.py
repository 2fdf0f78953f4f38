"""A self-join that is kept across append and remove (Corpus.keep_self_join), restated with numpy and scipy, the inputs built
to bite it, and the corpus engine double that keeps one.  TEST INFRASTRUCTURE ONLY.

A result is a list with one (columns, scores) pair of arrays per row, ordered as the multiply orders a row: score descending,
then column ascending.  The definition every update is held to is the port's whole self-join of the current rows,
``sp_matmul_topn_port(M, M.T, top_n, threshold)`` (oracle/port.py)."""
import numpy as np
import scipy.sparse as sp

from oracle import port as P
from tests._corpus_oracle import CorpusHostMatrix
from tests._corpus_remove_oracle import RemoveCorpusOracleEngine


# ------------------------------------------------------------------------------------------ results as lists of rows
def rows_of(C: sp.csr_matrix):
    """The rows of a CSR result in the order they are stored (no scipy operation that would sort them)."""
    ip = np.asarray(C.indptr, np.int64)
    return [(np.asarray(C.indices[ip[i]:ip[i + 1]], np.int32).copy(), np.asarray(C.data[ip[i]:ip[i + 1]]).copy())
            for i in range(C.shape[0])]


def csr_of(rows, n_cols, dtype) -> sp.csr_matrix:
    counts = np.array([len(c) for c, _ in rows], np.int64)
    indptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(counts, out=indptr[1:])
    cols = np.concatenate([c for c, _ in rows]).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    vals = np.concatenate([v for _, v in rows]).astype(dtype) if indptr[-1] else np.zeros(0, dtype)
    return sp.csr_matrix((vals, cols, indptr.astype(np.int32)), shape=(len(rows), n_cols))


def product(A, B, top_n, threshold):
    """sp_matmul_topn(A, B.T, top_n, threshold) as rows."""
    if A.shape[0] == 0:
        return []
    if B.shape[0] == 0:
        return [(np.zeros(0, np.int32), np.zeros(0, A.dtype))] * A.shape[0]
    return rows_of(P.sp_matmul_topn_port(sp.csr_matrix(A), sp.csr_matrix(B).T, top_n, threshold, True, 4))


def same_rows(got, want) -> bool:
    return len(got) == len(want) and all(
        np.array_equal(gc, wc) and gv.dtype == wv.dtype and np.array_equal(gv, wv) for (gc, gv), (wc, wv) in zip(got, want))


def differing_rows(got, want):
    assert len(got) == len(want)
    return {i for i, ((gc, gv), (wc, wv)) in enumerate(zip(got, want)) if not (np.array_equal(gc, wc) and np.array_equal(gv, wv))}


# ------------------------------------------------------------------------------------------ the device operations, restated
def zip_rows(parts, col_offsets, top_n):
    """sg_topn_zip (K5): per row the entries of every part, its columns offset, by score descending then column ascending,
    cut at top_n."""
    out = []
    for row in zip(*parts):
        cols = np.concatenate([c.astype(np.int64) + off for (c, _), off in zip(row, col_offsets)])
        vals = np.concatenate([v for _, v in row])
        order = np.lexsort((cols, -vals.astype(np.float64)))[:top_n]
        out.append((cols[order].astype(np.int32), vals[order]))
    return out


def concat_rows(parts):
    """sg_topn_concat_rows: scipy's vstack of result blocks."""
    return [row for part in parts for row in part]


def forget(rows, dead, top_n):
    """sg_topn_forget: C[keep][:, keep], and -- ascending, in the new numbering -- the surviving rows that held top_n
    entries and hold fewer now."""
    dead = np.asarray(dead, np.int64)
    gone = np.zeros(len(rows), bool)
    gone[dead] = True
    out, short = [], []
    for i, (c, v) in enumerate(rows):
        if gone[i]:
            continue
        live = ~np.isin(c, dead)
        if len(c) >= top_n and int(live.sum()) < top_n:
            short.append(len(out))
        out.append(((c[live] - np.searchsorted(dead, c[live])).astype(np.int32), v[live]))
    return out, np.array(short, np.int64)


def rows_that_lost_an_entry(rows, dead):
    """The other rule one might refill by: every surviving row that named a removed column, full or not (new numbering)."""
    dead = np.asarray(dead, np.int64)
    keep = np.setdiff1d(np.arange(len(rows)), dead)
    return np.array([k for k, i in enumerate(keep) if np.isin(rows[i][0], dead).any()], np.int64)


def put_rows(rows, which, src):
    """sg_topn_put_rows: row which[k] becomes row k of src."""
    assert len(which) == len(src) and len(set(int(w) for w in which)) == len(which)
    out = list(rows)
    for k, w in enumerate(which):
        out[int(w)] = src[k]
    return out


# ------------------------------------------------------------------------------------------ the two updates
class KeptSelfJoin:
    """The kept result of a corpus whose rows are the scipy matrix ``M``, by the two updates of engine.corpus_append and
    engine.corpus_remove.  ``refill``: 'rule' (the rows sg_topn_forget returns), 'none' (the refill left out) or 'losers'
    (every row that lost an entry).  ``refilled`` lists the rows of every remove."""

    def __init__(self, M, top_n, threshold, refill="rule"):
        self.M = sp.csr_matrix(M)
        self.top_n, self.threshold, self.refill = int(top_n), float(threshold), refill
        self.rows = product(self.M, self.M, self.top_n, self.threshold)
        self.refilled = []

    def append(self, new):
        new = sp.csr_matrix(new)
        n_old = self.M.shape[0]
        over_new = product(self.M, new, self.top_n, self.threshold)               # before the rows join
        old = zip_rows([self.rows, over_new], [0, n_old], self.top_n)
        self.M = sp.vstack([self.M, new], format="csr", dtype=self.M.dtype)
        self.rows = concat_rows([old, product(new, self.M, self.top_n, self.threshold)])

    def remove(self, dead):
        dead = np.asarray(sorted(set(int(d) for d in dead)), np.int64)
        before = self.rows
        self.rows, short = forget(before, dead, self.top_n)
        keep = np.ones(self.M.shape[0], bool)
        keep[dead] = False
        self.M = self.M[keep]
        which = {"rule": short, "none": np.zeros(0, np.int64), "losers": rows_that_lost_an_entry(before, dead)}[self.refill]
        if len(which):
            self.rows = put_rows(self.rows, which, product(self.M[which], self.M, self.top_n, self.threshold))
        self.refilled.append(which)
        return which

    def whole(self):
        """The definition: the port's self-join of the current rows."""
        return product(self.M, self.M, self.top_n, self.threshold)


# ------------------------------------------------------------------------------------------ inputs built to bite
def unit_rows(groups, n_cols, dtype):
    """One row per entry of ``groups``: rows of one group are identical (similarity exactly 1), rows of different groups
    share nothing.  Group g owns the columns 2 g and 2 g + 1; (0.6, 0.8) has norm 1 in both value types' arithmetic."""
    n = len(groups)
    indptr = np.arange(0, 2 * n + 1, 2)
    indices = np.array([[2 * g, 2 * g + 1] for g in groups], np.int32).reshape(-1)
    data = np.tile(np.array([0.6, 0.8], dtype), n)
    return sp.csr_matrix((data, indices, indptr), shape=(n, n_cols), dtype=dtype)


def near_rows(groups, n_cols, dtype, tilt):
    """Rows close to their group's (similarity below 1, above 0.9): another score in the same hub."""
    m = unit_rows(groups, n_cols, dtype).tolil()
    for i, g in enumerate(groups):
        m[i, 2 * g] = dtype(np.cos(tilt))
        m[i, 2 * g + 1] = dtype(np.sin(tilt))
    return m.tocsr().astype(dtype)


HUB, FULL, ONE_SHORT = 0, 1, 2          # groups of the built corpus: 40, 10 and 9 identical rows at top_n 10
BUILT_TOP_N = 10
BUILT_COLS = 64


def built_corpus(dtype):
    """A hub of 40 identical rows (top_n 10: every hub row names the ten lowest), a group that is exactly full (10 rows), one
    that is one short (9), pairs, singles and a row without entries, shuffled by a fixed pattern so that the hub's members
    lie all over the list.  Returns (matrix, group of every row; -1: no entries)."""
    groups = [HUB] * 40 + [FULL] * 10 + [ONE_SHORT] * 9 + [3, 3, 4, 4, 5, 6, 7]
    order = np.random.default_rng(12).permutation(len(groups))
    groups = [groups[i] for i in order]
    m = sp.vstack([unit_rows(groups, BUILT_COLS, dtype), sp.csr_matrix((1, BUILT_COLS), dtype=dtype)], format="csr", dtype=dtype)
    return m, np.array(groups + [-1])


def random_rows(rng, n, n_cols, dtype, pool=None):
    """Non-negative rows of norm ~1 with many exact duplicates (drawn from a small pool): ties everywhere."""
    if pool is None:
        pool = sp.random(max(n // 3, 4), n_cols, density=0.08, format="csr", random_state=rng, dtype=np.float64)
        pool.data = rng.integers(1, 9, pool.nnz).astype(np.float64)
        norms = np.sqrt(np.asarray(pool.multiply(pool).sum(axis=1))).ravel()
        norms[norms == 0] = 1.0
        pool = sp.diags(1.0 / norms) @ pool
    m = pool[rng.integers(0, pool.shape[0], n)].astype(dtype).tocsr()
    m.sort_indices()
    return m, pool


# ------------------------------------------------------------------------------------------ fixed-stride arrays (GPU tests)
def to_fixed(rows, stride, dtype, rubbish=True):
    """(cols, vals, counts) as a device result holds them; the slots behind a row's count hold rubbish."""
    cols = np.full((len(rows), stride), -7 if rubbish else 0, np.int32)
    vals = np.full((len(rows), stride), -1.0 if rubbish else 0.0, dtype)
    counts = np.zeros(len(rows), np.int32)
    for i, (c, v) in enumerate(rows):
        assert len(c) <= stride
        counts[i] = len(c)
        cols[i, :len(c)] = c
        vals[i, :len(c)] = v
    return cols, vals, counts


def from_fixed(cols, vals, counts):
    return [(cols[i, :n].copy(), vals[i, :n].copy()) for i, n in enumerate(counts)]


def random_result(rng, n_rows, stride, n_cols, dtype, must_name=()):
    """Rows as a multiply leaves them: distinct columns, few distinct scores, score descending then column ascending; every
    fifth row full, every seventh without entries, every third naming some of ``must_name``."""
    scores = (np.arange(1, 6) / 8.0).astype(dtype)
    out = []
    for i in range(n_rows):
        c = int(rng.integers(0, stride + 1))
        if i % 5 == 0:
            c = stride
        if i % 7 == 3:
            c = 0
        c = min(c, n_cols)
        chosen = rng.choice(n_cols, c, replace=False)
        if i % 3 == 1 and len(must_name) and c:
            k = min(c, len(must_name), 1 + i % 4)
            chosen = np.unique(np.concatenate([rng.choice(must_name, k, replace=False), chosen[k:]]))
        v = rng.choice(scores, len(chosen))
        order = np.lexsort((chosen, -v.astype(np.float64)))
        out.append((chosen[order].astype(np.int32), v[order]))
    return out


# ------------------------------------------------------------------------------------------ the engine double
class SelfJoinCorpusOracleEngine(RemoveCorpusOracleEngine):
    """The corpus double that keeps a self-join as HipEngine does: by the restatement above, served to a self-join of the
    corpus's current matrix whose two options equal the kept ones."""
    name = "oracle-corpus-selfjoin"

    def corpus_fit(self, *args, **kwargs):
        state = super().corpus_fit(*args, **kwargs)
        state.stats.update(self_join_full=0, self_join_served=0, self_join_append_updates=0, self_join_remove_updates=0,
                           self_join_rows_refilled=0)
        state.kept, state.kept_opts = None, None
        return state

    def corpus_keep_self_join(self, state, top_n, threshold):
        opts = (int(top_n), float(threshold))
        if state.kept_opts != opts:
            state.kept = None
        state.kept_opts = opts

    def corpus_drop_self_join(self, state):
        state.kept = state.kept_opts = None

    def corpus_free(self, state):
        state.kept = state.kept_opts = None
        super().corpus_free(state)

    def corpus_append(self, state, strings):
        if len(strings) and state.kept is not None:
            state.kept.append(state.vec.transform(list(strings)))
            state.stats["self_join_append_updates"] += 1
        super().corpus_append(state, strings)

    def corpus_remove(self, state, positions):
        if len(positions) and state.kept is not None:
            state.stats["self_join_rows_refilled"] += len(state.kept.remove(positions))
            state.stats["self_join_remove_updates"] += 1
        super().corpus_remove(state, positions)

    def topn_multiply(self, A, B, top_n, threshold):
        state = getattr(B, "corpus", None)
        if A is B and isinstance(B, CorpusHostMatrix) and B is state.matrix and state.kept_opts == (int(top_n), float(threshold)):
            if state.kept is None:
                state.kept = KeptSelfJoin(B.m, top_n, max(float(threshold), 0.0))
                state.stats["self_join_full"] += 1
            state.stats["self_join_served"] += 1
            return csr_of(state.kept.rows, B.m.shape[0], B.m.dtype)
        return super().topn_multiply(A, B, top_n, threshold)
