"""GPU tests of pair similarities: sg_csr_pairs_dot through ``Context.pairs_dot`` on every case of tests/_pair_cases.py, its
refusals (each followed by a good call, the output buffer untouched), the promise -- every (row, column, score) the top-n
multiply reports is reproduced bit for bit, by the binding and through the public API -- and ``Corpus.pair_similarities`` on a
corpus as it is fitted, grows, forgets, is compacted and refitted, against sklearn's fixed-vocabulary matrices.  No tolerance
anywhere: dtype, shape and bit patterns."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import string_grouper_amd as sga
import string_grouper_amd.engine as E
from string_grouper_amd import _native as N
from string_grouper_amd.synth import synth_names
from string_grouper_amd.vectorizer import HipTfidfVectorizer
from tests import _corpus_refit_oracle as R
from tests import _pair_cases as C
from tests._corpus_oracle import fixed_corpus_matrices

pytestmark = pytest.mark.gpu
DTYPES = C.DTYPES


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


def upload_raw(ctx, m: sp.csr_matrix) -> N.Csr:
    """sg_csr_from_host on the arrays as they are: Context.csr_from_scipy would sort the rows first."""
    indptr = np.ascontiguousarray(m.indptr, np.int64)
    indices = np.ascontiguousarray(m.indices, np.int32)
    data = np.ascontiguousarray(m.data)
    out = ctypes.c_void_p()
    N.check(N.lib().sg_csr_from_host(ctx.h, m.shape[0], m.shape[1], N._ptr(indptr), N._ptr(indices), N._ptr(data),
                                     N.np_dtype_code(data.dtype), ctypes.byref(out)))
    return N.Csr(ctx, out)


class Uploaded:
    """The matrices of the cases on the device, each once; A is B on the host: one handle."""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, {}

    def of(self, m) -> N.Csr:
        if id(m) not in self.held:
            self.held[id(m)] = (m, self.ctx.csr_from_scipy(m))
        return self.held[id(m)][1]

    def free(self):
        for _, h in self.held.values():
            h.free()


# ------------------------------------------------------------------------------------------ every case, both dtypes
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_case_equals_the_statement(ctx, dtype):
    up = Uploaded(ctx)
    try:
        for name, (A, B, left, right) in C.cases(dtype).items():
            got = ctx.pairs_dot(up.of(A), up.of(B), left, right)
            assert C.same_bits(got, C.expected(dtype, name)), name
        assert len(up.held) < 2 * len(C.cases(dtype))                       # (self-joins went in as ONE handle)
        # the same call three times, another case in between
        A, B, left, right = C.cases(dtype)["lengths_two_sided"]
        A2, B2, left2, right2 = C.cases(dtype)["arithmetic"]
        for _ in range(3):
            assert C.same_bits(ctx.pairs_dot(up.of(A), up.of(B), left, right), C.expected(dtype, "lengths_two_sided"))
            assert C.same_bits(ctx.pairs_dot(up.of(A2), up.of(B2), left2, right2), C.expected(dtype, "arithmetic"))
        # a view (absolute row pointers into the parent's arrays) on either side
        lo = 3
        view = up.of(A).row_block(lo, A.shape[0])
        keep = left >= lo
        assert C.same_bits(ctx.pairs_dot(view, up.of(B), left[keep] - lo, right[keep]), C.expected(dtype, "lengths_two_sided")[keep])
        view.free()
    finally:
        up.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_inf_and_negative_values_flow_through(ctx, dtype):
    A, B, left, right = C.special_values_case(dtype)
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    want = C.ref_pairs_dot(A, B, left, right)
    assert np.isnan(want).any() and np.isinf(want).any() and (want < 0).any()
    got = ctx.pairs_dot(a, b, left, right)
    nan = np.isnan(want)
    assert got.dtype == want.dtype and np.array_equal(np.isnan(got), nan) and np.array_equal(C.bits(got[~nan]), C.bits(want[~nan]))
    a.free()
    b.free()


def test_no_pairs_is_ok_and_reads_nothing(ctx):
    A, B, _, _ = C.cases(np.float32)["structured"]
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    assert N.lib().sg_csr_pairs_dot(ctx.h, a.h, b.h, None, None, 0, None) == N.SG_OK
    got = ctx.pairs_dot(a, b, [], [])
    assert got.dtype == np.float32 and got.shape == (0,)
    a.free()
    b.free()


# ------------------------------------------------------------------------------------------ refusals
def _refused(ctx, a, b, left, right, dtype, word):
    out = np.full(len(left), 7.5, dtype)
    with pytest.raises(ValueError, match=word):
        ctx.pairs_dot(a, b, left, right, out=out)
    assert np.all(out == 7.5), "a refused call wrote to the output buffer"


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_index_outside_its_matrix_is_refused_and_the_next_call_works(ctx, dtype):
    A, B, left, right = C.cases(dtype)["lengths_two_sided"]
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    want = C.expected(dtype, "lengths_two_sided")
    for bad in (-1, A.shape[0]):
        for at in (0, len(left) // 2, len(left) - 1):
            l2 = left.copy()
            l2[at] = bad
            _refused(ctx, a, b, l2, right, dtype, "left index")
            assert C.same_bits(ctx.pairs_dot(a, b, left, right), want)
            r2 = right.copy()
            r2[at] = bad
            _refused(ctx, a, b, left, r2, dtype, "right index")
            out = np.full(len(left) + 3, 7.5, dtype)
            assert C.same_bits(ctx.pairs_dot(a, b, left, right, out=out), want) and np.all(out[len(left):] == 7.5)
    l2, r2 = left.copy(), right.copy()
    l2[1], r2[5] = -1, B.shape[0]
    _refused(ctx, a, b, l2, r2, dtype, "left index.*right index")               # one bit a cause: both are named
    a.free()
    b.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_unsorted_row_is_refused_only_when_a_pair_reads_it(ctx, dtype):
    A, B, left, right = C.cases(dtype)["structured"]
    want = C.expected(dtype, "structured")
    lengths = np.diff(A.indptr)
    short, long_ = int(np.flatnonzero(lengths == 2 * C.LANES + 1)[0]), int(np.argmax(lengths))
    assert lengths[long_] > 1024
    for step in ("descending", "repeated"):
        for row in (short, long_):
            bad = A.copy()
            lo, hi = bad.indptr[row], bad.indptr[row + 1]
            at = lo + (hi - lo) // 2 if row == long_ else hi - 2                # deep inside the long row; the short row's last step
            if step == "descending":
                bad.indices[[at, at + 1]] = bad.indices[[at + 1, at]]
            else:
                bad.indices[at + 1] = bad.indices[at]
            sorted_side, bad_side = ctx.csr_from_scipy(B), upload_raw(ctx, bad)
            reads = left == row
            assert reads.any() and not reads.all()
            _refused(ctx, bad_side, sorted_side, left, right, dtype, "row of A .* not sorted")
            # the same matrix where no pair names that row: served
            assert C.same_bits(ctx.pairs_dot(bad_side, sorted_side, left[~reads], right[~reads]), want[~reads])
            # ... and on the right-hand side
            want_t = C.ref_pairs_dot(B, A, right, left)
            _refused(ctx, sorted_side, bad_side, right, left, dtype, "row of B .* not sorted")
            assert C.same_bits(ctx.pairs_dot(sorted_side, bad_side, right[~reads], left[~reads]), want_t[~reads])
            sorted_side.free()
            bad_side.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_differing_shapes_and_value_types_are_refused_on_the_host(ctx, dtype):
    A, B, left, right = C.cases(dtype)["structured"]
    other = np.float64 if dtype == np.float32 else np.float32
    a, b = ctx.csr_from_scipy(A), ctx.csr_from_scipy(B)
    wider = ctx.csr_from_scipy(sp.csr_matrix((B.data, B.indices, B.indptr), shape=(B.shape[0], B.shape[1] + 1)))
    other_type = ctx.csr_from_scipy(B.astype(other))
    _refused(ctx, a, wider, left, right, dtype, "differ in shape")
    assert C.same_bits(ctx.pairs_dot(a, b, left, right), C.expected(dtype, "structured"))
    _refused(ctx, a, other_type, left, right, dtype, "differ in value type")
    assert C.same_bits(ctx.pairs_dot(a, b, left, right), C.expected(dtype, "structured"))
    with pytest.raises(ValueError, match="left has"):
        ctx.pairs_dot(a, b, left, right[:-1])
    for h in (a, b, wider, other_type):
        h.free()


# ------------------------------------------------------------------------------------------ the promise
N_NAMES = 2000
# (min_similarity, max_n_matches, switches, what the multiply's counters must say): the pruned kernel, and the exact one
MULTIPLIES = [(0.8, 10, {}, lambda st: st["prune_rows"] > 0),
              (0.4, 100, {"SG_PRUNE": "0"}, lambda st: st["prune_rows"] == 0)]


def _names():
    master = synth_names(N_NAMES, seed=11)
    dupes = synth_names(700, seed=12, perturb_of=master, perturb_frac=0.6)
    return master, dupes


@pytest.mark.parametrize("thr,top_n,switches,took", MULTIPLIES, ids=["pruned-0.8-top10", "exact-0.4-top100"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_entry_of_the_multiply_is_reproduced_bit_for_bit(ctx, dtype, thr, top_n, switches, took):
    master, dupes = _names()
    vec = HipTfidfVectorizer(dtype=dtype, ctx=ctx)
    cols = [vec.prepare(pd.Series(master)), vec.prepare(pd.Series(dupes))]
    vec.fit_prepared(cols)
    with N.Scope() as s:
        a, b = s.own(vec.transform_prepared(cols[0])), s.own(vec.transform_prepared(cols[1]))
        for name, value in switches.items():
            ctx.set_option(name, value)
        for left_m, right_m in ((a, a), (a, b), (b, a)):                        # self-join; two-sided, of different lengths
            post = s.own(ctx.postings_build(right_m))
            res = s.own(ctx.spgemm_topn(left_m, post, top_n, thr, True))
            assert took(ctx.stats()), ctx.stats()
            Cm = res.to_scipy().tocoo()
            assert Cm.nnz > 100 and Cm.data.dtype == dtype
            got = ctx.pairs_dot(left_m, right_m, Cm.row, Cm.col)
            assert C.same_bits(got, np.ascontiguousarray(Cm.data))
    vec.free()


@pytest.mark.parametrize("thr,top_n", [(0.8, 10), (0.4, 100)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_public_function_gives_the_similarities_of_match_strings_frames(eng, dtype, thr, top_n):
    master, dupes = _names()
    master, dupes = pd.Series(master), pd.Series(dupes)
    kw = dict(min_similarity=thr, max_n_matches=top_n, tfidf_matrix_dtype=dtype)
    frame = sga.match_strings(master, **kw)
    off = frame[frame.left_index != frame.right_index]                          # (the frames set the diagonal to 1)
    assert len(off) > 100
    got = sga.pair_similarities(master, off.left_index.to_numpy(), off.right_index.to_numpy(), **kw)
    assert got.dtype == dtype and C.same_bits(got.astype(np.float64), off.similarity.to_numpy())
    frame = sga.match_strings(master, dupes, **kw)
    assert len(frame) > 100
    got = sga.pair_similarities(master, frame.left_index.to_numpy(), frame.right_index.to_numpy(), duplicates=dupes, **kw)
    assert got.dtype == dtype and C.same_bits(got.astype(np.float64), frame.similarity.to_numpy())


# ------------------------------------------------------------------------------------------ Corpus.pair_similarities
def _pairs(rng, n_left, n_right, count=300):
    """Random pairs, neighbours (similar names sit side by side in no particular order here, so: a row with itself, too) and
    negative positions."""
    left, right = rng.integers(-n_left, n_left, count), rng.integers(-n_right, n_right, count)
    left[:20] = right[:20] = np.arange(20) % min(n_left, n_right)
    return left, right


def _held(corpus, fit_on, current, left, right, dtype, duplicates=None, after_refit=False):
    """corpus.pair_similarities against the statement on sklearn's matrices, the vocabulary fixed to the original list's."""
    sets = [list(current)] + ([] if duplicates is None else [list(duplicates)])
    if after_refit:
        mats, _, _ = R.fixed_vocabulary_matrices(list(fit_on), list(current), sets, dtype=dtype)
    else:
        mats, _, _ = fixed_corpus_matrices(list(fit_on), sets, dtype=dtype)
    a = mats[0].tocsr()
    b = a if duplicates is None else mats[1].tocsr()
    want = C.ref_pairs_dot(a, b, left % a.shape[0], right % b.shape[0])
    got = corpus.pair_similarities(left, right) if duplicates is None else corpus.pair_similarities(left, right, duplicates=duplicates)
    assert C.same_bits(got, want)
    assert np.count_nonzero(got) > 20
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_corpus_pair_similarities_as_the_corpus_lives(eng, dtype):
    rng = np.random.default_rng(5)
    original = pd.Series(synth_names(N_NAMES, seed=21))
    extra = pd.Series(synth_names(20, seed=22, perturb_of=list(original), perturb_frac=0.7))
    batch = pd.Series(synth_names(150, seed=23, perturb_of=list(original), perturb_frac=0.5))
    with sga.Corpus(original, tfidf_matrix_dtype=dtype) as corpus:
        n = len(original)
        _held(corpus, original, original, *_pairs(rng, n, n), dtype)                               # fresh
        _held(corpus, original, original, *_pairs(rng, n, len(batch)), dtype, duplicates=batch)    # with duplicates
        assert corpus.stats["transforms"] == 1
        corpus.append(extra)                                                                       # rows wait in the second segment
        assert corpus.stats["segments"] == 2
        grown = pd.concat([original, extra])
        left, right = _pairs(rng, len(grown), len(grown))
        left[20:40], right[20:40] = np.arange(n, n + 20), rng.integers(0, n, 20)                   # new x old
        left[40:60], right[40:60] = rng.integers(0, n, 20), np.arange(n, n + 20)                   # old x new
        left[60:80], right[60:80] = np.arange(n, n + 20), np.arange(n, n + 20)[::-1]               # new x new
        _held(corpus, original, grown, left, right, dtype)
        assert corpus.stats["segments"] == 2 and corpus.stats["compactions"] == 0
        drop = [0, 5, 6, n - 1, n, n + 7]                                                          # removed rows pending
        corpus.remove(drop)
        keep = np.ones(len(grown), bool)
        keep[drop] = False
        shorter = grown[keep]
        before = corpus.stats
        assert before["dead_rows"] == len(drop) and before["compactions"] == 0
        m = len(shorter)
        left, right = _pairs(rng, m, m)
        left[20:40], right[20:40] = np.arange(20), np.arange(m - 20, m)                            # around the dead rows
        _held(corpus, original, shorter, left, right, dtype)
        _held(corpus, original, shorter, *_pairs(rng, m, len(batch)), dtype, duplicates=batch)
        after = corpus.stats
        assert after["compactions"] == before["compactions"] and after["dead_rows"] == before["dead_rows"]
        assert after["segments"] == 2 and after["tokenisations"] == 1
        with pytest.raises(IndexError):
            corpus.pair_similarities([m], [0])
        corpus.compact()                                                                           # after compact()
        assert corpus.stats["compactions"] == 1 and corpus.stats["dead_rows"] == 0 and corpus.stats["segments"] == 1
        stale = _held(corpus, original, shorter, left, right, dtype)
        corpus.refit_idf()                                                                         # after refit_idf()
        fresh = _held(corpus, original, shorter, left, right, dtype, after_refit=True)
        assert not np.array_equal(C.bits(fresh), C.bits(stale)), "the refit changed no score"
        _held(corpus, original, shorter, *_pairs(rng, m, len(batch)), dtype, duplicates=batch, after_refit=True)
        st = corpus.stats
        assert st["tokenisations"] == 1 and st["pair_calls"] == 8 and st["pairs_scored"] == 8 * 300


@pytest.mark.parametrize("dtype", DTYPES)
def test_corpus_pairs_are_the_bits_of_the_corpus_own_match_strings(eng, dtype):
    names = pd.Series(synth_names(N_NAMES, seed=31))
    with sga.Corpus(names, tfidf_matrix_dtype=dtype) as corpus:
        frame = corpus.match_strings(corpus.master, min_similarity=0.6, max_n_matches=20)
        off = frame[frame.left_index != frame.right_index]
        assert len(off) > 100
        got = corpus.pair_similarities(off.left_index.to_numpy(), off.right_index.to_numpy())
        assert C.same_bits(got.astype(np.float64), off.similarity.to_numpy())
