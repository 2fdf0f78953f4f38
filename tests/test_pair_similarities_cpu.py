"""CPU tests of pair similarities: the numpy statement of sg_csr_pairs_dot (tests/_pair_cases.py) held to scipy's product and
to sparse_dot_topn's port at every element, the wrong turns a kernel could take (each must change an answer on the cases),
the kernel's walk in plain Python held to the statement on every case, and the public methods -- ``Corpus.pair_similarities``
and ``string_grouper_amd.pair_similarities`` -- on the engine double of tests/_pair_oracle.py.  No GPU."""
import numpy as np
import pandas as pd
import pytest

import string_grouper
import string_grouper_amd as sga
import string_grouper_amd.engine as E
from oracle import port as P
from tests import _corpus_refit_oracle as R
from tests import _pair_cases as C
from tests._corpus_oracle import fixed_corpus_matrices
from tests._pair_oracle import PairCorpusOracleEngine
from tests.test_corpus_append_cpu import X1, X2
from tests.test_corpus_cpu import CORPUS, NEW

DTYPES = C.DTYPES


@pytest.fixture(autouse=True)
def _restore_engine():
    yield
    E.set_engine(None)


# ------------------------------------------------------------------------------------------ the statement and the cases
def test_the_cases_cover_what_the_kernel_deals_by():
    G = C.LANES
    assert {0, 1, G - 1, G, G + 1, 63, 64, 65} <= set(C.ROW_LENGTHS) and max(C.ROW_LENGTHS) > 1024
    names = set(C.cases(np.float32))
    for count in (1, C.WAVE_PAIRS - 1, C.WAVE_PAIRS, C.WAVE_PAIRS + 1, C.BLOCK_PAIRS - 1, C.BLOCK_PAIRS, C.BLOCK_PAIRS + 1):
        assert f"count_{count}" in names
    A, B, left, right = C.cases(np.float32)["lengths_self"]
    assert A is B and np.any(left == right) and np.any(left != right)
    A, B, left, right = C.cases(np.float32)["same_pair_twice"]
    assert len(set(zip(left.tolist(), right.tolist()))) < len(left)
    A, B, left, right = C.cases(np.float32)["hub_row"]
    assert len(set(right.tolist())) == 1 and len(set(left.tolist())) == len(C.ROW_LENGTHS)
    for dtype in DTYPES:
        for name, (A, B, left, right) in C.cases(dtype).items():
            assert A.dtype == dtype and B.dtype == dtype and len(left) == len(right) > 0, name
            assert A.shape[1] == B.shape[1] and left.max() < A.shape[0] and right.max() < B.shape[0], name
            assert C.expected(dtype, name).dtype == dtype and len(C.expected(dtype, name)) == len(left), name


def test_the_structured_case_places_the_common_columns_as_it_says():
    A, B, left, right = C.cases(np.float64)["structured"]
    common = [np.intersect1d(C._row(A, i)[0], C._row(B, j)[0]) for i, j in zip(left, right)]
    first_of_a = [len(c) and c[0] == C._row(A, i)[0][0] for c, i in zip(common, left)]
    last_of_a = [len(c) and c[-1] == C._row(A, i)[0][-1] for c, i in zip(common, left)]
    first_of_b = [len(c) and c[0] == C._row(B, j)[0][0] for c, j in zip(common, right)]
    last_of_b = [len(c) and c[-1] == C._row(B, j)[0][-1] for c, j in zip(common, right)]
    assert any(first_of_a) and any(last_of_a) and any(first_of_b) and any(last_of_b)
    assert any(a and b for a, b in zip(first_of_a, last_of_b)) and any(a and b for a, b in zip(last_of_a, first_of_b))
    assert any(len(c) == 0 for c in common)                                          # none common
    assert any(len(c) == len(C._row(A, i)[0]) > 1 for c, i in zip(common, left))     # all common
    interleaved = [len(c) == 0 and len(C._row(A, i)[0]) > 1 and C._row(A, i)[0][0] < C._row(B, j)[0][0] < C._row(A, i)[0][-1]
                   for c, i, j in zip(common, left, right)]
    assert any(interleaved)


@pytest.mark.parametrize("name", ["lengths_self", "lengths_two_sided", "structured", "arithmetic"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_statement_is_scipys_product_at_every_element(dtype, name):
    A, B, _, _ = C.cases(dtype)[name]
    dense = np.asarray((A @ B.T).toarray())
    assert dense.dtype == dtype
    ii, jj = [x.ravel() for x in np.meshgrid(np.arange(A.shape[0]), np.arange(B.shape[0]), indexing="ij")]
    got = C.ref_pairs_dot(A, B, ii, jj)
    assert C.same_bits(got, np.ascontiguousarray(dense[ii, jj]))
    assert np.count_nonzero(got) > len(got) // 8


@pytest.mark.parametrize("name", ["lengths_self", "lengths_two_sided", "structured", "arithmetic"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_statement_is_every_entry_the_port_keeps(dtype, name):
    A, B, _, _ = C.cases(dtype)[name]
    kept = P.sp_matmul_topn_port(A, B.T, B.shape[0], 0.0, True, 4).tocoo()
    assert kept.nnz > 0 and kept.data.dtype == dtype
    assert C.same_bits(C.ref_pairs_dot(A, B, kept.row, kept.col), np.ascontiguousarray(kept.data))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_case_through_the_kernels_walk_gives_the_statement(dtype):
    for name, (A, B, left, right) in C.cases(dtype).items():
        assert C.same_bits(C.walk_model(A, B, left, right), C.expected(dtype, name)), name
    A, B, left, right = C.special_values_case(dtype)
    want = C.ref_pairs_dot(A, B, left, right)
    assert C.same_bits(C.walk_model(A, B, left, right), want)
    assert np.isnan(want).any() and np.isinf(want).any() and (want < 0).any()


# ------------------------------------------------------------------------------------------ the arithmetic is pinned
# (a wider accumulator is a turn float32 alone can take: sums in double ARE the statement for float64)
WRONG_TURNS = [(d, v) for d in DTYPES for v in ("pairwise", "descending", "fma", "wide_accumulator", "from_first")
               if not (v == "wide_accumulator" and d == np.float64)]


@pytest.mark.parametrize("dtype,variant", WRONG_TURNS)
def test_every_wrong_turn_changes_an_answer_of_the_arithmetic_case(dtype, variant):
    A, B, left, right = C.cases(dtype)["arithmetic"]
    want, wrong = C.expected(dtype, "arithmetic"), C.wrong_pairs_dot(A, B, left, right, variant)
    differ = C.bits(want) != C.bits(wrong)
    assert differ.any(), f"{variant} gives the statement's bits on every pair: the case does not bite"
    if variant == "from_first":                   # the lone -0.0 (and the pair of them): +0.0 by the statement
        lone = [p for p in range(len(left)) if len(C._row(A, left[p])[0]) <= 2 and np.all(C._common(A, B, left[p], right[p])[1] == 0)]
        assert lone and all(differ[p] and want[p] == 0 and not np.signbit(want[p]) and np.signbit(wrong[p]) for p in lone)


@pytest.mark.parametrize("dtype", DTYPES)
def test_leaving_zero_products_out_cannot_show_on_its_own(dtype):
    """The accumulator starts at +0.0 and is never -0.0 afterwards (x + y = -0.0 only for x = y = -0.0), and x + (+-0.0) = x
    for every other x: a kernel that skips zero products gives the statement's bits, and these cases say so.  (K9 skips them AND
    starts from the first product that is left; of the two it is the start that shows: the test above.)"""
    for name in ("arithmetic", "structured"):
        A, B, left, right = C.cases(dtype)[name]
        assert C.same_bits(C.wrong_pairs_dot(A, B, left, right, "skip_zero"), C.expected(dtype, name))
    A, B, left, right = C.cases(dtype)["arithmetic"]
    zero_products = sum(int(np.count_nonzero((a * b) == 0)) for a, b in (C._common(A, B, i, j) for i, j in zip(left, right)))
    assert zero_products >= 5


# ------------------------------------------------------------------------------------------ the public methods on the double
def _corpus(**kwargs):
    eng = PairCorpusOracleEngine(use_port=True)
    E.set_engine(eng)
    return sga.Corpus(CORPUS, **kwargs), eng


def _want(fit_on, left_strings, right_strings, left, right, dtype):
    (a, b), _, _ = fixed_corpus_matrices(fit_on, [left_strings, right_strings], dtype=dtype)
    return C.ref_pairs_dot(a.tocsr(), b.tocsr(), left, right)


def test_the_new_names_are_the_amd_packages_alone():
    assert "pair_similarities" in sga.__all__ and callable(sga.pair_similarities) and hasattr(sga.Corpus, "pair_similarities")
    assert not hasattr(string_grouper, "pair_similarities") and not hasattr(string_grouper, "Corpus")


@pytest.mark.parametrize("dtype", DTYPES)
def test_positions_negative_ones_and_the_order_given(dtype):
    corpus, _ = _corpus(tfidf_matrix_dtype=dtype)
    n = len(CORPUS)
    left, right = [0, 1, n - 1, 3, 3, 0], [1, 0, 2, 3, 2, 1]
    want = _want(CORPUS, CORPUS, CORPUS, left, right, dtype)
    got = corpus.pair_similarities(left, right)
    assert C.same_bits(got, want) and got[0] > 0.3 and C.bits(got)[0] == C.bits(got)[5]
    for as_given in (np.array(left), np.array(left, np.int32), np.array(left, np.uint8), tuple(left), pd.Series(left)):
        assert C.same_bits(corpus.pair_similarities(as_given, right), want)
    assert C.same_bits(corpus.pair_similarities([-n, 1 - n, -1, 3 - n, 3, 0], [1, 0, 2 - n, -n + 3, 2, 1]), want)
    assert corpus.stats["pair_calls"] == 7 and corpus.stats["pairs_scored"] == 7 * len(left)
    assert corpus.stats["tokenisations"] == 1 and corpus.stats["transforms"] == 0


def test_refusals_of_the_host():
    corpus, eng = _corpus()
    n = len(CORPUS)
    for bad in ([True, False], np.array([True, False]), [0.0, 1.0], np.array([0.5, 1.0]), ["0", "1"], 3, True, None, [[0, 1]]):
        with pytest.raises(TypeError):
            corpus.pair_similarities(bad, [0, 1])
        with pytest.raises(TypeError):
            corpus.pair_similarities([0, 1], bad)
    with pytest.raises(ValueError, match="a pair needs one of each"):
        corpus.pair_similarities([0, 1, 2], [0, 1])
    for bad in (n, -n - 1, 2 ** 40):
        with pytest.raises(IndexError):
            corpus.pair_similarities([0, bad], [0, 1])
        with pytest.raises(IndexError):
            corpus.pair_similarities([0, 1], [bad, 1])
    with pytest.raises(IndexError):                              # right counts through `duplicates` when given
        corpus.pair_similarities([0], [len(NEW)], duplicates=NEW)
    with pytest.raises(TypeError):
        corpus.pair_similarities([0], [0], duplicates=pd.Series([1, 2]))
    assert eng.pair_calls == [] and corpus.stats["pair_calls"] == 0, "a refused call reached the engine"
    empty = corpus.pair_similarities([], [])
    assert empty.dtype == np.float64 and empty.shape == (0,)
    assert corpus.pair_similarities(np.zeros(0, np.int64), []).shape == (0,)
    assert corpus.pair_similarities([], [], duplicates=NEW).shape == (0,)
    assert eng.pair_calls == [] and corpus.stats["pair_calls"] == 0 and corpus.stats["transforms"] == 0, "no pairs: no device call"
    corpus.close()
    with pytest.raises(ValueError, match="closed"):
        corpus.pair_similarities([0], [1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_are_transformed_once_as_a_batch(dtype):
    corpus, eng = _corpus(tfidf_matrix_dtype=dtype)
    left, right = [0, 1, 4, 8, 11, 1], [0, 0, 2, 5, 6, 4]
    got = corpus.pair_similarities(left, right, duplicates=NEW)
    assert C.same_bits(got, _want(CORPUS, CORPUS, NEW, left, right, dtype)) and got[0] > 0.3
    assert corpus.stats["transforms"] == 1 and corpus.stats["pair_calls"] == 1 and corpus.stats["pairs_scored"] == 6
    assert eng.pair_calls == [(len(CORPUS), len(NEW), 6)]
    # the corpus's own Series as `duplicates`: the resident rows, nothing is transformed
    again = corpus.pair_similarities([0, 1], [1, 0], duplicates=corpus.master)
    assert C.same_bits(again, _want(CORPUS, CORPUS, CORPUS, [0, 1], [1, 0], dtype))
    assert corpus.stats["transforms"] == 1 and corpus.stats["tokenisations"] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_corpus_that_has_grown_forgotten_and_refitted(dtype):
    corpus, _ = _corpus(tfidf_matrix_dtype=dtype)
    corpus.append(X1)
    grown = pd.concat([CORPUS, X1])
    n = len(grown)
    left, right = [0, n - 3, n - 1, 1, -1], [n - 3, 1, 8, n - 1, -2]      # old x new, new x old, new x new
    norm = lambda v, m: [x % m for x in v]
    got = corpus.pair_similarities(left, right)
    assert C.same_bits(got, _want(CORPUS, grown, grown, norm(left, n), norm(right, n), dtype)) and got[0] > 0.3
    assert len(corpus.master) == n
    # rows leave: positions count through the shorter list
    before = dict(corpus.stats)
    drop = [1, 8, n - 2]
    corpus.remove(drop)
    keep = np.ones(n, bool)
    keep[drop] = False
    shorter = grown[keep]
    m = len(shorter)
    left, right = [0, 1, m - 1, 7, -1, 2], [m - 2, 0, 7, m - 1, 0, 2]
    got = corpus.pair_similarities(left, right)
    assert C.same_bits(got, _want(CORPUS, shorter, shorter, norm(left, m), norm(right, m), dtype))
    assert got[0] > 0.3                                                    # "Acme Corporation" x "Acme Corp Ltd", as before
    with pytest.raises(IndexError):
        corpus.pair_similarities([m], [0])
    assert corpus.stats["compactions"] == before["compactions"] and corpus.stats["tokenisations"] == 1
    # the idf follows the list: so do the scores
    corpus.append(X2)
    current = pd.concat([shorter, X2])
    k = len(current)
    left, right = [0, 1, k - 1, 3, k - 4], [m - 2, 0, 3, k - 1, 2]
    stale = corpus.pair_similarities(left, right)
    assert C.same_bits(stale, _want(CORPUS, current, current, left, right, dtype))
    corpus.refit_idf()
    (now,), _, _ = R.fixed_vocabulary_matrices(CORPUS, current, [current], dtype=dtype)
    fresh = corpus.pair_similarities(left, right)
    assert C.same_bits(fresh, C.ref_pairs_dot(now, now, left, right))
    assert not np.array_equal(C.bits(fresh), C.bits(stale)), "the refit changed no score"
    assert corpus.stats["tokenisations"] == 1 and corpus.stats["pair_calls"] == 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_module_level_function_fits_as_match_strings_does(dtype):
    eng = PairCorpusOracleEngine(use_port=True)
    E.set_engine(eng)
    kw = dict(tfidf_matrix_dtype=dtype, min_similarity=0.3)
    # self-join: every pair the frame reports, the diagonal left out, has the frame's similarity to the bit
    frame = sga.match_strings(CORPUS, **kw)
    off = frame[frame.left_index != frame.right_index]
    assert len(off) >= 8
    got = sga.pair_similarities(CORPUS, off.left_index.to_numpy(), off.right_index.to_numpy(), **kw)
    assert got.dtype == dtype and C.same_bits(got.astype(np.float64), off.similarity.to_numpy())
    # two-sided: the vectoriser is fitted on master + duplicates
    frame = sga.match_strings(CORPUS, NEW, **kw)
    assert len(frame) >= 4
    got = sga.pair_similarities(CORPUS, frame.left_index.to_numpy(), frame.right_index.to_numpy(), duplicates=NEW, **kw)
    assert C.same_bits(got.astype(np.float64), frame.similarity.to_numpy())
    assert eng.pair_calls == [(len(CORPUS), len(CORPUS), len(off)), (len(CORPUS), len(NEW), len(frame))]
    assert sga.pair_similarities(CORPUS, [], [], **kw).shape == (0,) and len(eng.pair_calls) == 2
    with pytest.raises(IndexError):
        sga.pair_similarities(CORPUS, [0], [len(NEW)], duplicates=NEW)
    with pytest.raises(ValueError):
        sga.pair_similarities(CORPUS, [0, 1], [0])
    with pytest.raises(TypeError):
        sga.pair_similarities(CORPUS, [0.5], [0])
    with pytest.raises(TypeError):
        sga.pair_similarities(CORPUS, [0], [0], no_such_option=1)


def test_the_distributed_engine_refuses():
    eng = E.DistributedHipEngine.__new__(E.DistributedHipEngine)
    with pytest.raises(NotImplementedError):
        eng.pairs_dot(None, None, [0], [0])
    with pytest.raises(NotImplementedError):
        eng.corpus_pairs(None, [0], [0])
