"""Every path of the vectoriser's host driver (sg_vectorize.hip: sg_vec_fit, sg_vec_fit_begin / sg_vec_fit_end, sg_vec_transform)
against sklearn, bit for bit -- vocabulary, idf and matrix: the df count in more than one pass (a vocabulary of more than
30 x 1024 columns, K2 through the dense table after a marks fit), the deferred long strings with two fitted columns of which
one has some and one has none, the counters form and the sorted vocabulary, the three sources of a transform's row pointers
(the fit's, a second sum for a fitted column, kept counts for any other column) and a matrix without non-zeros."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as O
from tests.test_parity_gpu import assert_csr_identical
from tests.test_postings_build_paths_gpu import _id, _options

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DF_PASS_COLUMNS = 30 * 1024      # columns one pass of the fit's df count takes (count_df_by_column)


def _vectoriser(ctx, dtype, **kw):
    from string_grouper_amd.vectorizer import HipTfidfVectorizer
    return HipTfidfVectorizer(dtype=dtype, ctx=ctx, **kw)


def list_r():
    """3 000 random strings of 40 characters over a-z0-9: 42 557 distinct 3-grams, two passes of the df count"""
    rng = np.random.default_rng(1)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz0123456789"))
    return ["".join(row) for row in letters[rng.integers(0, len(letters), (3000, 40))]]


def _texts():
    """texts of a given length made of name words, as test_vectoriser_strings_of_any_length makes them"""
    from string_grouper_amd.synth import synth_names
    rng = np.random.default_rng(3)
    words = synth_names(400, 9)

    def text(n_chars):
        out = []
        while sum(len(w) + 1 for w in out) < n_chars:
            out.append(words[int(rng.integers(len(words)))])
        return " ".join(out)[:n_chars]
    return text


class _Lists:
    """the lists of this file and sklearn's results on them -- computed once, never changed"""

    def __init__(self):
        from string_grouper_amd.synth import synth_names
        text = _texts()
        self.R = list_r()
        # N-short: names, an empty string, one shorter than an n-gram, one for the wave-per-string kernel's second stage
        self.N_short = list(synth_names(2000, 21)) + ["", "ab", text(300)]
        # strings of about TOK_CAP = 1024 characters, which the wave-per-string kernel still sorts in LDS (875 and 876
        # 3-grams once blanks and punctuation are deleted), and one for the last stage (4 288 3-grams)
        self.longs = [text(1023), text(1026), text(5000)]
        # ... and the two sides of the limit itself: 1 024 3-grams stay with the wave, 1 025 go to the last stage
        letters = "".join(ch for ch in text(1400) if ch.isalnum())
        self.longs += [letters[:1026], letters[:1027]]
        assert [len(O.ngrams(s)) for s in self.longs[-2:]] == [1024, 1025]
        self.N = self.N_short + self.longs
        self.master = self.N_short[:1500]
        self.duplicates = self.N_short[1500:] + self.longs
        # a column that was not fitted: n-grams the fit never saw, and a string for the last stage
        self.other = list(synth_names(300, 99)) + ["qzx0qzx1 jjq9", "0123456789" * 3, text(2000) + " zzqj", ""]
        self._want = {}

    def want(self, fit, sets, dtype, **kw):
        """(matrices of `sets`, vocabulary, idf) of sklearn fitted on the list(s) named by `fit`; lists are named by attribute"""
        key = (fit, sets, np.dtype(dtype).str, tuple(sorted(kw.items())))
        if key not in self._want:
            fit_strings = [s for name in fit for s in getattr(self, name)]
            mats, vocab, idf = O.tfidf_sklearn(fit_strings, [self._set(s) for s in sets], dtype=dtype, **kw)
            self._want[key] = ([sp.csr_matrix(m) for m in mats], vocab, idf)
        return self._want[key]

    def _set(self, name):
        if name == "R_head":
            return self.R[:100]
        if name == "N_tail":
            return self.N[-10:]
        return getattr(self, name)


@pytest.fixture(scope="module")
def lists():
    return _Lists()


def _assert_fit(vec, vocab, idf, what):
    assert vec.vocabulary_ == vocab, what
    np.testing.assert_array_equal(vec.idf_, idf, err_msg=what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_list_r_df_count_in_two_passes_and_k2_through_the_dense_table(ctx, lists, dtype):
    """The default single-GPU fit (marks) of a vocabulary of more than 30 x 1024 columns: the df count takes two passes, the
    keys of the tokens are not columns afterwards and K2 looks them up.  Then a column that was not fitted (kept counts)."""
    (m_ref, head_ref), vocab, idf = lists.want(("R",), ("R", "R_head"), dtype)
    vec = _vectoriser(ctx, dtype)
    p = vec.prepare(lists.R)
    vec.fit_prepared([p])
    assert len(vec.vocabulary_) > DF_PASS_COLUMNS
    _assert_fit(vec, vocab, idf, "list R")
    assert_csr_identical(vec.transform_prepared(p).to_scipy(), m_ref, "list R, the fitted column")
    assert_csr_identical(vec.transform(lists.R[:100]), head_ref, "list R, the first hundred strings alone")


OPTION_SETS = [{}, {"SG_K2_COLUMNS": "0"}, {"SG_DF_MARKS": "0"}, {"SG_DF_REPLICAS": "1"}, {"SG_K2_PLAIN": "1"},
               {"SG_VOCAB_SORTED": "1"}]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opts", OPTION_SETS, ids=_id)
def test_list_n_under_every_switch(ctx, lists, dtype, opts):
    """Names, an empty string, a short one and strings for every tokeniser stage in ONE fitted column: the fit, the fitted
    column's transform and the sklearn-shaped transform of the last ten strings (the five longest among them) alone."""
    (m_ref, tail_ref), vocab, idf = lists.want(("N",), ("N", "N_tail"), dtype)
    what = f"{np.dtype(dtype).name} {_id(opts)}"
    with _options(ctx, opts):
        vec = _vectoriser(ctx, dtype)
        p = vec.prepare(lists.N)
        vec.fit_prepared([p])
        assert ctx.vocab_coding(vec._vocab)[2] is ("SG_VOCAB_SORTED" in opts)
        _assert_fit(vec, vocab, idf, what)
        assert_csr_identical(vec.transform_prepared(p).to_scipy(), m_ref, what + ", the fitted column")
        assert_csr_identical(vec.transform(lists.N[-10:]), tail_ref, what + ", the last ten strings alone")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [("master", "duplicates"), ("duplicates", "master")], ids="+".join)
def test_two_fitted_columns_of_which_one_has_long_strings(ctx, lists, dtype, order):
    """Marks form: "any strings for the last stage?" is answered no for one column and yes for the other (in both orders),
    the vocabulary is taken twice and every column's row pointers are summed twice.  A third column was not fitted."""
    assert max(len(s) for s in lists.master) < 1024 < max(len(s) for s in lists.duplicates)
    (a_ref, b_ref, c_ref), vocab, idf = lists.want(("master", "duplicates"), order + ("other",), dtype)
    assert any(t not in vocab for t in O.ngrams(lists.other[300])) and len(O.ngrams(lists.other[302])) > 1024
    vec = _vectoriser(ctx, dtype)
    pa, pb, pc = (vec.prepare(getattr(lists, name)) for name in order + ("other",))
    vec.fit_prepared([pa, pb])
    _assert_fit(vec, vocab, idf, "+".join(order))
    assert_csr_identical(vec.transform_prepared(pa).to_scipy(), a_ref, order[0])
    assert_csr_identical(vec.transform_prepared(pb).to_scipy(), b_ref, order[1])
    assert_csr_identical(vec.transform_prepared(pc).to_scipy(), c_ref, "the column that was not fitted")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_fitted_column_transformed_twice(ctx, lists, dtype):
    """The first transform takes the row pointers the fit's end summed and read; the second sums its own."""
    (m_ref,), vocab, idf = lists.want(("N",), ("N",), dtype)
    vec = _vectoriser(ctx, dtype)
    p = vec.prepare(lists.N)
    vec.fit_prepared([p])
    first, second = vec.transform_prepared(p), vec.transform_prepared(p)
    assert_csr_identical(first.to_scipy(), m_ref, "first transform")
    assert_csr_identical(second.to_scipy(), m_ref, "second transform")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_split_fit_on_one_device(ctx, lists, dtype):
    """sg_vec_fit_begin + sg_vec_fit_end: the counters form, long strings tokenised at once.  The df table of 3-grams can be
    shared between ranks; that of 5-grams is coded with the alphabet of the local strings and cannot."""
    for kw, shareable in ((dict(), True), (dict(ngram_size=5), False)):
        (a_ref, b_ref), vocab, idf = lists.want(("master", "duplicates"), ("master", "duplicates"), dtype, **kw)
        vec = _vectoriser(ctx, dtype, **kw)
        pm, pd_ = vec.prepare(lists.master), vec.prepare(lists.duplicates)
        vec.fit_begin_prepared([pm, pd_])
        pointer, entries, can_share = vec.df_table()
        assert pointer and entries > 0 and can_share is shareable, kw
        vec.fit_end(0)
        _assert_fit(vec, vocab, idf, str(kw))
        assert_csr_identical(vec.transform_prepared(pm).to_scipy(), a_ref, f"master {kw}")
        assert_csr_identical(vec.transform_prepared(pd_).to_scipy(), b_ref, f"duplicates {kw}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_column_without_non_zeros(ctx, lists, dtype):
    vec = _vectoriser(ctx, dtype)
    vec.fit_prepared([vec.prepare(lists.N_short)])
    got = vec.transform_prepared(vec.prepare(["", "ab", "zq"] * 50)).to_scipy()
    assert got.shape == (150, len(vec.vocabulary_)) and got.nnz == 0
    assert got.data.dtype == dtype and not np.asarray(got.indptr).any()
