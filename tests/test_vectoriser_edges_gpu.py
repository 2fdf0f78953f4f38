"""GPU tests of the vectoriser's kernels (csrc/sg_vectorize.hip: K1, tokenise, and K2, weight and normalise) on the string
lists of tests/_vectoriser_edge_cases.py: every stage of the tokeniser at its limits, every form of key on byte and on symbol
columns, strings that were not fitted, and K2's rows at the ends of its trips of sixteen.  Vocabulary, idf and matrix are
compared with sklearn's bit for bit; the norms and the three words K2 leaves with a matrix are compared with the rows.
tests/test_vectoriser_edge_cases_cpu.py shows that the lists hold every edge and tell the reference from ten wrong ones."""
import math

import numpy as np
import pytest

from tests import _vectoriser_edge_cases as V
from tests.test_parity_gpu import assert_csr_identical
from tests.test_postings_build_paths_gpu import _id, _options

pytestmark = pytest.mark.gpu

CASES = [c.name for c in V.all_cases() if c.name != "few-columns-n1-bytes"]        # (that one has a test of its own)
SWITCHED = [n for n in CASES if n.startswith(("short-", "wave-", "missing-"))]
SWITCHES = [{"SG_K2_PLAIN": "1"}, {"SG_DF_MARKS": "0"}, {"SG_DF_REPLICAS": "1"}, {"SG_K2_COLUMNS": "0"}, {"SG_VOCAB_SORTED": "1"}]
WORDS = {"SG_ROW_BLOCKS": "1"}          # K2 leaves its three words only for the opt-in row blocks


def _name(dtype):
    return np.dtype(dtype).name


def _vectoriser(ctx, dtype, **kw):
    from string_grouper_amd.vectorizer import HipTfidfVectorizer
    return HipTfidfVectorizer(dtype=dtype, ctx=ctx, **kw)


def float32_at_or_above(x: float) -> np.float32:
    f = np.float32(x)
    return f if float(f) >= x else np.nextafter(f, np.float32(np.inf))


def check_words(m, got, what):
    """The words the multiply's gate trusts, against the rows: no violations; the longest row exactly; the norm word not
    below the largest sum of squares of a stored row (in double, exactly rounded) and not above that value rounded up to
    float32 and raised by two float32 steps -- the kernel rounds up once after a factor of 1 + 1e-12."""
    words = m.vectoriser_words()
    assert words is not None, what
    violations, norm_word, longest = words
    lengths = np.diff(got.indptr)
    squares = got.data.astype(np.float64) ** 2
    largest = max((math.fsum(squares[lo:hi].tolist()) for lo, hi in zip(got.indptr[:-1], got.indptr[1:])), default=0.0)
    top = float32_at_or_above(largest)
    for _ in range(2):
        top = np.nextafter(top, np.float32(np.inf))
    print(f"{what}: words {words}, largest sum of squares {largest!r}, longest row {int(lengths.max()) if len(lengths) else 0}")
    assert violations == 0, what
    assert longest == (int(lengths.max()) if len(lengths) else 0), what
    assert largest <= norm_word <= float(top), (what, largest, norm_word, float(top))


def check_matrix(m, want, want_norms, what, words):
    """One matrix the vectoriser made: sklearn's bits, the norm of every row, and (asked for) the words."""
    try:
        got = m.to_scipy()
        assert_csr_identical(got, want, what)
        norms = m.row_norms()
        assert norms is not None and np.array_equal(norms.view(np.uint64), want_norms.view(np.uint64)), what + ": row norms"
        assert not norms[np.diff(want.indptr) == 0].any(), what
        if words:
            check_words(m, got, what)
        else:
            assert m.vectoriser_words() is None
    finally:
        m.free()


def fit_and_check(ctx, case, dtype, what, opts):
    mats, vocab, idf = V.sklearn_reference(case.name, dtype)
    vec = _vectoriser(ctx, dtype, **case.form.kw)
    fitted = vec.prepare(case.fit)
    vec.fit_prepared([fitted])
    bits, symbols, sorted_vocabulary = ctx.vocab_coding(vec._vocab)
    assert (bits, symbols) == (V.device_bits(case.form, case.fit), case.form.symbols), what
    assert sorted_vocabulary == (case.form.keys == "key64" or opts.get("SG_VOCAB_SORTED") == "1"), what
    assert vec.vocabulary_ == vocab, what
    assert vec.idf_.dtype == idf.dtype and np.array_equal(vec.idf_, idf), what
    return vec, fitted


def run_case(ctx, name, dtype, opts):
    """Fit; then every list of the case -- the fitted column first -- is transformed twice in turn and a third time in the
    opposite order, so that it follows another list each time: a result must not depend on what the scratch held.  The third
    round runs without the words."""
    case = V.case(name)
    mats, _, _ = V.sklearn_reference(name, dtype)
    norms = V.norms_reference(name, dtype)
    what = f"{name} {_name(dtype)} {_id(opts)}"
    with _options(ctx, {**opts, **WORDS}):
        vec, fitted = fit_and_check(ctx, case, dtype, what, opts)
        columns = [fitted] + [vec.prepare(list(s)) for _, s in case.others]
        order = list(range(len(columns)))
        for round_, idx in enumerate((order, order, order[::-1])):
            if round_ == 2:
                ctx.set_option("SG_ROW_BLOCKS", None)
            for k in idx:
                where = f"{what}, list '{case.lists()[k][0]}', transform {round_ + 1}"
                check_matrix(vec.transform_prepared(columns[k]), mats[k], norms[k], where, words=round_ < 2)


@pytest.mark.parametrize("dtype", V.DTYPES, ids=_name)
@pytest.mark.parametrize("name", CASES)
def test_list_equals_sklearn_bit_for_bit(ctx, name, dtype):
    run_case(ctx, name, dtype, {})


@pytest.mark.parametrize("dtype", V.DTYPES, ids=_name)
@pytest.mark.parametrize("opts", SWITCHES, ids=_id)
@pytest.mark.parametrize("name", SWITCHED)
def test_short_wave_and_unfitted_lists_under_every_switch(ctx, name, opts, dtype):
    """The thread-per-row K2, df counters (in eight copies and in one) instead of marks, K2 through the dense table, and the
    sorted vocabulary with its 64-bit keys for every form."""
    run_case(ctx, name, dtype, opts)


@pytest.mark.parametrize("dtype", V.DTYPES, ids=_name)
def test_idf_reaches_the_device_both_ways_with_the_same_bits(ctx, dtype):
    """307 documents over eight columns: the first fit of that many documents fetches the counts and sends the weights (the
    vectoriser then holds them), the second weights on the device from a table (it holds none until asked)."""
    case = V.case("few-columns-n1-bytes")
    (want,), vocab, idf = V.sklearn_reference(case.name, dtype)
    (norms,) = V.norms_reference(case.name, dtype)
    with _options(ctx, WORDS):
        for attempt, on_host in ((1, True), (2, False)):
            vec = _vectoriser(ctx, dtype, **case.form.kw)
            fitted = vec.prepare(case.fit)
            vec.fit_prepared([fitted])
            assert (vec._idf is not None) == on_host, f"fit {attempt}"
            assert vec.vocabulary_ == vocab and np.array_equal(vec.idf_.view(np.uint8), idf.view(np.uint8)), f"fit {attempt}"
            check_matrix(vec.transform_prepared(fitted), want, norms, f"{case.name} {_name(dtype)} fit {attempt}", words=True)
            check_matrix(vec.transform_prepared(vec.prepare(list(case.fit))), want, norms,
                         f"{case.name} {_name(dtype)} fit {attempt}, the strings as a column that was not fitted", words=True)


@pytest.mark.parametrize("dtype", V.DTYPES, ids=_name)
def test_keys_of_64_bits_are_refused_and_a_good_fit_follows(ctx, dtype):
    """16 characters over an alphabet of 16 need one bit more than the 63 the vocabulary holds."""
    n, chars = V.TOO_WIDE["ngram_size"], V.TOO_WIDE["chars"]
    rng = np.random.default_rng(64)
    strings = [chars] + ["".join(chars[i] for i in rng.integers(0, 16, 40)) for _ in range(20)]
    with pytest.raises(NotImplementedError, match="64-bit keys"):
        _vectoriser(ctx, dtype, ngram_size=n).fit(strings)
    run_case(ctx, "short-n21a8-bytes", dtype, {})
