"""GPU tests of sg_topn_transpose_select (csrc/sg_corpus.hip) called directly, on the inputs of
tests/_transpose_select_cases.py: both kernels at their limits, a decision at every byte of the radix select's key, scores
of either sign, more queued rows than workgroups.  Every comparison is bit for bit against the plain reference (the
multiply's order: value descending, zeros of either sign equal, then the lower pair row; the input's bits written out).
tests/test_transpose_select_cases_cpu.py shows that these inputs tell the reference from nine wrong ones."""
import numpy as np
import pytest

import string_grouper_amd.engine as E
from oracle import port as P
from string_grouper_amd import _native as N
from string_grouper_amd.synth import synth_names
from tests import _transpose_select_cases as S
from tests.test_corpus_gpu import assert_same, corpus_names, device_multiply, oracle_mats

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng(ctx):
    e = E.HipEngine(ctx)
    E.set_engine(e)
    yield e
    E.set_engine(None)


FAMILY_CASES = [(name, dtype) for name in S.FAMILIES for dtype in S.family_dtypes(name)]


def upload(ctx, t: S.TopN):
    return ctx.topn_from_host(t.cols, t.vals, t.counts, t.n_cols)


def run(ctx, pairs, n_out, top_n):
    """(the result on the host, its dims (rows, stride, dtype code, columns))"""
    res = ctx.topn_transpose_select(pairs, n_out, top_n)
    try:
        dims = res.dims()
        cols, vals, counts = res.to_host()
    finally:
        res.free()
    return S.TopN(cols, vals, counts, dims[3]), dims


def check_case(ctx, family, dtype, index, pairs=None):
    """Every top_n of the case on one upload: dims, counts, columns and score bits of the first counts[m] entries."""
    case = S.family(family, dtype)[index]
    own = pairs is None
    if own:
        pairs = upload(ctx, S.build(case, dtype))
    try:
        failed = []
        for top_n in case.top_n:
            got, dims = run(ctx, pairs, case.n_out, top_n)
            want = S.reference(family, dtype, index, top_n)
            assert dims == (case.n_out, min(top_n, max(case.n_in, 1)), N.np_dtype_code(dtype), case.n_in), (case.name, top_n)
            bad = S.rows_that_differ(got, want)
            print(f"{case.name} {np.dtype(dtype).name} top_n={top_n}: {len(bad)} of {case.n_out} rows differ {bad[:20].tolist()}")
            if len(bad):
                failed.append((top_n, bad[:20].tolist()))
        assert not failed, f"{case.name}: (top_n, rows that differ from the reference) {failed}"
    finally:
        if own:
            pairs.free()


@pytest.mark.parametrize("family,dtype", FAMILY_CASES, ids=[f"{n}-{np.dtype(d).name}" for n, d in FAMILY_CASES])
def test_family_equals_the_reference_bit_for_bit(ctx, family, dtype):
    for index in range(len(S.family(family, dtype))):
        check_case(ctx, family, dtype, index)


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("family", ["many_hubs", "tie_blocks"])
def test_three_runs_give_identical_arrays(ctx, family, dtype):
    """The buckets fill in the order the atomics arrive and the queue of larger rows in the order the waves get there;
    neither may show in the result."""
    (case,) = S.family(family, dtype)
    pairs = upload(ctx, S.build(case, dtype))
    try:
        for top_n in case.top_n:
            runs = [run(ctx, pairs, case.n_out, top_n)[0] for _ in range(3)]
            mask = np.arange(runs[0].cols.shape[1])[None, :] < runs[0].counts[:, None]
            for other in runs[1:]:
                assert np.array_equal(other.counts, runs[0].counts), top_n
                assert np.array_equal(other.cols[mask], runs[0].cols[mask]), top_n
                assert np.array_equal(S.bits(other.vals)[mask], S.bits(runs[0].vals)[mask]), top_n
    finally:
        pairs.free()


# ---------------------------------------------------------------------------------------------------- refusals
GOOD = ("shapes", 0)      # 'extra_rows': a hub of 1 100, a wave row of 70, a row of 3 and empty rows


def good_call_still_right(ctx, dtype):
    check_case(ctx, GOOD[0], dtype, GOOD[1])


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("top_n", [0, 2049, -1])
def test_top_n_outside_1_to_2048_is_refused(ctx, dtype, top_n):
    case = S.family(GOOD[0], dtype)[GOOD[1]]
    pairs = upload(ctx, S.build(case, dtype))
    try:
        with pytest.raises(ValueError, match="top_n"):
            ctx.topn_transpose_select(pairs, case.n_out, top_n)
        check_case(ctx, GOOD[0], dtype, GOOD[1], pairs)
    finally:
        pairs.free()


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_pair_list_with_more_columns_than_result_rows_is_refused(ctx, dtype):
    case = S.family(GOOD[0], dtype)[GOOD[1]]
    pairs = upload(ctx, S.build(case, dtype))
    try:
        assert case.n_cols == 5
        with pytest.raises(ValueError, match="more columns"):
            ctx.topn_transpose_select(pairs, case.n_cols - 1, 10)
        check_case(ctx, GOOD[0], dtype, GOOD[1], pairs)
    finally:
        pairs.free()


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("where", ["hub", "wave_row"])
@pytest.mark.parametrize("column", ["n_rows_out", "minus_one"])
def test_counted_entry_outside_the_result_rows_is_refused(ctx, dtype, column, where):
    """sg_topn_from_host checks nothing, so the entry reaches the kernels: the counting pass flags it, the scatter skips
    it, and the call fails.  One entry of the hub's (corpus row 2) or of the wave row's (corpus row 4) is renamed."""
    case = S.family(GOOD[0], dtype)[GOOD[1]]
    t = S.build(case, dtype)
    cols = t.cols.copy()
    counted = np.arange(cols.shape[1])[None, :] < t.counts[:, None]
    r, j = np.argwhere(counted & (cols == (2 if where == "hub" else 4)))[7]
    cols[r, j] = case.n_out if column == "n_rows_out" else -1
    pairs = upload(ctx, S.TopN(cols, t.vals, t.counts, t.n_cols))
    try:
        for top_n in (1, 70, 2048):
            with pytest.raises(ValueError, match="outside"):
                ctx.topn_transpose_select(pairs, case.n_out, top_n)
    finally:
        pairs.free()
    good_call_still_right(ctx, dtype)


# ---------------------------------------------------------------------------------------------------- one level up
HUB_ROW = 17


def hub_batch():
    """1 500 distinct variants of corpus name 17 -- the name plus six letters out of another corpus name, so that the added
    n-grams are in the corpus's vocabulary and every variant scores differently --, 1 100 exact copies, 100 other names."""
    corpus = corpus_names(2000)
    hub = corpus[HUB_ROW]
    suffixes = list(dict.fromkeys(corpus[j].replace(" ", "")[a:a + 6] for a in (1, 4) for j in range(HUB_ROW + 1, 2000)))[:1500]
    variants = [f"{hub} {s}" for s in suffixes]
    assert len(set(variants)) == 1500
    others = synth_names(100, seed=123, perturb_of=list(corpus), perturb_frac=0.5)
    return corpus, tuple(variants + [hub] * 1100 + list(others))


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_corpus_hub_of_distinct_scores_and_copies_on_the_reverse_path(eng, monkeypatch, dtype):
    """A corpus row whose candidates exceed the workgroup kernel's LDS arrays, with more than a thousand different scores
    among them (the Corpus tests' hubs are copies that all score 1.0), through Corpus-level code: fit, transform, the
    new rows against the corpus index, zip, sg_topn_transpose_select."""
    corpus, batch = hub_batch()
    mc, mn = oracle_mats(corpus, batch, dtype)
    uncut = P.sp_matmul_topn_port(mc, mn.T, len(batch), 0.3, True, 16).getrow(HUB_ROW)
    assert uncut.nnz > S.MAX_TOP_N and len(np.unique(uncut.data)) > 1000
    for top_n in (1500, 2048):
        want = P.sp_matmul_topn_port(mc, mn.T, top_n, 0.3, True, 16)
        assert want.getrow(HUB_ROW).nnz == top_n
        got, took = device_multiply(eng, corpus, batch, dtype, top_n, 0.3, "reverse", monkeypatch)
        assert took == "reverse"
        assert_same(got, want, f"hub of distinct scores, top_n {top_n}")
