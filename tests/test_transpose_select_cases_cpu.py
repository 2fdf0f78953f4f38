"""The inputs, the reference and the mutants of tests/_transpose_select_cases.py, checked without a GPU and without the
library.  Every mutant -- the reference with one thing wrong -- gives a different answer on the family that was built for
it, and the families have the sizes, bytes and signs that tests/test_transpose_select_gpu.py relies on: an input that cannot
tell a mutant from the reference could not tell a wrong kernel either."""
import numpy as np
import pytest

from tests import _transpose_select_cases as S

F32, F64 = np.float32, np.float64


def differing(family, dtype, mutant):
    """{(case index, top_n): rows on which the mutant differs from the reference}, over the family's own top_n values."""
    out = {}
    for i, case in enumerate(S.family(family, dtype)):
        for top_n in case.top_n:
            rows = S.rows_that_differ(S.select(case, dtype, top_n, **S.MUTANTS[mutant]), S.reference(family, dtype, i, top_n))
            if len(rows):
                out[i, top_n] = rows
    return out


def byte_of(v, b):
    """Byte b (0: the most significant) of the bit patterns."""
    u = S.bits(v)
    return (u >> u.dtype.type(8 * (u.itemsize - 1 - b))) & u.dtype.type(0xff)


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_reference_is_the_order_of_the_port_on_a_row_written_out():
    """Value descending, zeros of either sign equal, then the lower pair row; the input's bits come out."""
    d = np.array([5, 1, 9, 3, 7, 2], np.int64)
    s = np.array([0.0, -0.0, 2.5, -1.0, 0.0, 2.5], F32)
    case = S._case("by_hand", {0: (d, s)}, 10, 1, (4,))
    got = S.select(case, F32, 4)
    assert got.counts.tolist() == [4] and got.cols[0].tolist() == [2, 9, 1, 5]
    assert S.bits(got.vals[0]).tolist() == S.bits(np.array([2.5, 2.5, -0.0, 0.0], F32)).tolist()
    assert S.select(case, F32, 4, order=S.order_bit_key).cols[0].tolist() == [2, 9, 5, 7]
    assert got.cols.shape == (1, 4) and S.select(case, F32, 2048).cols.shape == (1, 10) and got.n_cols == 10


@pytest.mark.parametrize("name", sorted(S.FAMILIES))
def test_pair_lists_meet_the_contract_and_carry_rubbish_behind_the_counts(name):
    """No pair row names a column twice, columns inside the list's, the stride is the longest pair row, and every slot behind
    a count holds column -7 and NaN.  The list holds exactly the family's pairs."""
    for dtype in S.family_dtypes(name):
        for case in S.family(name, dtype):
            t = S.build(case, dtype)
            S.check_pair_list(t)
            assert t.cols.shape[0] == case.n_in and t.n_cols == case.n_cols <= case.n_out
            assert t.counts.sum() == sum(len(d) for d, _ in case.pairs.values())
            for m, (d, s) in list(case.pairs.items())[:20]:
                r, j = np.nonzero((t.cols == m) & (np.arange(t.cols.shape[1])[None, :] < t.counts[:, None]))
                o = np.argsort(d)
                assert np.array_equal(r, d[o]) and np.array_equal(S.bits(t.vals[r, j]), S.bits(s[o]))
            assert all(1 <= k <= S.MAX_TOP_N for k in case.top_n)


def test_pair_rows_are_shuffled():
    t = S.build(S.family("many_hubs", F32)[0], F32)
    full = t.cols[t.counts == t.cols.shape[1]]
    assert len(full) and (np.diff(full.astype(np.int64), axis=1) < 0).any(axis=1).all()


# ---------------------------------------------------------------------------------------------------- structural facts
@pytest.mark.parametrize("dtype", S.DTYPES)
def test_bucket_sizes_are_as_listed(dtype):
    (case,) = S.family("bucket_sizes", dtype)
    assert S.BUCKET_SIZES == (0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1026, 1087, 1088, 2047, 2048, 2049, 3000)
    assert tuple(len(d) for d, _ in case.pairs.values()) == S.BUCKET_SIZES and case.n_in == 3000
    assert case.top_n == (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048)
    # on the workgroup kernel: keep = c - 1 (1 025 of 1 026, 2 047 of 2 048), keep = c (1 025, 2 047, 2 048), full LDS arrays
    big = [c for c in S.BUCKET_SIZES if c > S.WAVE_MAX]
    assert {c - 1 for c in big} & set(case.top_n) and set(big) & set(case.top_n)
    assert S.MAX_TOP_N in case.top_n and max(big) > S.MAX_TOP_N
    for d, s in case.pairs.values():      # equal scores and full-mantissa ones in every larger bucket
        assert len(d) < 63 or (len(np.unique(s)) > len(s) // 3 and (s == 0.5).sum() > len(s) // 10)


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_many_hubs_has_more_big_rows_than_workgroups(dtype):
    (case,) = S.family("many_hubs", dtype)
    c = np.array([len(d) for d, _ in case.pairs.values()])
    assert len(c) == case.n_out == case.n_in == 1100
    assert (c > S.WAVE_MAX).sum() == S.MANY_HUBS_BIG > S.BIG_GRID and c.min() >= 1000 and c.max() <= 1100
    assert case.top_n == (1, 1030, 2048)
    # with top_n = 1030 queued rows of both kinds: taken whole and selected from
    assert ((c > S.WAVE_MAX) & (c <= 1030)).sum() > 10 and (c > 1030).sum() > S.BIG_GRID


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_every_score_byte_hub_has_equal_upper_bytes_and_decides_at_its_byte(dtype):
    """Hub b: positive finite scores, all distinct (more distinct values than any top_n below the hub's size), the bytes
    above b equal, and many different digits at byte b itself -- every value of the byte that leaves the score positive,
    finite and normal for the sign's byte (0x01 .. 0x7e, at least 100 of them drawn), over 200 below it.  The lowest byte:
    neighbouring floats, so the byte takes all 256 values and the byte above it counts them in sixes."""
    (case,) = S.family("deciding_score_byte", dtype)
    nb = np.dtype(dtype).itemsize
    assert case.top_n == (1, 255, 256, 257, 749, 1499, 1500) and case.n_out == nb + 1
    for b in range(nb):
        d, s = case.pairs[b]
        assert len(s) == 1500 > S.WAVE_MAX and len(np.unique(s)) == 1500 and np.isfinite(s).all() and (s > 0).all()
        assert (s >= np.finfo(dtype).tiny).all()
        digits = len(np.unique(byte_of(s, b)))
        if b < nb - 1:
            assert all(len(np.unique(byte_of(s, a))) == 1 for a in range(b))
            assert digits >= (100 if b == 0 else 200)
        else:
            assert all(len(np.unique(byte_of(s, a))) == 1 for a in range(b - 1))
            assert digits == 256 and len(np.unique(byte_of(s, b - 1))) == 6
            u = np.sort(S.bits(s))
            assert (np.diff(u) == 1).all()
    d, s = case.pairs[nb]
    assert len(s) == 300 and (np.diff(np.sort(S.bits(s))) == 1).all()


def test_the_row_byte_hub_has_equal_scores_and_rows_in_all_four_byte_ranges():
    (case,) = S.family("deciding_row_byte", F32)
    assert case.n_in == (1 << 24) + 2048 and case.n_out == 8
    assert case.top_n == (100, 200, 400, 600, 800, 1000, 1200, 1400)
    d, s = case.pairs[S.ROW_BYTE_HUB]
    assert len(np.unique(S.bits(s))) == 1 and len(d) == 1600 > S.WAVE_MAX and len(np.unique(d)) == 1600
    ends = np.cumsum([((d >= lo) & (d < hi)).sum() for lo, hi, _ in S.ROW_BYTE_RANGES])
    assert ends.tolist() == [200, 600, 1000, 1600]
    assert set(ends[:3]) <= set(case.top_n)                                             # cuts exactly at a range's end
    assert all(any(lo < k < hi for k in case.top_n) for lo, hi in zip([0] + ends.tolist(), ends))     # and inside each
    u = d.astype(np.uint32).view(np.float32)         # (byte_of reads bit patterns)
    for k, (lo, hi, _) in enumerate(S.ROW_BYTE_RANGES):
        inside = u[(d >= lo) & (d < hi)]
        b = (3, 2, 1, 2)[k]                          # the first byte that differs inside the range
        assert all(len(np.unique(byte_of(inside, a))) == 1 for a in range(b))
        assert len(np.unique(byte_of(inside, b))) > (100 if k != 3 else 7)
        assert (byte_of(inside, 0) == (1 if k == 3 else 0)).all()       # only the last range has the top byte set
    dw, sw = case.pairs[S.ROW_BYTE_WAVE_ROW]
    assert 100 < len(dw) <= S.WAVE_MAX and (dw >= 1 << 24).any() and not len(np.intersect1d(dw, d))


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_signs_hold_every_kind_of_value_and_zeros_the_two_orders_disagree_on(dtype):
    (case,) = S.family("signs", dtype)
    info = np.finfo(dtype)
    for m, lay in ((0, S.SIGNS_HUB), (1, S.SIGNS_WAVE_ROW)):
        d, s = case.pairs[m]
        assert len(d) == lay.n and (lay.n > S.WAVE_MAX) == (m == 0)
        assert np.isposinf(s).sum() == 1 and (s == info.max).sum() == 1 and not np.isnan(s).any() and not np.isneginf(s).any()
        for sign in (1, -1):
            assert ((sign * s > 0) & (sign * s < info.tiny)).sum() == lay.denormal
            assert ((sign * s >= 0.001) & (sign * s < 1001)).sum() > 25
        zero = s == 0
        assert zero.sum() == lay.zeros and np.signbit(s[zero]).sum() == lay.zeros // 2
        assert (s > 0).sum() == lay.before_zeros
        o = np.argsort(d[zero])
        assert np.signbit(s[zero][o]).tolist() == [True, False] * (lay.zeros // 2)          # -0.0 at the lowest pair row
        lo, hi = lay.before_zeros, lay.before_zeros + lay.zeros
        assert {lo - 1, lo, lo + 1, hi - 1, hi, hi + 1} <= set(case.top_n)
        assert any(lo < k < hi for k in case.top_n)


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_tie_blocks_have_equal_scores_across_every_cut(dtype):
    (case,) = S.family("tie_blocks", dtype)
    assert tuple(len(d) for d, _ in case.pairs.values()) == (1024, 1025, 2049, 5000, 5000) and case.top_n == (64, 1024, 2047, 2048)
    for m, c in enumerate(S.TIE_BUCKETS):
        d, s = case.pairs[m]
        v = np.sort(s)[::-1]
        for a, b in ((62, 65), (1022, 1025), (2046, 2048)):         # positions 63 / 64 / 65 ... counted from 1
            if b < c:
                assert v[a] == v[b], (c, a, b)
        runs = sum(min(hi, c) - lo - 1 for lo, hi in S.TIE_RUNS if lo < c)
        assert len(np.unique(s)) == c - runs                                          # distinct everywhere else
    assert len(np.unique(case.pairs[4][1])) == 1


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_shapes_are_the_listed_ends(dtype):
    by_name = {c.name: c for c in S.family("shapes", dtype)}
    assert by_name["extra_rows"].n_cols < by_name["extra_rows"].n_out
    assert max(by_name["extra_rows"].pairs) < by_name["extra_rows"].n_cols
    assert by_name["five_pair_rows"].n_in == 5 and S.MAX_TOP_N in by_name["five_pair_rows"].top_n
    assert S.reference("shapes", dtype, 1, 2048).cols.shape == (7, 5)
    assert by_name["one_pair_row"].n_in == 1
    assert by_name["no_entries"].pairs == {} and by_name["no_entries"].n_in > 0
    assert (by_name["no_pair_rows_no_result_rows"].n_in, by_name["no_pair_rows_no_result_rows"].n_out) == (0, 0)
    assert (by_name["no_pair_rows"].n_in, by_name["no_pair_rows"].n_out) == (0, 3)
    assert S.reference("shapes", dtype, 5, 2048).cols.shape == (3, 1)


# ---------------------------------------------------------------------------------------------------- the mutants
@pytest.mark.parametrize("dtype", S.DTYPES)
def test_a_bit_key_order_differs_on_signs(dtype):
    """On both rows (hub and wave row), at every top_n that cuts inside the zeros; a cut outside them still shows the order."""
    diff = differing("signs", dtype, "a_bit_key_order")
    for m, lay in ((0, S.SIGNS_HUB), (1, S.SIGNS_WAVE_ROW)):
        for k in (lay.before_zeros + 1, lay.before_zeros + lay.zeros // 2, lay.before_zeros + lay.zeros - 1):
            assert m in diff[0, k]
        assert m not in diff.get((0, lay.before_zeros), [])


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("mutant", ["b_high_row_first", "c_arrival_order"])
def test_b_c_tie_rules_differ_on_tie_blocks(mutant, dtype):
    diff = differing("tie_blocks", dtype, mutant)
    assert set(diff) == {(0, k) for k in (64, 1024, 2047, 2048)}
    assert all(4 in rows for rows in diff.values())                     # the all-equal bucket at every cut
    assert set(diff[0, 64]) == {0, 1, 2, 3, 4} and {2, 3} <= set(diff[0, 2047])


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("mutant", ["b_high_row_first", "c_arrival_order"])
def test_b_c_tie_rules_differ_on_bucket_sizes_and_many_hubs(mutant, dtype):
    assert set(differing("bucket_sizes", dtype, mutant)) == {(0, k) for k in (63, 64, 65, 1023, 1024, 1025, 2047, 2048)}
    assert all(len(rows) > 1000 for rows in differing("many_hubs", dtype, mutant).values())


def test_d_rounding_to_float32_differs_on_the_low_score_bytes_of_float64():
    """float32 keeps the sign, 8 bits of exponent and 23 of the mantissa: bytes 0 .. 3 of a float64 and three bits of byte 4.
    The hubs of bytes 5, 6 and 7 collapse to one value."""
    diff = differing("deciding_score_byte", F64, "d_rounded_to_float32")
    for k in (1, 255, 256, 257, 749, 1499):
        assert {4, 5, 6, 7, 8} <= set(diff[0, k])
    assert all(len(np.unique(S.family("deciding_score_byte", F64)[0].pairs[b][1].astype(F32))) == 1 for b in (5, 6, 7))


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_e_ignoring_the_lowest_score_byte_differs_on_deciding_score_byte(dtype):
    """On the hub of neighbouring floats (row nb - 1) and on the wave row (row nb) at every cut."""
    nb = np.dtype(dtype).itemsize
    diff = differing("deciding_score_byte", dtype, "e_without_lowest_byte")
    for k in (1, 255, 256, 257, 749, 1499):
        assert nb - 1 in diff[0, k]
    assert all(nb in diff[0, k] for k in (1, 255, 256, 257))


def test_f_rows_modulo_2_24_differ_on_deciding_row_byte():
    """Wherever the cut lies behind the first rows that 2^24 folds down: those land among the first 2 048."""
    diff = differing("deciding_row_byte", F32, "f_row_modulo_2_24")
    assert all(S.ROW_BYTE_HUB in diff[0, k] for k in (100, 200, 400, 600, 800, 1000, 1200, 1400))
    assert S.ROW_BYTE_WAVE_ROW in diff[0, 100]


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_g_raw_bits_differ_on_signs(dtype):
    diff = differing("signs", dtype, "g_raw_bits")
    assert all({0, 1} <= set(diff[0, k]) for k in S.family("signs", dtype)[0].top_n)


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_h_cutting_big_rows_at_1024_differs_on_bucket_sizes_and_tie_blocks(dtype):
    diff = differing("bucket_sizes", dtype, "h_big_rows_at_wave_max")
    big = [m for m, c in enumerate(S.BUCKET_SIZES) if c > S.WAVE_MAX]
    assert set(diff) == {(0, 1025), (0, 2047), (0, 2048)} and set(diff[0, 1025]) == set(big)
    diff = differing("tie_blocks", dtype, "h_big_rows_at_wave_max")
    assert set(diff) == {(0, 2047), (0, 2048)} and set(diff[0, 2048]) == {1, 2, 3, 4}


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_i_leaving_the_pivot_out_differs_on_bucket_sizes_and_tie_blocks(dtype):
    diff = differing("bucket_sizes", dtype, "i_without_pivot")
    assert len(diff) == 10
    for k in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048):          # exactly the rows that are cut
        assert set(diff[0, k]) == {m for m, c in enumerate(S.BUCKET_SIZES) if c > k}
    diff = differing("tie_blocks", dtype, "i_without_pivot")
    assert set(diff[0, 1024]) == {1, 2, 3, 4} and set(diff[0, 2048]) == {2, 3, 4}
