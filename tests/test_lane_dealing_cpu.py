"""CPU test: the rule by which the pruned multiply deals a wave's 64 lanes to the prefix terms of a row
(string_grouper_amd/csrc/sg_k4_device.h), through the library's host restatement sg_debug_deal_lanes -- the same
functions the kernel calls -- against a restatement in Python integers.  No GPU.

The rule: every one of the np prefix terms gets a lane; the 64 - np spare ones go by largest remainder,
    spare * df_t = q_t * dsum + rem_t,   G_t = 1 + q_t,   R = 64 - sum G,
and the R terms with the largest rem_t get one more, the first of equal remainders first.  The earlier rule,
G_t = 1 + floor(spare * 0.999 * df_t / dsum) in float32, is kept behind SG_DEAL=floor and restated here in numpy float32.

The hook also evaluates every share the way the wave does (32 bits, a float estimate of the quotient set right by the
remainder) whenever the sum of the lists is below 2^30, and returns 2 if that disagrees with the 64-bit division: every
call below with small enough lists checks the kernel's arithmetic too."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def deal():
    from string_grouper_amd import _native as N
    lib = ctypes.CDLL(N.LIB_PATH)
    fn = lib.sg_debug_deal_lanes
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]

    def call(df, floor_rule=False):
        df = np.ascontiguousarray(df, dtype=np.uint32)
        out = np.zeros(len(df), dtype=np.uint32)
        rc = fn(df.ctypes.data, len(df), out.ctypes.data, 1 if floor_rule else 0)
        assert rc == 0, f"sg_debug_deal_lanes returned {rc} for {df.tolist()}"
        return out.astype(np.int64)
    return call


def restated(df):
    """largest remainder in Python integers; ties to the lower index"""
    df = [int(x) for x in df]
    n, dsum = len(df), sum(df)
    spare = 64 - n
    G = [1 + spare * d // dsum for d in df]
    rem = [spare * d % dsum for d in df]
    R = 64 - sum(G)
    assert 0 <= R < max(n, 2)
    for t in sorted(range(n), key=lambda t: (-rem[t], t))[:R]:
        G[t] += 1
    return np.array(G, dtype=np.int64)


def restated_floor(df):
    df = np.asarray(df, dtype=np.uint32)
    n = len(df)
    dsum = np.float32(int(df.astype(np.uint64).sum()))
    share = df.astype(np.float32) / dsum
    assert share.dtype == np.float32
    x = np.float32(64 - n) * np.float32(0.999)
    return 1 + np.floor(x * share).astype(np.int64)


def rows():
    """(name, df) of every input the rule is tried on"""
    out = []
    for n in (1, 2, 3, 63, 64):
        out.append((f"np={n} equal", [19] * n))
        out.append((f"np={n} rising", list(range(1, n + 1))))
        out.append((f"np={n} one long", [100000] + [3] * (n - 1)))
    for n in (5, 7, 9, 10, 11, 13, 31, 33, 50):
        out.append((f"all equal np={n}", [1234] * n))            # every remainder ties
        out.append((f"all one np={n}", [1] * n))
        out.append((f"one list 1000 x the others np={n}", [7] * (n - 1) + [7000]))
        out.append((f"one list 1000 x the others, first, np={n}", [2000] + [2] * (n - 1)))
    out.append(("a list of 199 beside ten of 2", [199] + [2] * 10))
    out.append(("empty lists among the others", [0, 5, 0, 9, 1]))
    # up to 2^31: sums beyond 32 bits (the 64-bit evaluation alone), and sums just below 2^30 (the wave's, too)
    out.append(("2^31 and small", [2 ** 31, 1, 2, 3]))
    out.append(("2^31 everywhere", [2 ** 31] * 64))
    out.append(("2^31 and 2^31 - 1", [2 ** 31 - 1, 2 ** 31, 2 ** 31 - 1, 2 ** 31]))
    out.append(("sum 2^30 - 1", [2 ** 29, 2 ** 29 - 1]))
    out.append(("sum just below 2^30, many", [2 ** 24 - 1] * 63 + [5]))
    out.append(("sum 2^30 - 1, one long", [2 ** 30 - 64] + [1] * 63))
    rng = np.random.default_rng(20240607)
    for i in range(2000):
        n = int(rng.integers(1, 65))
        kind = i % 4
        if kind == 0:      # name data: many short lists, a few long ones
            df = np.floor(np.exp(rng.uniform(0.0, 12.0, n))).astype(np.int64)
        elif kind == 1:    # small numbers: many equal remainders
            df = rng.integers(1, 6, n)
        elif kind == 2:    # the whole range of the wave's arithmetic (sum below 2^30)
            df = rng.integers(1, 2 ** 30 // 64, n)
        else:              # up to 2^31
            df = rng.integers(1, 2 ** 31 + 1, n)
        out.append((f"random {i}", [int(x) for x in df]))
    return out


ROWS = rows()


def test_inputs_cover_what_they_should():
    sizes = {len(df) for _, df in ROWS}
    assert {1, 2, 3, 63, 64} <= sizes
    assert sum(name.startswith("random") for name, _ in ROWS) == 2000
    assert any(max(df) == 2 ** 31 for _, df in ROWS)
    assert any(sum(df) < 2 ** 30 and sum(df) > 2 ** 29 for _, df in ROWS)


def test_every_lane_is_dealt_and_every_term_has_one(deal):
    for name, df in ROWS:
        G = deal(df)
        assert G.sum() == 64, (name, df, G.tolist())
        assert G.min() >= 1, (name, df, G.tolist())


def test_a_longer_list_never_has_fewer_lanes(deal):
    for name, df in ROWS:
        G = deal(df)
        d = np.asarray(df, dtype=np.int64)
        order = np.argsort(d, kind="stable")
        # along ascending df, G may only fall between EQUAL df (ties go to the term that comes first)
        falls = (np.diff(G[order]) < 0) & (np.diff(d[order]) > 0)
        assert not falls.any(), (name, df, G.tolist())
        # ... and equal lists differ by one lane at most, the earlier term having the larger share
        for v in np.unique(d):
            g = G[d == v]
            assert g.max() - g.min() <= 1 and (np.diff(g) <= 0).all(), (name, df, G.tolist())


def test_equals_the_restatement_entry_for_entry(deal):
    for name, df in ROWS:
        assert np.array_equal(deal(df), restated(df)), (name, df)


def test_floor_rule_is_the_earlier_formula(deal):
    idle = 0
    for name, df in ROWS:
        G = deal(df, floor_rule=True)
        assert np.array_equal(G, restated_floor(df)), (name, df)
        assert G.min() >= 1 and G.sum() <= 64, (name, df, G.tolist())
        idle += 64 - int(G.sum())
    assert idle > 0      # what the new rule is for: the earlier one leaves lanes without a term


def test_known_rows(deal):
    assert deal([5]).tolist() == [64]
    assert deal([1, 1]).tolist() == [32, 32]
    assert deal([1, 1, 1]).tolist() == [22, 21, 21]          # 61 spare lanes: 20 each, the remainder to the first
    assert deal([3] * 64).tolist() == [1] * 64
    # 53 spare lanes: 53 * 199 / 219 = 48 rem 35 for the long list, 0 rem 106 for each short one: the five lanes left over
    # go to the first five short lists
    assert deal([199] + [2] * 10).tolist() == [49, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1]


def test_arguments_the_kernel_never_sees_are_refused():
    from string_grouper_amd import _native as N
    lib = ctypes.CDLL(N.LIB_PATH)
    out = np.zeros(80, dtype=np.uint32)
    for df in ([], [1] * 65, [0, 0, 0]):
        a = np.asarray(df, dtype=np.uint32)
        assert lib.sg_debug_deal_lanes(ctypes.c_void_p(a.ctypes.data if len(a) else None), ctypes.c_int(len(a)),
                                       ctypes.c_void_p(out.ctypes.data), ctypes.c_int(0)) == 1
