"""The pruned multiply on rows made to pin down how a wave's 64 lanes are dealt to a row's prefix terms
(tests/_lane_dealing_cases.py: rows of exactly 1, 2, 63 and 64 rare terms; one list of 199 entries beside ten of 2 and rows
whose lists are all equal, over two super-tiles; rows of 65 .. 128 entries with 60 .. 64 prefix terms in both halves of the
row), in every setting the dealing serves -- f32 and f64, the self-join form and the one-sided one, the stream form and the
tile-by-tile loop (SG_K4_STREAM=0), the largest-remainder rule and the earlier one (SG_DEAL=floor):

  * the result is the oracle port's, bit for bit (indptr, indices, data);
  * the pruned kernel really took the rows (prune_rows > 0, nothing went to the exact kernel);
  * the two dealings see the same rows and the same postings: the rule only decides which lane reads which posting.
    (prune_survivors may differ: the order of the adds decides which posting finds a folded accumulator above its bar.)

tests/test_lane_dealing_cpu.py checks the rule itself without a GPU, tests/test_lane_dealing_cases_cpu.py that the matrices
are what they claim to be."""
import numpy as np
import pytest

from tests import _lane_dealing_cases as L

pytestmark = pytest.mark.gpu

# (the bar of the pruned kernels and the pruned-or-exact pilot are tunings: out of the way)
BASE = {"SG_COLLAPSE": "0", "SG_PRUNE_MIN_THRESHOLD": "0.25", "SG_PRUNE_PILOT": "0"}


def assert_identical(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got.indptr, want.indptr), f"{what}: match counts differ"
    assert np.array_equal(got.indices, want.indices), f"{what}: match columns differ"
    assert got.data.dtype == want.data.dtype and np.array_equal(got.data, want.data), f"{what}: scores differ"


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", L.CASES)
def test_every_form_and_dealing_gives_the_port_s_bits(ctx, case, dtype):
    A = L.matrix(case, dtype)
    want = L.port(case, dtype)
    runs = 0
    for stream in (None, "0"):
        ctx.reset_options()
        for k, v in BASE.items():
            ctx.set_option(k, v)
        if stream is not None:
            ctx.set_option("SG_K4_STREAM", stream)
        dA = ctx.csr_from_scipy(A)
        post = ctx.postings_build(dA)
        for sym in ("1", "0"):
            ctx.set_option("SG_SYM", sym)
            seen = {}
            for deal in (None, "floor"):
                ctx.set_option("SG_DEAL", deal)
                res = ctx.spgemm_topn(dA, post, L.TOP_N, L.THRESHOLD, True)
                st = ctx.stats()
                got = res.to_scipy()
                res.free()
                what = f"{case} {np.dtype(dtype).name} SG_K4_STREAM={stream} SG_SYM={sym} SG_DEAL={deal}"
                print(what, {k: st[k] for k in ("prune_rows", "prune_postings", "prune_survivors", "prune_scored", "exact_rows",
                                                "prune_symmetric")})
                assert st["prune_rows"] > 0 and st["exact_rows"] == 0, f"{what}: another kernel took rows: {st}"
                assert st["prune_symmetric"] == int(sym), f"{what}: another form ran: {st}"
                assert_identical(got, want, what)
                seen[deal] = (st["prune_rows"], st["prune_postings"])
                runs += 1
            assert seen[None] == seen["floor"], f"{case} SG_K4_STREAM={stream} SG_SYM={sym}: rows / postings differ between the dealings: {seen}"
        post.free()
        dA.free()
    assert runs == 8
