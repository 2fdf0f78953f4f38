"""The index build's count and fill (sg_postings.hip: plan_build's split, postings_count_lds, postings_fill_staged) on the
matrices of tests/_fill_edge_cases.py, in which every posting of a checked cell decides a match
(tests/test_fill_edge_cases_cpu.py): the index is built under every number of parts the planner may choose, with parts of one
chunk and of several, staged and posting by posting, and the multiply over it must give the port's bits -- f32 and f64, the
self-join and a one-sided product.  The index is built in row order (permute=False) so that the cells are the ones the cases
describe; one run leaves the library's row permutation on."""
import numpy as np
import pytest

from tests import _fill_edge_cases as F
from tests.test_parity_gpu import assert_csr_identical

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def on_device(_session_ctx):
    made = {}

    def get(name, dtype):
        if (name, dtype) not in made:
            c = F.case(name, dtype)
            made[name, dtype] = (_session_ctx.csr_from_scipy(c.B), _session_ctx.csr_from_scipy(c.B[c.left_rows]))
        return made[name, dtype]

    yield get
    for dA, dL in made.values():
        dL.free()
        dA.free()


def _id(opts):
    return "+".join(f"{k[3:].lower()}={v}" for k, v in opts.items()) or "defaults"


def _build_multiply_compare(ctx, on_device, name, dtype, opts, permute=False):
    c = F.case(name, dtype)
    dA, dL = on_device(name, dtype)
    for k, v in opts.items():               # (the ctx fixture takes them back when the test ends)
        ctx.set_option(k, v)
    if c.collapse_off:
        ctx.set_option("SG_COLLAPSE", "0")
    post = ctx.postings_build(dA, permute=permute)
    try:
        for one_sided in (False, True):
            res = ctx.spgemm_topn(dL if one_sided else dA, post, F.TOP_N, F.THRESHOLD, True)
            st = ctx.stats()
            got = res.to_scipy()
            res.free()
            assert st["prune_rows"] > 0, st          # the pruned multiply: it finds candidates through the filter postings alone
            assert_csr_identical(got, F.port(name, dtype, one_sided), f"{name} {dtype.__name__} {_id(opts)} one_sided={one_sided}")
    finally:
        post.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", F.SPLITS)
@pytest.mark.parametrize("name", ["one_tile", "frequent_everywhere", "rows_of_60"])
def test_every_split_the_planner_may_choose(ctx, on_device, name, dtype, split):
    """One tile that is not full (3 000 rows) in 1 .. 8 parts: cells of 0, 1, 63, 64 and 65 entries in part 0, a group with an
    entry or two in every part, rows of 0, 1, 16, 17 and 64 entries, the first and the last term occupied, an odd vocabulary
    of ~18 000; a frequent term in every row; rows of 60 entries, for which a part is several chunks under every split."""
    _build_multiply_compare(ctx, on_device, name, dtype, {"SG_POSTINGS_SPLIT": str(split)})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opts", [{}, {"SG_POSTINGS_SPLIT": "3"}, {"SG_POSTINGS_SPLIT": "5"}, {"SG_POSTINGS_SPLIT": "7"}], ids=_id)
@pytest.mark.parametrize("name", ["two_tiles_and_a_row", "ends_on_a_part", "part_of_one_row"])
def test_row_counts_at_the_edges_of_tiles_and_parts(ctx, on_device, name, dtype, opts):
    """8 193 rows (two tiles and one row: every other part of the last tile is empty), a row count that ends exactly where
    part 1 of 5 begins, and one row more (a part of one row) -- under the planner's own choice and three forced ones."""
    _build_multiply_compare(ctx, on_device, name, dtype, opts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_with_the_row_permutation_on(ctx, on_device, dtype):
    """more than two tiles of rows: the index is built over the library's row permutation, the cells are whatever it makes"""
    _build_multiply_compare(ctx, on_device, "two_tiles_and_a_row", dtype, {}, permute=True)
    _build_multiply_compare(ctx, on_device, "two_tiles_and_a_row", dtype, {"SG_COLLAPSE": "0", "SG_POSTINGS_SPLIT": "5"}, permute=True)


@pytest.mark.parametrize("split", [1, 5, 8])
@pytest.mark.parametrize("terms", [1, 2, 63, 64, 65])
def test_tiny_vocabularies(ctx, on_device, terms, split):
    """1, 2, 63, 64 and 65 terms: one cell holds every row of a part (or every 2nd, 63rd ...); one packed word of counters, a
    half-used last word, one group of 64 terms, one and a bit"""
    _build_multiply_compare(ctx, on_device, f"terms_{terms}", np.float32, {"SG_POSTINGS_SPLIT": str(split)})


def _largest_part(name, split):
    c = F.case(name, np.float32)
    n = c.B.shape[0]
    assert n <= F.TILE
    return max(F.postings_of_chunk(c, min(F.part_begin(p, split), n), min(F.part_begin(p + 1, split), n)) for p in range(split))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("how", ["below_every_part", "largest_part_does_not_fit", "largest_part_just_fits"])
@pytest.mark.parametrize("split", [5, 8])
def test_stage_capacity_around_a_parts_postings(ctx, on_device, dtype, split, how):
    """SG_FILL_STAGE_CAP below every part's postings (every workgroup writes posting by posting), one below the largest
    part's (that workgroup alone does, beside staging ones) and exactly the largest part's (it just fits)"""
    largest = _largest_part("one_tile", split)
    cap = {"below_every_part": 100, "largest_part_does_not_fit": largest - 1, "largest_part_just_fits": largest}[how]
    _build_multiply_compare(ctx, on_device, "one_tile", dtype, {"SG_POSTINGS_SPLIT": str(split), "SG_FILL_STAGE_CAP": str(cap)})


@pytest.mark.parametrize("opts", [{"SG_FILL_STAGE_CAP": "4000"}, {"SG_FILL_STAGE_CAP": "4000", "SG_POSTINGS_SPLIT": "3"},
                                  {"SG_FILL_STAGED": "0", "SG_POSTINGS_SPLIT": "7"}, {"SG_POSTINGS_LAZY": "0", "SG_POSTINGS_SPLIT": "6"}],
                         ids=_id)
def test_rows_of_60_chunks_that_do_not_fit_and_the_unstaged_fill(ctx, on_device, opts):
    """Rows of 60 entries with a stage of 4 000 postings: a chunk (planned for the full stage) does not fit, every part goes
    posting by posting.  And the fill without a stage (postings_fill_lds) under a split that is no power of two."""
    _build_multiply_compare(ctx, on_device, "rows_of_60", np.float32, opts)
