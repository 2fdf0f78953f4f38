"""The inputs of tests/_fill_edge_cases.py bite: for every checked cell of every case, taking ONE posting of the cell out of
the right-hand matrix changes the port's result.  A condition of the cases, not a measurement -- no GPU, no library."""
import numpy as np
import pytest

from oracle import port as P
from tests import _fill_edge_cases as F


def _same(a, b):
    return (np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", F.CASES)
def test_every_checked_cell_decides_a_match(name, dtype):
    c = F.case(name, dtype)
    want = F.port(name, dtype, False)
    norms = np.sqrt(np.asarray(c.B.multiply(c.B).sum(axis=1), np.float64).ravel())
    assert norms.max() <= 1.0 and c.B.data.min() > 0                      # cosine-like: the pruned multiply takes it
    entries = np.diff(c.B.indptr)
    assert ((np.diff(want.indptr) > 0) == (entries > 0)).all()             # every row with entries finds itself at least
    assert len(c.checked) > 0
    for term, rows in c.checked:
        assert len(rows) > 0
        # the group's heaviest row (it survives any cut), and where nothing is cut its first, middle and last row
        heaviest = max(rows, key=lambda r: c.B[r, term])
        some = {heaviest} | ({rows[0], rows[len(rows) // 2], rows[-1]} if len(rows) <= F.TOP_N else set())
        for row in sorted(some):
            got = P.sp_matmul_topn_port(c.B, F.without_posting(c.B, row, term).T, F.TOP_N, F.THRESHOLD, True, 8)
            assert not _same(got, want), f"{name}: the posting (row {row}, term {term}) decides nothing"


def test_the_shapes_are_the_edges_they_claim():
    s5 = [F.part_begin(p, 5) for p in range(6)]
    assert s5 == [0, 768, 1600, 2432, 3264, 4096]
    assert F.case("ends_on_a_part").B.shape[0] == F.TILE + s5[1] and F.case("part_of_one_row").B.shape[0] == F.TILE + s5[1] + 1
    assert F.case("two_tiles_and_a_row").B.shape[0] == 2 * F.TILE + 1
    for split in F.SPLITS:                                                  # the sized cells lie in part 0 under every split
        assert F.part_begin(1, split) >= 512 or split == 1
        assert all(F.part_begin(p + 1, split) > F.part_begin(p, split) for p in range(split))
    one = F.case("one_tile")
    lens = np.diff(one.B.indptr)
    assert one.B.shape[1] % 2 == 1 and {0, 1, 16, 17, 64} <= set(lens.tolist())
    sizes = sorted(len(rows) for _, rows in one.checked)
    assert sizes == [10, 63, 64, 65]
    cols = np.unique(one.B.indices)
    assert cols[0] == 0 and cols[-1] == one.B.shape[1] - 1                  # the first and the last term are occupied
    assert (np.diff(F.case("rows_of_60").B.indptr) == 60).all()
    freq = F.case("frequent_everywhere").B
    assert (np.diff(freq.tocsc().indptr)[-1]) == (np.diff(freq.indptr) > 0).sum()     # the last term: in every row with entries
    for v in (1, 2, 63, 64, 65):
        assert F.case(f"terms_{v}").B.shape[1] == v and len(np.unique(F.case(f"terms_{v}").B.indices)) == v
