"""Every form of the top-n multiply (tests/_threshold_cases.py: FORMS) on inputs whose scores sit exactly at the threshold
and at the cut, compared BIT FOR BIT with the oracle's port: shape, indptr, indices, dtype and data are equal or the test
fails; no tolerance anywhere.  The two rules under test: a pair is a match when its score is STRICTLY greater than the
threshold; a row keeps its best top_n by score descending, then column ascending.

  ladder   power-of-two entries: thousands of pairs score exactly each threshold, hundreds of rows are cut inside a block of
           equal scores between DISTINCT rows that lie in different tiles and super-tiles of the index;
  long     the same with rows of 112 entries (the wide launch) and a few of 256 (the exact kernel inside a pruned pass);
  names    the parity tests' 20 000 names with thresholds made from their own scores: s and the number below s, and for
           float32 doubles between the two.

Each form is forced with context options at any size and must PROVE from ctx.stats() that it ran before its result counts.
Each runs four ways -- identical rows grouped or not (SG_COLLAPSE), the index over the library's row permutation or in row
order -- and the forms that can be one-sided also as a true one-sided product (a slice of the rows uploaded as a matrix of
its own).  tests/test_threshold_cases_cpu.py shows without a GPU that the port's answer on these inputs is the arithmetic
one and that `>=` for `>`, or arrival order for column order, changes it."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import _threshold_cases as T

pytestmark = pytest.mark.gpu

CASES = ("ladder", "long", "names")


def schedule(form: T.Form, case: str, dtype):
    """[(top_n, thr, sort)] of a form on a case.  Forms without cuts of their own take cuts up to 64 (one register list,
    one pass of the exact kernel); 65 .. 128 and 129+ belong to the forms that are about them."""
    out = []
    if case == "ladder":
        for t in T.LADDER_THRESHOLDS:
            full = t in T.FULL_CUT_THRESHOLDS
            if form.cuts is not None:
                cuts = form.cuts if full else ()
            else:
                cuts = [c for c in T.CUTS if c <= 64] if full else T.CUTS_EVERYWHERE
            out += [(c, thr, True) for thr in (t, T.pred(t, dtype)) for c in cuts]
        out.append(((form.cuts or T.CUTS_EVERYWHERE)[0], T.pred(0.75, dtype), False))
    elif case == "long":
        # (the forms about cuts beyond 64: up to 0.625 -- at 0.75, with identical rows grouped, no list comes out full)
        cuts = form.cuts[::3] if form.cuts is not None else T.LONG_CUTS[:2]
        thresholds = T.LONG_THRESHOLDS[:2] if form.cuts is not None else T.LONG_THRESHOLDS
        out += [(c, thr, True) for t in thresholds for thr in (t, T.pred(t, dtype)) for c in cuts]
        out.append((cuts[0], T.pred(T.LONG_THRESHOLDS[1], dtype), False))
    else:
        top_n = form.cuts[0] if form.cuts is not None else T.NAME_TOP_N
        thresholds = [nt.thr for nt in T.name_thresholds(dtype) if nt.thr <= form.max_name_thr]
        out += [(top_n, thr, True) for thr in thresholds]
        out.append((top_n, thresholds[-1], False))
    return out


def assert_identical(got: sp.csr_matrix, want: sp.csr_matrix, what: str):
    assert got.shape == want.shape, what
    gp, wp = np.asarray(got.indptr, np.int64), np.asarray(want.indptr, np.int64)
    if not np.array_equal(gp, wp):
        rows = np.flatnonzero(np.diff(gp) != np.diff(wp))
        r = int(rows[0])
        raise AssertionError(f"{what}: {len(rows)} rows differ in their number of matches, first row {r}: "
                             f"got {np.diff(gp)[r]} {got.data[gp[r]:gp[r + 1]][-3:]}, want {np.diff(wp)[r]} {want.data[wp[r]:wp[r + 1]][-3:]}")
    assert got.data.dtype == want.data.dtype, what
    if not (np.array_equal(got.indices, want.indices) and np.array_equal(got.data, want.data)):
        bad = (got.indices != want.indices) | (got.data != want.data)
        rows = np.unique(np.searchsorted(gp, np.flatnonzero(bad), side="right") - 1)
        r = int(rows[0])
        raise AssertionError(f"{what}: {len(rows)} rows differ, first row {r}:\n got  {got.indices[gp[r]:gp[r + 1]]} {got.data[gp[r]:gp[r + 1]]}\n"
                             f" want {want.indices[gp[r]:gp[r + 1]]} {want.data[gp[r]:gp[r + 1]]}")


def products(ctx, form: T.Form, case: str, dtype, ways=(("0", True), ("0", False), ("1", True), ("1", False))):
    """Run the form's schedule the four ways; yields (what, proof holds, stats, info, got, want) per multiply."""
    A = T.matrix(case, dtype)
    sched = schedule(form, case, dtype)
    n_long = int((np.diff(A.indptr) > 128).sum())
    for collapse, permute in ways:
        ctx.reset_options()
        for k, v in {**form.build, **form.run, "SG_COLLAPSE": collapse}.items():
            ctx.set_option(k, v)
        if collapse == "1":
            ctx.set_option("SG_COLLAPSE_LEFT", "1")        # identical LEFT rows of the one-sided product grouped as well
        dA = ctx.csr_from_scipy(A)
        post = ctx.postings_build(dA, permute=permute)
        n_index, n_caller, _ = ctx.postings_rows(post)
        assert n_caller == A.shape[0]
        assert (n_index < n_caller) == (collapse == "1") and (n_index == n_caller) == (collapse == "0")   # every case repeats rows
        assert n_index > 2 * T.TILE_ROWS and (ctx.postings_permutation(post)[0] != 0) == permute
        lefts = [(None, dA, A.shape[0])]
        if not form.self_join:
            rows = T.LEFT_SLICE[case]
            lefts.append((rows, ctx.csr_from_scipy(A[rows]), rows.stop - rows.start))
        for rows, dL, n_left in lefts:
            long_left = n_long if rows is None else int((np.diff(A[rows].indptr) > 128).sum())
            for top_n, thr, sort in sched:
                res = ctx.spgemm_topn(dL, post, top_n, thr, sort)
                st = ctx.stats()
                got = res.to_scipy()
                res.free()
                info = dict(n=n_index if rows is None else n_left, n_left=n_left, long_rows=long_left, top_n=top_n, thr=thr)
                what = (f"{form.name} {case} {np.dtype(dtype).name} SG_COLLAPSE={collapse} permute={permute} "
                        f"{'self-product' if rows is None else 'one-sided slice'} top_n={top_n} thr={thr!r} sort={sort}")
                yield what, bool(form.proof(st, info)), st, info, got, T.port(case, dtype, top_n, thr, sort, 0, rows)
        for _, dL, _ in lefts[1:]:
            dL.free()
        post.free()
        dA.free()


@pytest.mark.parametrize("dtype", T.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name,case", [(f.name, c) for f in T.FORMS for c in CASES if c in f.cases])
def test_form_equals_the_port_at_the_threshold_and_the_cut(ctx, name, case, dtype):
    """One line of FORMS on one case: every ladder threshold t with thr = t (the pairs at t are no matches) and thr = the
    number below t (they are, by one ulp), cuts 5 and 64 at all of them and every cut of the form's range at 0.4375 and 0.75;
    the long rows at 0.5 / 0.625 / 0.75; the names at thresholds made from their own scores; sort=False once.  Four ways
    (rows grouped or not, row permutation or not), the one-sided forms also with a slice of the rows as the left matrix.
    Two combinations are left out because the shapes cannot reach them, whatever the switches: the second filter on the
    long rows (rows beyond 60 entries have no 8-bit copy: nothing for it to reject, so nothing to prove it ran), and full
    lists handed on among the names above 0.45 (no row there has 64 matches)."""
    form = T.form(name)
    n = 0
    for what, proved, st, info, got, want in products(ctx, form, case, dtype):
        keys = ("prune_rows", "prune_symmetric", "exact_rows", "prune_survivors", "prune_scored")
        assert proved, f"{what}: another form ran: { {k: st[k] for k in keys} } {info}"      # FIRST: which form ran
        assert_identical(got, want, what)
        n += 1
    assert n >= 4 * len(schedule(form, case, dtype))


def _assemble(blocks, n, stride, dtype, n_cols):
    """The ranks' blocks put together on the host: every block names the caller's row of each of its rows."""
    cols = np.zeros((n, stride), np.int32)
    vals = np.zeros((n, stride), dtype)
    cnt = np.full(n, -1, np.int32)
    for b in blocks:
        c, v, k = b.to_host()
        ids = b.rows.cpu().numpy()
        assert (cnt[ids] == -1).all(), "a row in two blocks"
        cols[ids], vals[ids], cnt[ids] = c, v, k
    assert (cnt >= 0).all(), "a row in no block"
    mask = np.arange(stride)[None, :] < cnt[:, None]
    return sp.csr_matrix((vals[mask], cols[mask], np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])), shape=(n, n_cols))


@pytest.mark.parametrize("dtype", T.DTYPES, ids=lambda d: np.dtype(d).name)
def test_row_ranges_of_the_selfjoin_form_on_the_ladder(ctx, dtype):
    """sg_selfjoin_range / sg_selfjoin_merge with three ranks played one after the other: three contiguous ranges and three
    interleaved shares, top_n 10 and 64 at the number below 0.75 (pairs at exactly 0.75 are matches by one ulp; hundreds
    of rows are cut inside a block of equal scores), the ranks' pair lists concatenated in rank order and with every record
    in REVERSE order -- the merge must select by score and column, not by arrival.  The rows put together are the port's."""
    import torch
    from string_grouper_amd import distributed as D
    from string_grouper_amd.vectorizer import HipTfidfVectorizer
    A = T.ladder(dtype)
    n = A.shape[0]
    thr = T.pred(0.75, dtype)
    ops = D.HipOps(ctx, lambda: HipTfidfVectorizer(dtype=dtype, ctx=ctx))
    ctx.set_option("SG_COLLAPSE", "0")
    dA = ctx.csr_from_scipy(A)
    world = 3
    bounds = D.selfjoin_row_ranges(n, world)
    for permute in (True, False):
        post = ctx.postings_build(dA, permute=permute)
        assert ctx.postings_rows(post) == (n, n, 0)
        layouts = {"contiguous": [(int(bounds[r]), int(bounds[r + 1]), 1) for r in range(world)],
                   "interleaved": [(0, n - r, world) for r in range(world)]}
        for top_n in (10, 64):
            want = T.port("ladder", dtype, top_n, thr)
            for layout, shares in layouts.items():
                for reverse in (False, True):
                    parts = [ops.selfjoin_range(dA, post, top_n, thr, *sh) for sh in shares]
                    assert all(p is not None for p in parts), "the self-join form did not take the range"
                    assert ctx.stats()["prune_symmetric"] == 1 and ctx.stats()["prune_rows"] > 0
                    words = parts[0].words
                    pairs_all = torch.cat([ops.selfjoin_pairs(p).clone() for p in parts])
                    assert pairs_all.numel() > 0 and pairs_all.numel() % words == 0
                    if reverse:
                        pairs_all = pairs_all.view(-1, words).flip(0).contiguous().view(-1)
                    blocks = [ops.selfjoin_merge(parts[r], pairs_all, *shares[r]) for r in range(world)]
                    got = _assemble(blocks, n, min(top_n, n), dtype, n)
                    for b in blocks:
                        b.free()
                    assert_identical(got, want, f"{layout} top_n={top_n} reverse={reverse} permute={permute}")
        post.free()
    dA.free()
