"""The rank blocks of the self-join form (``distributed.RankBlock``, ``distributed.SelfJoinPart``) on the device, three ranks
played one after the other on one context: every layout -- index in row order or over the library's row permutation,
contiguous ranges or interleaved shares, identical rows grouped or not -- gives blocks whose ``rows`` say where their rows
belong, and every device list the library hands out is an owned handle: ``_native.live_handles()`` comes back to where it
was after the blocks are freed, after a discarded range, after a refused range and after an exception between range and
merge.  (Before the lists were handles, a leaked list was a bare integer that nothing could count.)

Input: 9 600 synthetic names and 100 repeats of five of them (groups of more than one row; rows whose top-n is cut).  The
library leaves an index of at most two tiles of rows (8 192 by default) in row order, so a smaller column has no permuted
layout to test; the names -- and, grouped, their some 8 500 distinct rows -- are more than that."""
import gc

import numpy as np
import pytest

from oracle import oracle as O
from oracle import port as P
from string_grouper_amd import distributed as D
from string_grouper_amd.synth import synth_names
from tests._numpy_ops import GroupedIndex, NumpyOps
from tests.test_multiply_threshold_gpu import _assemble, assert_identical

SEED = 77            # (with it every share of every layout publishes pairs: shares_without_pairs() == [], checked below)
N_BASE, REPEATS, WORLD, TOP_N, THR = 9600, 100, 3, 10, 0.75
LAYOUTS = [(permute, interleave, collapse) for collapse in ("0", "1") for permute in (False, True) for interleave in (False, True)]


def names_of(seed=SEED):
    base = synth_names(N_BASE, seed)
    return base + [base[k] for k in (3, 11, 500, 4000, 8000)] * (REPEATS // 5)


def shares_of(n_index, interleave):
    if interleave:
        return [(0, n_index - r, WORLD) for r in range(WORLD)]          # what selfjoin_share deals by default
    b = D.selfjoin_row_ranges(n_index, WORLD)
    return [(int(b[r]), int(b[r + 1]), 1) for r in range(WORLD)]


def shares_without_pairs(A, want):
    """The (layout, rank) whose share would publish no mirrored pair: none of its index rows i has a match j of ``want``
    (the port's top-n) at a lower position.  Host only: positions by the library's formula (NumpyOps.permutation), groups
    numbered by their lowest member (GroupedIndex)."""
    n = A.shape[0]
    gid_grouped = GroupedIndex(A).gid
    i_of = np.repeat(np.arange(n), np.diff(want.indptr))
    missing = []
    for permute, interleave, collapse in LAYOUTS:
        gid = gid_grouped if collapse == "1" else np.arange(n)
        n_index = int(gid.max()) + 1
        pos_of = NumpyOps.permutation(n_index)[1] if permute else np.arange(n_index)
        pi, pj = pos_of[gid[i_of]], pos_of[gid[want.indices]]
        publishing = np.unique(pi[pj < pi])                             # positions whose row publishes a pair
        for r, share in enumerate(shares_of(n_index, interleave)):
            if not np.isin(D.share_positions(*share), publishing).any():
                missing.append((permute, interleave, collapse, r))
    return missing


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_blocks_name_their_rows_and_own_their_lists(ctx, dtype, monkeypatch):
    import torch
    from string_grouper_amd import _native as N
    from string_grouper_amd.vectorizer import HipTfidfVectorizer
    names = names_of()
    n = len(names)
    (A,), _, _ = O.tfidf_sklearn(names, [names], dtype=dtype)
    want = P.sp_matmul_topn_port(A, A.T, TOP_N, THR, True, 8)
    assert shares_without_pairs(A, want) == []          # the condition on the input, before anything runs on the device
    ops = D.HipOps(ctx, lambda: HipTfidfVectorizer(dtype=dtype, ctx=ctx))
    dA = ctx.csr_from_scipy(A)
    for permute, interleave, collapse in LAYOUTS:
        what = f"permute={permute} interleave={interleave} collapse={collapse}"
        ctx.set_option("SG_COLLAPSE", collapse)
        live = N.live_handles()
        post = ctx.postings_build(dA, permute=permute)
        n_index, n_caller, p_gid = ctx.postings_rows(post)
        assert n_caller == n and bool(p_gid) == (collapse == "1") and (n_index < n) == (collapse == "1"), what
        p_orig, _ = ctx.postings_permutation(post)
        assert bool(p_orig) == permute, what
        orig_of = (torch.as_tensor(D.DeviceTensorView(p_orig, n_index, "<i4"), device=ops.device).cpu().numpy().astype(np.int64)
                   if permute else np.arange(n_index))
        shares = shares_of(n_index, interleave)
        with_index = N.live_handles()
        # a range the form refuses (top_n > 64) gives None and leaves nothing behind
        assert ops.selfjoin_range(dA, post, 65, THR, *shares[0]) is None and N.live_handles() == with_index, what
        # a range alone, discarded
        part = ops.selfjoin_range(dA, post, TOP_N, THR, *shares[1])
        assert part is not None and N.live_handles() > with_index, what
        ops.selfjoin_discard(part)
        assert N.live_handles() == with_index, what
        # an exception between range and merge: the part takes its lists with it
        part = ops.selfjoin_range(dA, post, TOP_N, THR, *shares[2])
        pairs = ops.selfjoin_pairs(part).clone()
        with monkeypatch.context() as m:
            def refuse(*args, **kwargs):
                raise ValueError("injected before the library is called")
            m.setattr(N.Context, "selfjoin_merge", refuse)
            with pytest.raises(ValueError, match="injected"):
                ops.selfjoin_merge(part, pairs, *shares[2])
        del part
        gc.collect()
        assert N.live_handles() == with_index, what
        # the three ranks
        parts = [ops.selfjoin_range(dA, post, TOP_N, THR, *sh) for sh in shares]
        assert all(p is not None and len(p.pairs) > 0 and len(p.pairs) % p.words == 0 for p in parts), what
        pairs_all = torch.cat([ops.selfjoin_pairs(p).clone() for p in parts])
        blocks = [ops.selfjoin_merge(parts[r], pairs_all, *shares[r]) for r in range(WORLD)]
        rows = [b.rows.cpu().numpy() for b in blocks]
        assert all(r.dtype == np.int64 and b.dims()[0] == len(r) for r, b in zip(rows, blocks)), what
        assert np.array_equal(np.sort(np.concatenate(rows)), np.arange(n)), what              # a partition of the rows
        if collapse == "0":
            for r in range(WORLD):
                assert np.array_equal(rows[r], orig_of[D.share_positions(*shares[r])]), f"{what} rank {r}"
        assert_identical(_assemble(blocks, n, TOP_N, dtype, n), want, what)
        for h in blocks + [post]:
            h.free()
        assert N.live_handles() == live, what
    dA.free()
