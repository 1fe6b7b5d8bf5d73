"""The schedule of PCG's staggered x flush (pcg_state.hpp pcg_flush_pending / pcg_block_of_tile, through
psk_lab_pcg_flush_schedule; no GPU): the one function the SpMV launches' flush role, K3, pcg_flush_kernel and the
host call. Replayed here as the loop runs it — SpMV launch k >= 1 brings block k mod S up to date, whoever ends the
solve at iteration k catches up every row — for every S the ring of p buffers supports."""
import ctypes

import pytest

from pysolvers_amd import _native as N


def _build():
    s, ring = N.I32(), N.I32()
    N.check(N.load_lab().psk_lab_pcg_stagger(ctypes.byref(s), ctypes.byref(ring)), "psk_lab_pcg_stagger")
    return s.value, ring.value


def _sched(S, nv, tile, k, in_spmv):
    blk = N.I32()
    fl = (N.I64 * 2)()
    N.check(N.load_lab().psk_lab_pcg_flush_schedule(S, nv, tile, k, 1 if in_spmv else 0, ctypes.byref(blk), fl),
            "psk_lab_pcg_flush_schedule")
    return blk.value, fl[0], fl[1]


def test_build_ties_blocks_to_ring():
    """SpMV k reads p_{k-S} after K3 k-1 has written p_k over p_{k-ring}: S < ring (0: built without)."""
    S, ring = _build()
    assert ring >= 1 and 0 <= S < ring


def _sizes(S):
    return sorted({v for v in (1, 2, S - 1, S, S + 1, 3 * S + 2, 258) if v >= 1})


def _supported():
    _, ring = _build()
    return list(range(1, ring))   # S = ring needs a buffer more than the ring has


@pytest.mark.parametrize("S", _supported())
def test_every_update_once_in_order_within_the_ring(S):
    _, ring = _build()
    for nv in _sizes(S):
        # the blocks: contiguous runs of tiles in block order; trailing blocks may own no tile (harmless: their
        # launches find nothing to serve, and no tile waits for them)
        blk_of = [_sched(S, nv, t, 0, False)[0] for t in range(nv)]
        assert blk_of[0] == 0 and all(0 <= b < S for b in blk_of)
        assert all(0 <= blk_of[t + 1] - blk_of[t] <= 1 for t in range(nv - 1))
        applied = [0] * nv   # iterations 0 .. applied[t] - 1 are in x's rows of tile t (0: never stored)
        for k in range(0, 4 * S + 4):
            if k >= 1:   # SpMV launch k: the flush role serves block k mod S
                for t in range(nv):
                    if blk_of[t] != k % S:
                        continue
                    blk, first, last = _sched(S, nv, t, k, True)
                    assert blk == k % S
                    # exactly the updates not yet applied, up to k - 1, in increasing order (a range)
                    assert (first, last) == (applied[t], k - 1), (S, nv, t, k)
                    assert 1 <= last - first + 1 <= S
                    # p_first is still in the ring: K3 k-1 wrote p_k over p_{k-ring}
                    assert first >= k - ring + 1, (S, nv, t, k)
                    applied[t] = k
            # the solve could end at this k (K3 on convergence or at maxiter - 1, pcg_flush_kernel after a
            # breakdown): every tile's catch-up range is what its block still lacks
            for t in range(nv):
                blk, first, last = _sched(S, nv, t, k, False)
                assert blk == blk_of[t]
                assert (first, last) == (applied[t], k - 1), (S, nv, t, k)   # then + alpha_k p_k: 0 .. k once each
                assert last - first + 1 <= S - 1
                assert first >= k - ring + 1
                # K3 k writes p_{k+1} into slot (k + 1) mod ring = p_{k+1-ring}'s: in no block's pending range
                assert all(j % ring != (k + 1) % ring for j in range(first, last + 1)), (S, nv, t, k)


def test_rejects_bad_arguments():
    lab = N.load_lab()
    blk, fl = N.I32(), (N.I64 * 2)()
    for S, nv, tile, k in ((0, 4, 0, 1), (3, 0, 0, 1), (3, 4, 4, 1), (3, 4, -1, 1), (3, 4, 0, -1)):
        assert lab.psk_lab_pcg_flush_schedule(S, nv, tile, k, 0, ctypes.byref(blk), fl) != 0
