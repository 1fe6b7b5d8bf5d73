"""The workspace layouts of psk_pcg, psk_gmres, psk_bicgstab and psk_vcycle (solve_loop.hpp Carve, through psk_lab_solver_layout;
no GPU). Each solver sizes its buffers and carves its pointers with one layout function; here every offset is
recomputed from the formulas the solvers used before that (one chain of 256-byte-rounded terms for the size, a
second one for the pointers), written out independently.

Offsets must be equal to those, 256-aligned (the V-cycle's history, which follows its 64-byte state directly so
that one copy reads both, is the stated exception) and increasing by at least the extent of the region before:
strictly increasing wherever that extent is not zero (at n = 0 the parent's vectors share an offset too). The last
region ends within the reported size."""
import ctypes
import itertools

import pytest

from pysolvers_amd import _native as N

PCG, GMRES, VCYCLE, BICGSTAB = 0, 1, 2, 3
GEN, OWN_X, DEV_IO = 1, 2, 4
MAX_GRID = 2048          # kMaxGrid
STATE = 256              # sizeof(PcgState) (80) and sizeof(GmresState) (64) rounded up to 256
VC_STATE = 64            # sizeof(VcState)
BICG_STATE = 112         # sizeof(BicgState): 6 int32, 2 int64, 7 doubles, a pointer, an int64
VC_TICK = 65 * 64 * 4    # (kVcGroups + 1) counters, one per 256-byte line


def up(v, a=256):
    return (v + a - 1) // a * a


def layout(solver, n=0, ncols=0, maxiter=0, restart=0, flags=0, P=1):
    off = (N.I64 * 64)()
    cnt = N.I32(64)
    nbytes = (N.I64 * 2)()
    N.check(N.load_lab().psk_lab_solver_layout(solver, n, ncols, maxiter, restart, flags, P, off, ctypes.byref(cnt),
                                               nbytes), "psk_lab_solver_layout")
    return [off[i] for i in range(cnt.value)], [nbytes[0], nbytes[1]]


def check(offs, extents, size, unaligned=()):
    """offs / extents of one buffer, in layout order"""
    assert len(offs) == len(extents)
    for i, o in enumerate(offs):
        assert o % 256 == 0 or i in unaligned, (i, o)
    for i in range(len(offs) - 1):
        assert offs[i + 1] >= offs[i] + extents[i], (i, offs)
        assert extents[i] == 0 or offs[i + 1] > offs[i]
    assert offs[-1] + extents[-1] <= size, (offs, extents, size)


def _defer():
    s, ring = N.I32(), N.I32()
    N.check(N.load_lab().psk_lab_pcg_stagger(ctypes.byref(s), ctypes.byref(ring)), "psk_lab_pcg_stagger")
    return ring.value


@pytest.mark.parametrize("gen,own_x,P", list(itertools.product((0, 1), (0, 1), (1, 3))))
def test_pcg_layout(gen, own_x, P):
    defer = _defer()
    for n, maxiter in itertools.product((0, 1, 511, 512, 513), (0, 1, 100)):
        ncols = n + 37
        offs, size = layout(PCG, n=n, ncols=ncols, maxiter=maxiter, flags=gen * GEN + own_x * OWN_X, P=P)
        # the large workspace: r, Ap, [x], then p (general: p and u; otherwise the ring of kPcgDefer)
        vec, vecc = up(n * 8), up(ncols * 8)
        big = (2 + own_x + gen) * vec + (1 if gen else defer) * vecc
        want = [0, vec] + ([2 * vec] if own_x else [])
        ext = [n * 8] * len(want)
        pb = (2 + own_x) * vec
        if gen:
            want += [pb, pb + vecc]
            ext += [ncols * 8, n * 8]
        else:
            want += [pb + t * vecc for t in range(defer)]
            ext += [ncols * 8] * defer
        nbig = len(want)
        assert offs[:nbig] == want, (n, maxiter, offs, want)
        assert size[0] == (big if big > 0 else 256)
        check(offs[:nbig], ext, size[0])
        # the small one: state, part1, part3, part2, udr, hist, alphas, pinit, [part1g, part2g, initg]
        ext = [80, MAX_GRID * 8, MAX_GRID * 8, 2 * MAX_GRID * 8, (maxiter + 2) * 8, (maxiter + 1) * 8, (maxiter + 1) * 8,
               256]
        small = STATE + 2 * up(MAX_GRID * 8) + up(2 * MAX_GRID * 8) + up((maxiter + 2) * 8) + 2 * up((maxiter + 1) * 8) + 256
        if P > 1:
            ext += [P * 8, P * 16, P * 16]
            small += up(P * 8) + 2 * up(P * 16)
        want, s = [], 0
        for e in ext:
            want.append(s)
            s += up(e)
        assert offs[nbig:] == want, (n, maxiter, offs[nbig:], want)
        assert size[1] == small == s
        check(offs[nbig:], ext, size[1])


@pytest.mark.parametrize("gen,restart,maxiter", list(itertools.product((0, 1), (0, 5), (1, 40))))
def test_gmres_layout(gen, restart, maxiter):
    for n in (0, 1, 511, 512, 513):
        offs, size = layout(GMRES, n=n, maxiter=maxiter, restart=restart, flags=gen * GEN)
        K = restart if restart > 0 else maxiter
        K = max(1, min(K, maxiter))
        ld = K + 1
        vec = up(n * 8)
        qbytes = vec * (K + 1)
        want = [0, qbytes, qbytes + vec, qbytes + 2 * vec] + ([qbytes + 3 * vec, qbytes + 4 * vec] if gen else [])
        ext = [qbytes] + [n * 8] * (len(want) - 1)
        nbig = len(want)
        assert offs[:nbig] == want, (n, offs, want)
        assert size[0] == qbytes + (5 if gen else 3) * vec
        check(offs[:nbig], ext, size[0])
        hb =up(ld * K * 8)
        ext = [64, ld * K * 8, ld * K * 8, 2 * K * 8, ld * 8, MAX_GRID * 8, (maxiter + 1) * 8, ld * 8, (K + 2) * 8]
        small = STATE + 2 * hb + up(2 * K * 8) + up(ld * 8) + up(MAX_GRID * 8) + up((maxiter + 1) * 8) + up(ld * 8) + \
            up((K + 2) * 8)
        want, s = [], 0
        for e in ext:
            want.append(s)
            s += up(e)
        assert offs[nbig:] == want, (n, offs[nbig:], want)
        assert size[1] == small == s
        check(offs[nbig:], ext, size[1])


@pytest.mark.parametrize("dev_io", (0, 1))
def test_vcycle_layout(dev_io):
    for n, maxiter in itertools.product((1, 511, 512, 513), (1, 31, 32, 100)):
        offs, size = layout(VCYCLE, n=n, maxiter=maxiter, flags=dev_io * DEV_IO)
        off_hist = VC_STATE
        off_tick = up(off_hist + maxiter * 8)
        off_b = off_tick + VC_TICK
        vec = up(n * 8)
        want = [0, off_hist, off_tick] + ([] if dev_io else [off_b, off_b + vec])
        ext = [VC_STATE, maxiter * 8, VC_TICK] + ([] if dev_io else [n * 8, n * 8])
        assert offs == want, (n, maxiter, offs, want)
        assert size == [off_b + (0 if dev_io else 2 * vec), 0]
        # the history follows the state directly: the solve's final copy reads both as one range
        assert offs[1] == offs[0] + VC_STATE
        check(offs, ext, size[0], unaligned=(1,))


@pytest.mark.parametrize("gen", (0, 1))
def test_bicgstab_layout(gen):
    for n, maxiter in itertools.product((0, 1, 511, 512, 513), (0, 1, 100)):
        offs, size = layout(BICGSTAB, n=n, maxiter=maxiter, flags=gen * GEN)
        # the large workspace: bv, x, r, p, v, s, t, then ph and sh for a general preconditioner
        vec, nbig = up(n * 8), 9 if gen else 7
        want = [i * vec for i in range(nbig)]
        assert offs[:nbig] == want, (n, maxiter, offs, want)
        assert size[0] == (nbig * vec if n > 0 else 256)
        check(offs[:nbig], [n * 8] * nbig, size[0])
        # the small one: the state, the 8 sums, the history (one entry more than maxiter)
        ext = [BICG_STATE, 64, (maxiter + 1) * 8]
        assert offs[nbig:] == [0, 256, 512], (n, maxiter, offs[nbig:])
        assert size[1] == 512 + up((maxiter + 1) * 8)
        check(offs[nbig:], ext, size[1])


def test_rejects_bad_arguments():
    lab = N.load_lab()
    off, cnt, nbytes = (N.I64 * 64)(), N.I32(64), (N.I64 * 2)()
    assert lab.psk_lab_solver_layout(4, 1, 1, 1, 0, 0, 1, off, ctypes.byref(cnt), nbytes) != 0
    assert lab.psk_lab_solver_layout(PCG, -1, 1, 1, 0, 0, 1, off, ctypes.byref(cnt), nbytes) != 0
    assert lab.psk_lab_solver_layout(PCG, 1, 1, 1, 0, 0, 0, off, ctypes.byref(cnt), nbytes) != 0
    cnt = N.I32(2)
    assert lab.psk_lab_solver_layout(PCG, 1, 1, 1, 0, 0, 1, off, ctypes.byref(cnt), nbytes) != 0


def test_gmres_workspace_view_rejects_bad_arguments():
    """psk_lab_gmres_internals / psk_lab_gmres_prefill carve a matrix's buffers with the layout above; without a
    matrix (or with a negative size) they return PSK_ERR_ARG before any GPU call."""
    lab = N.load_lab()
    none = [None] * 7
    assert lab.psk_lab_gmres_internals(None, 10, 0, 0, 1, *none) == N.PSK_ERR_ARG
    assert lab.psk_lab_gmres_prefill(None, 10, 0, 0, 0) == N.PSK_ERR_ARG
