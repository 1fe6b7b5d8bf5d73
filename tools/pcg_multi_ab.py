#!/usr/bin/env python3
"""psk_pcg_multi against psk_pcg, one GPU, one process (DESIGN.md §5 "Several right-hand sides").

    python tools/pcg_multi_ab.py [--side 4096] [--side3d 256] [--maxiter 50] [--rounds 5] [--out profiles/pcg_multi_ab.txt]

For each operator: A = ONE psk_pcg_multi call with nrhs = 4, B = FOUR psk_pcg calls on the same four columns, both with
the Jacobi preconditioner, tau = 0 and a fixed maxiter (failOnMaxiter = 0), so both sides run exactly maxiter iterations
per column: the same work. All vectors are device-resident (no host copies inside the timed calls). One untimed warm-up
of each side, then `rounds` rounds alternating A and B; the figure of a side is the MEDIAN over the rounds (minimum and
maximum beside it) of
  * loop_ms: the solve's own device-event interval (init to end; summed over the four calls of B), and
  * wall_ms: the host clock around the call(s), each of which ends in a device synchronise.
Operators:
  fd_csr   FDLaplacian2D(-1, 1, side) generated on the device, SpMV layout forced to CSR;
  fd_auto  the same with the automatic layout (the diagonal layout: psk_pcg's matrix stream is 1 B/row there, while
           psk_pcg_multi reads the CSR arrays whatever the layout), where the single-vector loop is expected to win;
  s27      a 27-point 3-D stencil, side3d^3 rows (diagonal 27, off-diagonal -1: kron of three tridiagonal patterns),
           uploaded from scipy, automatic layout.
Counted bytes per row, per column and iteration (arithmetic on the shapes, NOT measured): the matrix stream of the
side's layout (psk_csr_layout's stream_bytes for psk_pcg; 12 nnz + 4 (n + 1) for psk_pcg_multi) plus the vector traffic
of the kernels as they are written: psk_pcg 73 B (SpMV 8 + 8, K2 8 + 8 + 8 + DInv 8 unless uniform, K3 8 + 8 + 8 and x
deferred 9; the gathers of p counted once), psk_pcg_multi per column 8 + 8 (S) + 48 + 2 (U: x, r, p, Ap read, x, r
written, DInv shared) + 24 + 2 (P).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def stencil27(s):
    import scipy.sparse as sp
    T = sp.diags([np.ones(s - 1), np.ones(s), np.ones(s - 1)], [-1, 0, 1], format="csr")
    K = sp.kron(sp.kron(T, T, format="csr"), T, format="csr")
    K.data[:] = -1.0
    return (K + sp.identity(s ** 3, format="csr") * 28.0).tocsr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--side3d", type=int, default=256)
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ops", nargs="+", default=["fd_csr", "fd_auto", "s27"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU"
    lines = []

    def say(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    say(dict(what="command", argv=["tools/pcg_multi_ab.py"] + sys.argv[1:]))
    NR = N.PSK_PCG_MULTI_MAX

    def stream_bytes(dA):
        sb = N.I64()
        N.check(N.lib.psk_csr_layout(dA.handle, -1, None, None, None, ctypes.byref(sb)), "psk_csr_layout")
        return sb.value

    for op in args.ops:
        if op == "s27":
            dA = psk.DeviceCSR.from_scipy(stencil27(args.side3d))
        else:
            dA = psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, args.side)
            if op == "fd_csr":
                dA.set_layout("csr")
        n, nnz = dA.n, dA.nnz
        prec = psk.JacobiPreconditionerType().form(dA)
        uni = N.I32()
        N.check(N.lib.psk_prec_jacobi_uniform(prec.device_handle, ctypes.byref(uni), None), "psk_prec_jacobi_uniform")
        B = np.random.default_rng(12345).standard_normal((n, NR))
        dB, dX = psk.DeviceVector.from_numpy(B.ravel()), psk.DeviceVector(n * NR)
        db = [psk.DeviceVector.from_numpy(np.ascontiguousarray(B[:, j])) for j in range(NR)]
        dx = [psk.DeviceVector(n) for _ in range(NR)]
        del B
        ctl = N.PskCtl(maxiter=args.maxiter, tau=0.0, fail_on_maxiter=0, restart=0, check_every=0, time_kernels=0,
                       norm_b=0.0)
        rm, r1 = (N.PskResult * NR)(), N.PskResult()

        def multi():
            t0 = time.perf_counter()
            N.check(N.lib.psk_pcg_multi(dA.handle, prec.device_handle, NR, dB._p, dX._p, ctypes.byref(ctl), rm, None,
                                        N.PSK_DEVICE), "psk_pcg_multi")
            wall = (time.perf_counter() - t0) * 1e3
            assert all(rm[j].iters == args.maxiter and rm[j].hist_len == args.maxiter for j in range(NR))
            return rm[0].loop_ms, wall, [rm[j].resid for j in range(NR)]

        def singles():
            loop, resid = 0.0, []
            t0 = time.perf_counter()
            for j in range(NR):
                N.check(N.lib.psk_pcg(dA.handle, prec.device_handle, db[j]._p, dx[j]._p, ctypes.byref(ctl),
                                      ctypes.byref(r1), None, N.PSK_DEVICE), "psk_pcg")
                assert r1.iters == args.maxiter
                loop += r1.loop_ms
                resid.append(r1.resid)
            return loop, (time.perf_counter() - t0) * 1e3, resid

        wm, ws = multi(), singles()   # warm-up, and the results agree: the last residuals to rounding
        agree = max(abs(a - b) / b for a, b in zip(wm[2], ws[2]))
        tm, ts = [], []
        for _ in range(args.rounds):
            tm.append(multi()[:2])
            ts.append(singles()[:2])

        def stat(v):
            return dict(median=statistics.median(v), min=min(v), max=max(v))

        mat_multi = (12.0 * nnz + 4.0 * (n + 1)) / n
        mat_single = stream_bytes(dA) / n
        vec_single = 73.0 - (8.0 if uni.value else 0.0)
        vec_multi = 16.0 + 50.0 + 26.0
        lm, ls = stat([t[0] for t in tm]), stat([t[0] for t in ts])
        say(dict(what="result", op=op, layout=dA.layout, n=n, nnz=nnz, nrhs=NR, iterations_per_column=args.maxiter,
                 rounds=args.rounds, multi_loop_ms=lm, four_singles_loop_ms=ls,
                 multi_wall_ms=stat([t[1] for t in tm]), four_singles_wall_ms=stat([t[1] for t in ts]),
                 ratio_singles_over_multi_loop=ls["median"] / lm["median"],
                 counted_bytes_per_row_per_column=dict(multi=mat_multi / NR + vec_multi, single=mat_single + vec_single,
                                                       matrix_multi=mat_multi, matrix_single=mat_single),
                 counted_GBps=dict(multi=(mat_multi + NR * vec_multi) * n * args.maxiter / lm["median"] / 1e6,
                                   singles=(mat_single + vec_single) * NR * n * args.maxiter / ls["median"] / 1e6),
                 last_residual_rel_diff=agree))
        del dA, prec, dB, dX, db, dx
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
