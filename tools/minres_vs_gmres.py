#!/usr/bin/env python3
"""MINRES against GMRES(30), both with Jacobi, on a symmetric indefinite operator — cost per iteration.

    python tools/minres_vs_gmres.py [--side 4096] [--shift 1.5] [--iters 300] [--solvers minres gmres bicgstab] \
        [--out profiles/minres_vs_gmres.json]

The operator is the unscaled 5-point Laplacian kron(I, T) + kron(T, I), T = tridiag(-1, 2, -1), minus shift * I
(built on the host, uploaded once), b = A x for a random x, operands resident in HBM, one process. tau = 0 and a
fixed iteration count: every solver runs exactly --iters iterations (GMRES: Arnoldi steps, in cycles of --restart),
so the figure is cost per iteration, not time to solution. Per solver: one warm-up solve, then the median of
--reps solves of psk_result.loop_ms (HIP events around the solve), iterations (steps) per second, and for MINRES the
achieved bytes/s against the schedule's count per iteration: one SpMV (matrix stream of the layout in use + 16 B/row:
x and y) + 136 B/row of vector traffic in the three vector launches (minres.hip's table, Jacobi).
BiCGStab (--solvers ... bicgstab) is not a competitor on this matrix: it is run so that one kernel trace holds its
update kernels, the yardstick of the same read/write shape, beside MINRES's.
One JSON document.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def shifted_laplacian(m, shift):
    I = sp.identity(m, format="csr")
    T = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], [-1, 0, 1], format="csr")
    A = (sp.kron(I, T, format="csr") + sp.kron(T, I, format="csr") - shift * sp.identity(m * m, format="csr")).tocsr()
    A.sort_indices()
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--shift", type=float, default=1.5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solvers", nargs="+", default=["minres", "gmres"], choices=["minres", "gmres", "bicgstab"],
                    help="a subset: the run a kernel profiler wraps")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "minres_vs_gmres.json"))
    args = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N

    m = args.side
    n = m * m
    dA = psk.DeviceCSR.from_scipy(shifted_laplacian(m, args.shift))
    sb = N.I64()
    N.check(N.lib.psk_csr_layout(dA.handle, -1, None, None, None, ctypes.byref(sb)), "psk_csr_layout")
    x = psk.DeviceVector.from_numpy(np.random.default_rng(12345).random(n))
    b = psk.Linear.spmv(dA, x)
    del x
    M = psk.JacobiPreconditionerType().form(dA)
    sol = psk.DeviceVector(n)
    entry = {"side": m, "n": n, "shift": args.shift, "tau": 0.0, "iters": args.iters, "layout": dA.layout,
             "matrix_stream_bytes": sb.value, "precond": "jacobi"}

    def run(fn, restart):
        ctl = N.PskCtl(maxiter=args.iters, tau=0.0, fail_on_maxiter=1, restart=restart, check_every=0, time_kernels=0)
        res = N.PskResult()
        N.check(fn(dA.handle, M.device_handle, b._p, sol._p, ctypes.byref(ctl), ctypes.byref(res), None, N.PSK_DEVICE),
                "solve")
        return res

    for name, fn, restart in (("minres", N.lib.psk_minres, 0), ("gmres", N.lib.psk_gmres, args.restart),
                              ("bicgstab", N.lib.psk_bicgstab, 0)):
        if name not in args.solvers:
            continue
        run(fn, restart)                                   # warm-up
        rs = [run(fn, restart) for _ in range(args.reps)]
        ms = statistics.median(r.loop_ms for r in rs)
        r = rs[-1]
        its = int(r.iters) + (1 if r.status == N.PSK_MAXITER else 0)   # iterations run (maxiter reports k)
        e = {"iters": its, "status": N.STATUS_NAMES[r.status], "spmv_launches": int(r.spmv_launches),
             "loop_ms_median": ms, "loop_ms_all": [float(q.loop_ms) for q in rs], "iters_per_s": its / (ms * 1e-3),
             "us_per_iter": ms * 1e3 / max(its, 1), "resid_over_normb": float(r.resid / r.norm_b)}
        if name == "minres":
            per_iter = (sb.value + 16 * n) + 136 * n
            e["schedule_bytes_per_iter"] = per_iter
            e["achieved_bytes_per_s"] = per_iter * its / (ms * 1e-3)
        if name == "gmres":
            e["restart"] = restart
        entry[name] = e
    print(json.dumps(entry), flush=True)
    with open(args.out, "w") as f:
        json.dump(entry, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
