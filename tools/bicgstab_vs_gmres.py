#!/usr/bin/env python3
"""BiCGStab against GMRES(30), both with Jacobi, on convection-diffusion operators — time to solution.

    python tools/bicgstab_vs_gmres.py [--sides 2048 4096] [--c 0.2] [--tau 1e-6] [--maxiter 3000] \
        [--solvers bicgstab gmres] [--out profiles/bicgstab_vs_gmres.json]

The operator is cd m: kron(I, tridiag(-1-c, 2, -1+c)) + kron(tridiag(-1, 2, -1), I) (built on the host, uploaded
once), b = A x for a random x, operands resident in HBM, one process. Per solver: one warm-up solve, then the
median of 5 solves of psk_result.loop_ms (HIP events around the solve). Reported per solver: iterations, SpMV
launches, time to solution, iterations/s, whether it converged within maxiter, and for BiCGStab the achieved
bytes/s against the schedule's count per iteration: 2 SpMVs (matrix stream of the layout in use + 32 B/row: x, y,
q and DInv) + 128 B/row of vector traffic in the four vector launches (bicgstab.hip's table, Jacobi).
One JSON document: a list with one entry per side.
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


def cd_matrix(m, c):
    I = sp.identity(m, format="csr")
    T1 = sp.diags([np.full(m - 1, -1.0 - c), np.full(m, 2.0), np.full(m - 1, -1.0 + c)], [-1, 0, 1], format="csr")
    T2 = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], [-1, 0, 1], format="csr")
    A = (sp.kron(I, T1, format="csr") + sp.kron(T2, I, format="csr")).tocsr()
    A.sort_indices()
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--c", type=float, default=0.2)
    ap.add_argument("--tau", type=float, default=1e-6)
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solvers", nargs="+", default=["bicgstab", "gmres"], choices=["bicgstab", "gmres"],
                    help="one solver alone: the run a kernel profiler wraps")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bicgstab_vs_gmres.json"))
    args = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N

    doc = []
    for m in args.sides:
        n = m * m
        dA = psk.DeviceCSR.from_scipy(cd_matrix(m, args.c))
        sb = N.I64()
        N.check(N.lib.psk_csr_layout(dA.handle, -1, None, None, None, ctypes.byref(sb)), "psk_csr_layout")
        x = psk.DeviceVector.from_numpy(np.random.default_rng(12345).random(n))
        b = psk.Linear.spmv(dA, x)
        del x
        M = psk.JacobiPreconditionerType().form(dA)
        sol = psk.DeviceVector(n)
        entry = {"side": m, "n": n, "c": args.c, "tau": args.tau, "maxiter": args.maxiter, "layout": dA.layout,
                 "matrix_stream_bytes": sb.value, "precond": "jacobi"}

        def run(fn, restart):
            ctl = N.PskCtl(maxiter=args.maxiter, tau=args.tau, fail_on_maxiter=1, restart=restart, check_every=0,
                           time_kernels=0)
            res = N.PskResult()
            N.check(fn(dA.handle, M.device_handle, b._p, sol._p, ctypes.byref(ctl), ctypes.byref(res), None,
                       N.PSK_DEVICE), "solve")
            return res

        for name, fn, restart in (("bicgstab", N.lib.psk_bicgstab, 0), ("gmres", N.lib.psk_gmres, args.restart)):
            if name not in args.solvers:
                continue
            run(fn, restart)                                   # warm-up
            rs = [run(fn, restart) for _ in range(args.reps)]
            ms = statistics.median(r.loop_ms for r in rs)
            r = rs[-1]
            its = int(r.iters) + (1 if r.status == N.PSK_MAXITER else 0)   # iterations run (maxiter reports k)
            e = {"iters": its, "status": N.STATUS_NAMES[r.status], "converged": bool(r.success),
                 "spmv_launches": int(r.spmv_launches), "loop_ms_median": ms,
                 "loop_ms_all": [float(q.loop_ms) for q in rs], "iters_per_s": its / (ms * 1e-3),
                 "resid_over_normb": float(r.resid / r.norm_b)}
            if name == "bicgstab":
                per_iter = 2 * (sb.value + 32 * n) + 128 * n
                e["schedule_bytes_per_iter"] = per_iter
                e["achieved_bytes_per_s"] = per_iter * its / (ms * 1e-3)
            else:
                e["restart"] = restart
            entry[name] = e
        if len(args.solvers) == 2:
            entry["bicgstab_faster_to_solution"] = (
                entry["bicgstab"]["converged"] and
                (not entry["gmres"]["converged"] or
                 entry["bicgstab"]["loop_ms_median"] < entry["gmres"]["loop_ms_median"]))
        print(json.dumps(entry), flush=True)
        doc.append(entry)
        del dA, M, b, sol
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
