#!/usr/bin/env python3
"""Multicolour Gauss-Seidel measurements on the 2-D Laplacian stencil, one GPU (DESIGN.md "Multicolour Gauss-Seidel").

    python tools/mcgs_ab.py [--sides 2048 4096] [--amg-side 2048] [--regions 5] [--out profiles/mcgs_ab.txt]

Each side m means -FDLaplacian2D(-1, 1, m) (positive definite, uploaded from scipy). From ONE process it reports

* PCG to tau = 1e-8 on b = A rand(seed 12345): iterations, iterations per second and time to solution (psk_result's
  loop_ms, device events) for Jacobi, Chebyshev(2), FSAI(1) and MulticolorGS with 1 and 2 symmetric sweeps, and the
  set-up time of each (host clock around the constructor, which ends in a device synchronise);
* apply: psk_prec_apply of MulticolorGS (1 symmetric sweep) on device vectors (host clock around `apply-reps` calls,
  each of which synchronises), beside two psk_spmv calls on A measured the same way — the floor a symmetric sweep on
  two colours (1.5 streams of A, two gathers of z) cannot beat by much — and beside psk_spmv_timed of A (device events
  around back-to-back launches, no host in the interval);
* on --amg-side: one AMG apply (numIters 2, 5 levels) with the Gauss-Seidel, Chebyshev(2) and multicolour smoothers.

Every timing is the median of `regions` repetitions after one untimed warm-up, with the minimum and maximum. The
output file is written line by line, so a run that is cut short keeps what it measured.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--amg-side", type=int, default=2048)
    ap.add_argument("--amg-levels", type=int, default=5)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--apply-reps", type=int, default=20)
    ap.add_argument("--maxiter", type=int, default=40000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import (AMGPreconditioner, ChebyshevPreconditioner, ChebyshevSmoother, FSAIPreconditioner,
                                      GaussSeidelSmoother, JacobiPreconditioner, MulticolorGSPreconditioner,
                                      MulticolorGaussSeidelSmoother)
    assert N.device_count() >= 1, "no GPU"
    out = open(args.out, "w") if args.out else None

    def say(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    # the settings that shape the measurement; where the lines are written to is not one of them
    say(dict(what="command", tool="tools/mcgs_ab.py", sides=args.sides, amg_side=args.amg_side,
             amg_levels=args.amg_levels, regions=args.regions, apply_reps=args.apply_reps, maxiter=args.maxiter))

    def sync():
        N.check(N.lib.psk_synchronize(), "psk_synchronize")

    def med(f, reps=1):
        f()
        sync()
        ts = []
        for _ in range(args.regions):
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            sync()
            ts.append((time.perf_counter() - t0) * 1e3 / reps)
        return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))

    def pcg(dA, M, bd, xd):
        c = N.PskCtl(maxiter=args.maxiter, tau=1e-8, fail_on_maxiter=1, restart=0, check_every=0, time_kernels=0,
                     norm_b=0.0)
        res = N.PskResult()
        N.check(N.lib.psk_pcg(dA.handle, M.device_handle, bd._p, xd._p, ctypes.byref(c), ctypes.byref(res), None,
                              N.PSK_DEVICE), "psk_pcg")
        return res

    def solve(dA, M, bd, xd):
        ms, its, ok = [], None, None
        pcg(dA, M, bd, xd)
        for _ in range(args.regions):
            res = pcg(dA, M, bd, xd)
            ms.append(res.loop_ms)
            its, ok = int(res.iters), bool(res.success)
        t = statistics.median(ms)
        return dict(iters=its, converged=ok, solve_ms=t, solve_min_max_ms=[min(ms), max(ms)],
                    iters_per_s=its / (t * 1e-3))

    def upload(m):
        A = (-psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m).to_scipy()).tocsr()
        return A, psk.DeviceCSR.from_scipy(A)

    for m in args.sides:
        A, dA = upload(m)
        n = dA.n
        name = "-FD %d^2" % m
        say(dict(what="matrix", name=name, n=n, nnz=dA.nnz, layout=dA.layout))
        bd = psk.DeviceVector.from_numpy(A @ np.random.default_rng(12345).random(n))
        del A
        xd = psk.DeviceVector(n)
        vd = psk.DeviceVector.from_numpy(np.random.default_rng(1).standard_normal(n))
        td, od = psk.DeviceVector(n), psk.DeviceVector(n)
        forms = [("jacobi", lambda: JacobiPreconditioner(dA)),
                 ("chebyshev(2)", lambda: ChebyshevPreconditioner(dA, degree=2)),
                 ("fsai(1)", lambda: FSAIPreconditioner(dA, power=1)),
                 ("multicolor_gs(1)", lambda: MulticolorGSPreconditioner(dA, sweeps=1, symmetric=True)),
                 ("multicolor_gs(2)", lambda: MulticolorGSPreconditioner(dA, sweeps=2, symmetric=True))]
        for label, form in forms:
            ts = med(lambda: form() and None)
            M = form()
            extra = dict(ncolors=M.ncolors, color_rows=M.color_rows.tolist()) if label.startswith("multicolor") else {}
            say(dict(what="setup", matrix=name, precond=label, **ts, **extra))
            say(dict(what="pcg", matrix=name, precond=label, **solve(dA, M, bd, xd)))
            if label == "multicolor_gs(1)":
                ta = med(lambda: N.check(N.lib.psk_prec_apply(M.device_handle, n, vd._p, od._p, N.PSK_DEVICE),
                                         "psk_prec_apply"), args.apply_reps)

                def two():
                    N.check(N.lib.psk_spmv(dA.handle, vd._p, td._p, N.PSK_DEVICE), "psk_spmv")
                    N.check(N.lib.psk_spmv(dA.handle, td._p, od._p, N.PSK_DEVICE), "psk_spmv")
                tt = med(two, args.apply_reps)
                vals = []
                for _ in range(args.regions + 1):
                    a = ctypes.c_double()
                    N.check(N.lib.psk_spmv_timed(dA.handle, vd._p, td._p, args.apply_reps, ctypes.byref(a)),
                            "psk_spmv_timed")
                    vals.append(a.value)
                say(dict(what="apply", matrix=name, precond=label, prec_apply=ta, two_spmv_calls=tt,
                         spmv_timed_one_ms=statistics.median(vals[1:])))
            del M
        del dA, bd, xd, vd, td, od

    if args.amg_side > 0:
        m = args.amg_side
        A, dA = upload(m)
        n = dA.n
        name = "-FD %d^2" % m
        v = np.random.default_rng(1).standard_normal(n)
        vd = psk.DeviceVector.from_numpy(v)
        od = psk.DeviceVector(n)
        for label, sm in (("gauss_seidel", GaussSeidelSmoother), ("chebyshev(2)", ChebyshevSmoother),
                          ("multicolor_gs(1)", MulticolorGaussSeidelSmoother),
                          ("multicolor_gs(1,forward)", MulticolorGaussSeidelSmoother.of(1, False))):
            t0 = time.perf_counter()
            M = AMGPreconditioner(A, numIters=2, numLevels=args.amg_levels, smoother=sm)
            sync()
            setup_ms = (time.perf_counter() - t0) * 1e3
            ta = med(lambda: N.check(N.lib.psk_prec_apply(M.device_handle, n, vd._p, od._p, N.PSK_DEVICE),
                                     "psk_prec_apply"), 3)
            y = od.numpy()
            rel = float(np.linalg.norm(v - A @ y) / np.linalg.norm(v))
            say(dict(what="amg_apply", matrix=name, levels=args.amg_levels, num_iters=2, smoother=label,
                     setup_once_ms=setup_ms, apply=ta, rel_residual_after_apply=rel))
            del M
    if out:
        out.close()


if __name__ == "__main__":
    main()
