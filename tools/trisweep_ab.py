#!/usr/bin/env python3
"""Swept against exact triangular applies (psk_prec_trisolve_sweeps) on FDLaplacian2D(m), one GPU, one process
(DESIGN.md "Swept against exact triangular applies").

    timeout 1100 python tools/trisweep_ab.py --sides 1024 2896 4096 [--out profiles/trisweep_ab.txt]

Per side: RightILU0 exact and with s in --ilu0-sweeps Jacobi sweeps per factor; up to --ilut-max-side also RightILUT
exact and with s in --ilut-sweeps. One preconditioner object per kind, switched between the variants (the switch is
a host-side word). One JSON line each:
  factors   off-diagonal entries and dependency levels of L and U, the planner's schedules, the lanes per row a sweep
            uses, and the bytes ONE sweep of ONE factor streams (mean of L and U): 12 B per entry (column + value),
            rowptr and order (4 B per row each), right-hand side, diagonal (non-unit factors), previous iterate and
            output (8 B per row each)
  spmv      the yardstick: psk_spmv (CSR layout forced) on a matrix with the pattern and values of the factor's
            off-diagonal part, median kernel ms (psk_spmv_timed) of L and of U
  apply     median ms of one M^-1 v (device vector in and out) over `regions` regions of `reps` applies; for a swept
            variant also ms per sweep and factor — the slope between the smallest and the largest sweep count —
            and the fraction of 8 TB/s the bytes above give at that time
  gmres     GMRES(30) steps per second over a fixed number of steps (tau = 0; the solve's own device-event time), and
            one solve to tau = 1e-8 capped at --maxiter: iterations, loop ms, true relative residual
The variants' regions alternate in the same run (the machine is shared). The exact variant runs exactly the launches
of a chain that was never switched (the mode is opt-in), so its line is the parent's exact apply measured in this run.
Every timing ends in a device synchronise or is a device-event interval; nothing here runs without a GPU.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 2896, 4096])
    ap.add_argument("--ilut-max-side", type=int, default=2896)
    ap.add_argument("--ilu0-sweeps", type=int, nargs="+", default=[2, 4, 6])
    ap.add_argument("--ilut-sweeps", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--maxiter", type=int, default=1500)
    ap.add_argument("--no-spmv", action="store_true", help="skip the SpMV yardstick (it downloads the factors)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU"
    if args.out:
        open(args.out, "w").close()

    def say(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        if args.out:                       # line by line: a run cut short keeps what it measured
            with open(args.out, "a") as f:
                f.write(s + "\n")

    def sync():
        N.check(N.lib.psk_synchronize(), "psk_synchronize")

    def gmres(dA, M, bd, sol, maxiter, tau):
        c = N.PskCtl(maxiter=maxiter, tau=tau, fail_on_maxiter=0, restart=30, check_every=0, time_kernels=0,
                     norm_b=0.0)
        res = N.PskResult()
        N.check(N.lib.psk_gmres(dA.handle, M.device_handle, bd._p, sol._p, ctypes.byref(c), ctypes.byref(res), None,
                                N.PSK_DEVICE), "psk_gmres")
        return res

    def spmv_ms(T, n):
        """median kernel ms of y = T x in the CSR layout (T: scipy CSR, the factor without its diagonal)"""
        dT = psk.DeviceCSR.from_scipy(T)
        dT.set_layout("csr")
        x = psk.DeviceVector.from_numpy(np.random.default_rng(2).standard_normal(n))
        y = psk.DeviceVector(n)
        ms, out = ctypes.c_double(), []
        for _ in range(args.regions * args.reps + 1):
            N.check(N.lib.psk_spmv_timed(dT.handle, x._p, y._p, N.PSK_DEVICE, ctypes.byref(ms)), "psk_spmv_timed")
            out.append(ms.value)
        return statistics.median(out[1:])

    for m in args.sides:
        dA = psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m)
        A = dA.to_scipy()
        n = A.shape[0]
        bh = A @ np.random.default_rng(12345).random(n)
        bd = psk.DeviceVector.from_numpy(bh)
        vd = psk.DeviceVector.from_numpy(np.random.default_rng(1).standard_normal(n))
        sol = psk.DeviceVector(n)
        say(dict(what="setup", side=m, n=n, nnz=int(A.nnz), regions=args.regions, reps=args.reps, steps=args.steps))
        for kind in ("ilu0", "ilut"):
            if kind == "ilut" and m > args.ilut_max_side:
                continue
            sweeps = args.ilu0_sweeps if kind == "ilu0" else args.ilut_sweeps
            sync()
            t0 = time.perf_counter()
            try:
                M = psk.RightILU0().form(dA) if kind == "ilu0" else psk.RightILUT().form(A)
            except (MemoryError, RuntimeError) as e:
                say(dict(what="form", side=m, prec=kind, formed=False, why=repr(e)[:200]))
                continue
            sync()
            say(dict(what="form", side=m, prec=kind, formed=True, form_ms=(time.perf_counter() - t0) * 1e3))
            info = M.device_info()
            unit_rows = {"L": True, "U": False}
            byt = {}
            for w, nz in (("L", info["nnz_l"]), ("U", info["nnz_u"])):
                byt[w] = 12 * nz + 4 * (n + 1) + 4 * n + 8 * n * (3 if unit_rows[w] else 4)
            width = {}
            for w in ("L", "U"):   # the rule of trisolve_sweep.hip (no entry point reports it)
                mean = info["nnz_" + w.lower()] / n
                width[w] = 1 if mean <= 2.0 else 4 if mean <= 8.0 else 16 if mean <= 32.0 else 64
            sweep_bytes = (byt["L"] + byt["U"]) / 2.0
            say(dict(what="factors", side=m, prec=kind, nnz_l=info["nnz_l"], nnz_u=info["nnz_u"],
                     levels_l=info["levels_l"], levels_u=info["levels_u"], schedule_l=M.schedule("L")["schedule"],
                     schedule_u=M.schedule("U")["schedule"], lanes_per_row_l=width["L"], lanes_per_row_u=width["U"],
                     sweep_bytes_l=byt["L"], sweep_bytes_u=byt["U"]))
            if not args.no_spmv:
                if kind == "ilu0":
                    F = M.factors()
                    NL, NU = sp.tril(F, k=-1).tocsr(), sp.triu(F, k=1).tocsr()
                    del F
                else:
                    NL, NU = sp.tril(M.ILU().L.tocsr(), k=-1).tocsr(), sp.triu(M.ILU().U.tocsr(), k=1).tocsr()
                say(dict(what="spmv", side=m, prec=kind, spmv_l_ms=spmv_ms(NL, n), spmv_u_ms=spmv_ms(NU, n),
                         layout="csr"))
                del NL, NU
            variants = [0] + list(sweeps)

            def switch(s):
                M.sweeps("L", s)
                M.sweeps("U", s)

            ap_ms = {s: [] for s in variants}
            st_s = {s: [] for s in variants}
            for r in range(args.regions + 1):          # the first region is a warm-up
                for s in variants:
                    switch(s)
                    sync()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        N.check(N.lib.psk_prec_apply(M.device_handle, n, vd._p, sol._p, N.PSK_DEVICE), "psk_prec_apply")
                    sync()
                    ap_ms[s].append((time.perf_counter() - t0) * 1e3 / args.reps)
                    res = gmres(dA, M, bd, sol, args.steps, 0.0)
                    st_s[s].append(args.steps / (res.loop_ms * 1e-3))
            med = {s: statistics.median(ap_ms[s][1:]) for s in variants}
            per_sweep = None
            if len(sweeps) >= 2:
                per_sweep = (med[sweeps[-1]] - med[sweeps[0]]) / (2.0 * (sweeps[-1] - sweeps[0]))
            for s in variants:
                a, t = ap_ms[s][1:], st_s[s][1:]
                rec = dict(what="apply", side=m, prec=kind, sweeps=s, apply_ms=med[s], min_max_ms=[min(a), max(a)],
                           vs_exact=med[s] / med[0])
                if s > 0 and per_sweep and per_sweep > 0:
                    rec.update(ms_per_sweep_and_factor=per_sweep, sweep_bytes=sweep_bytes,
                               fraction_of_8TBs=sweep_bytes / (per_sweep * 1e-3) / HBM_PEAK)
                say(rec)
                say(dict(what="gmres30_steps", side=m, prec=kind, sweeps=s, steps=args.steps,
                         steps_per_s=statistics.median(t), min_max=[min(t), max(t)]))
            for s in variants:
                switch(s)
                res = gmres(dA, M, bd, sol, args.maxiter, 1e-8)
                xh = sol.numpy()
                say(dict(what="gmres30_solve", side=m, prec=kind, sweeps=s, tau=1e-8, maxiter=args.maxiter,
                         iters=int(res.iters), converged=res.exit == N.PSK_EXIT_TOLERANCE, loop_ms=res.loop_ms,
                         true_rel_resid=float(np.linalg.norm(bh - A @ xh) / np.linalg.norm(bh))))
            del M


if __name__ == "__main__":
    main()
