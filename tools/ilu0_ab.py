#!/usr/bin/env python3
"""RightILU0 (factored on the device) against RightILUT (SuperLU spilu on the host) on FDLaplacian2D(m), one GPU
(DESIGN.md "ILU(0) on the device").

    python tools/ilu0_ab.py --sides 1024 2896 4096 [--out profiles/ilu0_ab.txt]

Per side and preconditioner, one JSON line each:
  form      wall time of form() (host clock around it, ending in a device synchronise); for ILU(0) also its split
            (psk_lab_ilu0_timing): column sort and structure checks, pattern download and dependency levels, the numeric
            launches (HIP events around them), value download and L / U split, planner and uploads
            (psk_prec_create_trisolve). ILUT above --ilut-max-side is not attempted: spilu cannot form it
            (SUPERLU_MALLOC at 4096^2) and the line says so.
  factors   entries and bytes (12 B per entry) of L + U, dependency levels, the planner's schedules
  apply     median ms of one M^-1 v (device vector in and out) over `regions` regions of `reps` applies
  gmres     GMRES(30) steps per second over a fixed number of steps (tau = 0; the solve's own device-event time), and
            the iterations to tau = 1e-8 (capped at --maxiter; converged or not is recorded)
The two preconditioners' apply and GMRES regions alternate in the same run (the machine is shared). Every timing
ends in a device synchronise or is a device-event interval; nothing here runs without a GPU.
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
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 2896, 4096])
    ap.add_argument("--ilut-max-side", type=int, default=2896)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--maxiter", type=int, default=1500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU"
    lab = N.load_lab()
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

    for m in args.sides:
        dA = psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m)
        A = dA.to_scipy()
        n = A.shape[0]
        bh = A @ np.random.default_rng(12345).random(n)
        bd = psk.DeviceVector.from_numpy(bh)
        vd = psk.DeviceVector.from_numpy(np.random.default_rng(1).standard_normal(n))
        sol = psk.DeviceVector(n)
        say(dict(what="setup", side=m, n=n, nnz=int(A.nnz), regions=args.regions, reps=args.reps, steps=args.steps))
        precs = {}
        for name in ("ilu0", "ilut"):
            if name == "ilut" and m > args.ilut_max_side:
                say(dict(what="form", side=m, prec=name, formed=False,
                         why="not attempted: spilu cannot form this factor (SUPERLU_MALLOC at 4096^2, VERDICT.md)"))
                continue
            sync()
            t0 = time.perf_counter()
            try:
                M = (psk.RightILU0() if name == "ilu0" else psk.RightILUT()).form(dA if name == "ilu0" else A)
            except (MemoryError, RuntimeError) as e:
                say(dict(what="form", side=m, prec=name, formed=False, why=repr(e)[:200]))
                continue
            sync()
            rec = dict(what="form", side=m, prec=name, formed=True, form_ms=(time.perf_counter() - t0) * 1e3)
            if name == "ilu0":
                t = (ctypes.c_double * 7)()
                N.check(lab.psk_lab_ilu0_timing(t), "psk_lab_ilu0_timing")
                rec.update(sort_ms=t[0], levels_ms=t[1], numeric_ms=t[2], split_ms=t[3], plan_upload_ms=t[4],
                           numeric_launches=int(t[5]), lanes_per_row=int(t[6]))
            say(rec)
            info = M.device_info()
            ent = info["nnz_l"] + info["nnz_u"] + n
            sched = {w: N.I32() for w in ("L", "U")}
            for w, k in (("L", 0), ("U", 1)):
                N.check(N.lib.psk_prec_trisolve_schedule(M.device_handle, k, -1, ctypes.byref(sched[w]), None, None,
                                                         None, None), "psk_prec_trisolve_schedule")
            names = ("syncfree", "band", "lds", "grid", "part", "levels")
            say(dict(what="factors", side=m, prec=name, entries=ent, bytes=12 * ent, over_nnz_a=ent / A.nnz,
                     levels_l=info["levels_l"], levels_u=info["levels_u"], schedule_l=names[sched["L"].value],
                     schedule_u=names[sched["U"].value]))
            precs[name] = M
        # apply and GMRES(30) steps, the preconditioners alternating region by region
        ap_ms = {k: [] for k in precs}
        st_s = {k: [] for k in precs}
        for r in range(args.regions + 1):          # the first region is a warm-up
            for k, M in precs.items():
                sync()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    N.check(N.lib.psk_prec_apply(M.device_handle, n, vd._p, sol._p, N.PSK_DEVICE), "psk_prec_apply")
                sync()
                ap_ms[k].append((time.perf_counter() - t0) * 1e3 / args.reps)
                res = gmres(dA, M, bd, sol, args.steps, 0.0)
                st_s[k].append(args.steps / (res.loop_ms * 1e-3))
        for k, M in precs.items():
            a, s = ap_ms[k][1:], st_s[k][1:]
            say(dict(what="apply", side=m, prec=k, apply_ms=statistics.median(a), min_max_ms=[min(a), max(a)]))
            say(dict(what="gmres30_steps", side=m, prec=k, steps=args.steps, steps_per_s=statistics.median(s),
                     min_max=[min(s), max(s)]))
        for k, M in precs.items():
            res = gmres(dA, M, bd, sol, args.maxiter, 1e-8)
            xh = sol.numpy()
            say(dict(what="gmres30_solve", side=m, prec=k, tau=1e-8, maxiter=args.maxiter, iters=int(res.iters),
                     converged=res.exit == N.PSK_EXIT_TOLERANCE, loop_ms=res.loop_ms,   # not the maxiter exit
                     true_rel_resid=float(np.linalg.norm(bh - A @ xh) / np.linalg.norm(bh))))
        del precs, M


if __name__ == "__main__":
    main()
