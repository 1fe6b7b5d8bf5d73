#!/usr/bin/env python3
"""FSAI measurements on the 2-D Laplacian stencils, one GPU (DESIGN.md "Factorized sparse approximate inverse").

    python tools/fsai_ab.py [--sides -4096 3163] [--regions 5] [--out profiles/fsai_ab.txt]

A negative side means -FDLaplacian2D(-1, 1, |side|) (positive definite, uploaded from scipy), a positive one
FDLaplacian2D(-1, 1, side) as the benchmark's headline generates it on the device (negative definite, diagonal SpMV
layout). For each matrix and for power 1 and 2 it reports, from ONE process:

* setup: psk_prec_create_fsai (host clock around the call, which ends in a device synchronise; for power 2 the
  pattern's SpGEMM is timed separately), beside psk_csr_ilu0 on the same matrix;
* apply: psk_prec_apply on device vectors (host clock, the call synchronises), beside two psk_spmv calls on G and
  Gt measured the same way, and beside psk_spmv_timed of G plus Gt (device events around back-to-back launches, no
  host in the interval): the apply IS those two launches, so the first two agree up to noise and their distance to the
  third is the host's call and synchronise overhead;
* PCG to tau = 1e-8 on b = A rand(seed 12345): iterations, iterations per second and time to solution (psk_result's
  loop_ms, device events) for Jacobi and for FSAI.

Every timing is the median of `regions` repetitions after one untimed warm-up, with the minimum and maximum.
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
    ap.add_argument("--sides", type=int, nargs="+", default=[-4096, 3163])
    ap.add_argument("--powers", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--apply-reps", type=int, default=20)
    ap.add_argument("--maxiter", type=int, default=40000)
    ap.add_argument("--skip-ilu0", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import FSAIPreconditioner, JacobiPreconditioner, matmat
    assert N.device_count() >= 1, "no GPU"
    lines = []

    def say(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    say(dict(what="command", argv=["tools/fsai_ab.py"] + sys.argv[1:], regions=args.regions,
             apply_reps=args.apply_reps))

    def sync():
        N.check(N.lib.psk_synchronize(), "psk_synchronize")

    def med(f, reps=1):
        f()
        sync()
        ts = []
        r = None
        for _ in range(args.regions):
            t0 = time.perf_counter()
            for _ in range(reps):
                r = f()
            sync()
            ts.append((time.perf_counter() - t0) * 1e3 / reps)
        return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts)), r

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

    for side in args.sides:
        m = abs(side)
        dA = psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m)
        A = dA.to_scipy()
        if side < 0:
            A = (-A).tocsr()
            dA = psk.DeviceCSR.from_scipy(A)
        n = dA.n
        name = "%sFD %d^2" % ("-" if side < 0 else "", m)
        say(dict(what="matrix", name=name, n=n, nnz=dA.nnz, layout=dA.layout))
        bh = A @ np.random.default_rng(12345).random(n)
        del A
        bd = psk.DeviceVector.from_numpy(bh)
        xd = psk.DeviceVector(n)
        vd = psk.DeviceVector.from_numpy(np.random.default_rng(1).standard_normal(n))
        td, od = psk.DeviceVector(n), psk.DeviceVector(n)
        if not args.skip_ilu0:
            t, _ = med(lambda: dA.ilu0() and None)
            say(dict(what="ilu0_setup", matrix=name, **t))
        J = JacobiPreconditioner(dA)
        say(dict(what="pcg", matrix=name, precond="jacobi", **solve(dA, J, bd, xd)))
        for power in args.powers:
            pat = None
            if power == 2:
                t, _ = med(lambda: matmat(dA, dA) and None)
                say(dict(what="pattern_spgemm", matrix=name, power=power, **t))
            t, _ = med(lambda: FSAIPreconditioner(dA, power=power) and None)
            if power == 2:   # the class forms the pattern itself: the factor alone is the difference
                pat = matmat(dA, dA)
                t2, _ = med(lambda: dA.fsai(pattern=pat) and None)
                say(dict(what="fsai_factor_given_pattern", matrix=name, power=power, **t2))
            say(dict(what="fsai_setup", matrix=name, power=power, **t))
            G, sign = dA.fsai(pattern=pat)
            del pat
            Gt = G.transpose()
            M = FSAIPreconditioner(dA, power=power)
            say(dict(what="fsai", matrix=name, power=power, sign=sign, nnz_g=M.nnz, max_row=M.max_row,
                     layout_g=G.layout, layout_gt=Gt.layout))
            ta, _ = med(lambda: N.check(N.lib.psk_prec_apply(M.device_handle, n, vd._p, od._p, N.PSK_DEVICE),
                                        "psk_prec_apply"), args.apply_reps)

            def two():
                N.check(N.lib.psk_spmv(G.handle, vd._p, td._p, N.PSK_DEVICE), "psk_spmv")
                N.check(N.lib.psk_spmv(Gt.handle, td._p, od._p, N.PSK_DEVICE), "psk_spmv")
            tt, _ = med(two, args.apply_reps)
            ev = []
            for H, src, dst in ((G, vd, td), (Gt, td, od)):
                vals = []
                for _ in range(args.regions + 1):
                    a = ctypes.c_double()
                    N.check(N.lib.psk_spmv_timed(H.handle, src._p, dst._p, args.apply_reps, ctypes.byref(a)),
                            "psk_spmv_timed")
                    vals.append(a.value)
                ev.append(statistics.median(vals[1:]))
            say(dict(what="apply", matrix=name, power=power, prec_apply=ta, two_spmv_calls=tt,
                     spmv_timed_g_ms=ev[0], spmv_timed_gt_ms=ev[1], spmv_timed_sum_ms=ev[0] + ev[1]))
            del G, Gt
            say(dict(what="pcg", matrix=name, precond="fsai", power=power, **solve(dA, M, bd, xd)))
            del M
        del J, dA, bd, xd, vd, td, od
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
