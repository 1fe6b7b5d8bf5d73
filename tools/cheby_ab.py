#!/usr/bin/env python3
"""Chebyshev smoother measurements on -FDLaplacian2D(m), one GPU (DESIGN.md "Chebyshev polynomial smoother").

    python tools/cheby_ab.py --side 2048 --levels 5 [--out profiles/cheby_ab.txt]

Part 1, the fused step (cheby_step_kernel) against the same step as the launches the library had before it
(residual SpMV in the level's own layout, DInv scale, d update, z update), on the fine level and SA levels 3 and 2
of the hierarchy: both in the same run, alternating, `regions` regions of `reps` back-to-back steps between device
events (psk_lab_cheby_ab), medians reported, with the fused step's modelled bytes (12 nnz + 4 n matrix, 52 n vectors)
over its time as a fraction of the 8.0 TB/s HBM peak.

Part 2, the smoothers inside the hierarchy: one AMG apply (2 cycles), the standalone V-cycle solver to
tau = 1e-8 (cycles and time to solution), and PCG + AMG for a fixed number of iterations (with the reference's
V-cycle apply, which starts from x = copy(v), PCG does not converge on this matrix with any smoother: the protocol
of tools/bench_amg.py), for Gauss-Seidel nu = 2 and Chebyshev degree 2 / 3 at nu = 1 / 2. Every timing is a median of
`regions` host-clock regions that end in a device synchronise.
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

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--pcg-iters", type=int, default=10)
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import AMGPreconditioner, AMGVCycleSolver, ChebyshevPreconditioner, ChebyshevSmoother
    assert N.device_count() >= 1, "no GPU"
    lab = N.load_lab()
    lines = []

    def say(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    m = args.side
    A = -psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m).to_scipy()
    dA = psk.DeviceCSR.from_scipy(A)
    n = A.shape[0]
    say(dict(what="setup", side=m, n=n, levels=args.levels, regions=args.regions, reps=args.reps))

    def med(f):
        f()
        N.check(N.lib.psk_synchronize(), "sync")
        ts = []
        for _ in range(args.regions):
            t0 = time.perf_counter()
            r = f()
            N.check(N.lib.psk_synchronize(), "sync")
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts), r

    # the Gauss-Seidel hierarchy gives the level matrices for part 1 and the baseline of part 2
    Mgs = AMGPreconditioner(dA, numIters=2, numLevels=args.levels)
    say(dict(what="levels", sizes=Mgs.levels()))

    # ---- part 1 ------------------------------------------------------------------------------------------
    for k in sorted({args.levels - 1, min(3, args.levels - 1), min(2, args.levels - 1)}, reverse=True):
        dk = Mgs._A[k]
        C = ChebyshevPreconditioner(dk, degree=3)
        v = psk.DeviceVector.from_numpy(np.random.default_rng(k).standard_normal(dk.n))
        fu, pi = [], []
        a, b = ctypes.c_double(), ctypes.c_double()
        for _ in range(args.regions + 1):          # the first region is a warm-up
            N.check(lab.psk_lab_cheby_ab(C.device_handle, v._p, args.reps, ctypes.byref(a), ctypes.byref(b)),
                    "psk_lab_cheby_ab")
            fu.append(a.value)
            pi.append(b.value)
        fu, pi = fu[1:], pi[1:]
        fm, pm = statistics.median(fu), statistics.median(pi)
        model = 12.0 * dk.nnz + 4.0 * dk.n + 52.0 * dk.n
        say(dict(what="step", level=k, n=dk.n, nnz=dk.nnz, layout=dk.layout, fused_us=fm * 1e3, pieces_us=pm * 1e3,
                 fused_min_max_us=[min(fu) * 1e3, max(fu) * 1e3], pieces_min_max_us=[min(pi) * 1e3, max(pi) * 1e3],
                 fused_over_pieces=fm / pm, model_bytes=model, fused_frac_hbm_peak=model / (fm * 1e-3) / HBM_PEAK,
                 lmax=C.lmax))
        del C, v

    # ---- part 2 ------------------------------------------------------------------------------------------
    if not args.skip_solves:
        x = np.random.default_rng(12345).random(n)
        bh = A @ x
        bd = psk.DeviceVector.from_numpy(bh)
        vd = psk.DeviceVector.from_numpy(np.random.default_rng(1).standard_normal(n))
        sol = psk.DeviceVector(n)
        configs = [("gs", None, 2)] + [("cheb", d, nu) for d in (2, 3) for nu in (1, 2)]
        for kind, deg, nu in configs:
            sm = psk.GaussSeidelSmoother if kind == "gs" else ChebyshevSmoother.of(degree=deg)
            M = Mgs if kind == "gs" else AMGPreconditioner(dA, numIters=2, numLevels=args.levels, nuPre=nu, nuPost=nu,
                                                           smoother=sm)
            apply_ms = med(lambda: M.apply(vd))[:3]
            per = []
            for k in range(1, args.levels):
                vk = psk.DeviceVector.from_numpy(np.random.default_rng(k).standard_normal(M.levels()[k]))
                per.append(dict(level=k, n=M.levels()[k], op_ms=med(lambda: M._S[k].operator.apply(vk))[0]))
            ctl = psk.CommonSolverArgs(maxiter=200, tau=1e-8, showIters=False, showFinal=False, failOnMaxiter=False)
            vs = AMGVCycleSolver(ctl, numLevels=args.levels, nuPre=nu, nuPost=nu, smoother=sm)
            vs._cycleMgr = AMGPreconditioner(dA, numIters=1, numLevels=args.levels, nuPre=nu, nuPost=nu, smoother=sm,
                                             tau=0.0)
            vs.freezeMatrix()
            vc = med(lambda: vs.solve(dA, bd))
            st = vc[3]
            rr = np.linalg.norm(bh - A @ st.soln().numpy()) / np.linalg.norm(bh)

            def pcg():
                c = N.PskCtl(maxiter=args.pcg_iters, tau=0.0, fail_on_maxiter=0, restart=0, check_every=0,
                             time_kernels=0, norm_b=0.0)
                res = N.PskResult()
                N.check(N.lib.psk_pcg(dA.handle, M.device_handle, bd._p, sol._p, ctypes.byref(c), ctypes.byref(res),
                                      None, N.PSK_DEVICE), "psk_pcg")
                return res
            pc = med(pcg)
            say(dict(what="amg", smoother=kind, degree=deg, nu=nu, apply_ms=apply_ms[0], apply_min_max_ms=apply_ms[1:],
                     smoother_op_ms=per, vcycle_cycles=int(st.iters()), vcycle_converged=bool(st.success()),
                     vcycle_ms=vc[0], vcycle_min_max_ms=[vc[1], vc[2]], vcycle_true_rel_resid=rr,
                     pcg_iters=args.pcg_iters, pcg_ms=pc[0], pcg_rec_resid_ratio=pc[3].resid_recursive / pc[3].norm_b))
            if kind != "gs":
                del M
            del vs
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
