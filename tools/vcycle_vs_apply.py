"""Per-cycle cost of the standalone V-cycle solver (psk_vcycle) against the AMG preconditioner apply on the SAME
hierarchy: -FD m^2 (default 2048), AMG(numLevels=5, nu=2+2, Gauss-Seidel), 8 cycles each with tau = 0 (no early
exit on either side). The apply enqueues, per cycle, the cycle, the residual SpMV and three small launches
(check, conditional copy, promote; none after the last cycle); the solver the cycle, the residual SpMV and
vc_check_kernel. After one warm-up of each, `reps` repetitions alternate between the two:

* apply: wall time of AMGPreconditioner.apply on a device vector (the entry point synchronises) / cycles;
* solver: psk_result.loop_ms / cycles (HIP events around the loop) and the call's wall time / cycles.

One JSON line on stdout: both series, their medians, the apply's max - min spread and whether the solver's
x equals the apply's bitwise.

    python tools/vcycle_vs_apply.py [--m 2048] [--levels 5] [--cycles 8] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import AMGPreconditioner
    m, n, k = a.m, a.m * a.m, a.cycles
    t0 = time.time()
    A = -psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m).to_scipy()
    dA = psk.DeviceCSR.from_scipy(A)
    M = AMGPreconditioner(dA, numIters=k, numLevels=a.levels, tau=0.0)
    del A
    print("setup %.1f s, levels %s" % (time.time() - t0, M.levels()), file=sys.stderr, flush=True)
    b = psk.DeviceVector.from_numpy(np.random.default_rng(1).standard_normal(n))
    x = psk.DeviceVector(n)
    ctl = N.PskCtl(maxiter=k, tau=0.0, fail_on_maxiter=0, restart=0, check_every=0, time_kernels=0, norm_b=0.0)
    res = N.PskResult()

    def sync():
        N.check(N.lib.psk_synchronize(), "psk_synchronize")

    def apply_once():
        sync()
        t = time.perf_counter()
        y = M.apply(b)
        sync()
        return (time.perf_counter() - t) * 1e3 / k, y

    def solve_once():
        sync()
        t = time.perf_counter()
        N.check(N.lib.psk_vcycle(M.device_handle, b._p, x._p, ctypes.byref(ctl), ctypes.byref(res), None, 0,
                                 N.PSK_DEVICE), "psk_vcycle")
        sync()
        return res.loop_ms / k, (time.perf_counter() - t) * 1e3 / k

    _, y = apply_once()      # warm-up of each
    solve_once()
    same = bool(np.array_equal(y.numpy(), x.numpy()))
    ap_ms, sv_loop, sv_wall = [], [], []
    for r in range(a.reps):
        ap_ms.append(apply_once()[0])
        lo, wa = solve_once()
        sv_loop.append(lo)
        sv_wall.append(wa)
        print("rep %d: apply %.4f ms/cycle, solver loop %.4f wall %.4f ms/cycle" % (r, ap_ms[-1], lo, wa),
              file=sys.stderr, flush=True)
    out = {"workload": "-FDLaplacian2D %dx%d, AMG(numLevels=%d, nu=2+2, GS), %d cycles, tau=0" % (m, m, a.levels, k),
           "n": n, "levels": M.levels(), "cycles": k, "reps": a.reps, "bitwise_equal_x": same,
           "apply_ms_per_cycle": ap_ms, "solver_loop_ms_per_cycle": sv_loop, "solver_wall_ms_per_cycle": sv_wall,
           "apply_median": float(np.median(ap_ms)), "apply_spread": float(max(ap_ms) - min(ap_ms)),
           "solver_loop_median": float(np.median(sv_loop)), "solver_wall_median": float(np.median(sv_wall))}
    out["solver_loop_minus_apply"] = out["solver_loop_median"] - out["apply_median"]
    out["solver_wall_minus_apply"] = out["solver_wall_median"] - out["apply_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
