#!/usr/bin/env python3
"""IDR(4) and IDR(8) against BiCGStab and GMRES(30) on convection-diffusion operators: steps/s and time to solution.

    python tools/idrs_vs_bicgstab.py [--jacobi-side 4096] [--ilu0-side 1024] [--c 0.2] [--tau 1e-8] \
        [--maxiter 6000] [--reps 3] [--baseline-tree DIR] [--out profiles/idrs_vs_bicgstab.txt]

The operator is cd m (tools/bicgstab_vs_gmres.py's), b = A x for a random x, operands resident in HBM. Two systems:
side --jacobi-side with Jacobi, and side --ilu0-side with RightILU0 (0 skips one). One STEP is one SpMV with its
preconditioner apply, for every method: an IDR(s) step, half a BiCGStab iteration, a GMRES Arnoldi step; --maxiter
counts steps (BiCGStab gets maxiter/2 iterations). Each library is measured in a child process of its own (this
process never opens the GPU): one short warm-up solve per method, then --reps solves of each, the methods alternating;
the time is psk_result.loop_ms (HIP events around the loop). Reported per method: whether it met tau within maxiter,
the SpMV launches that did their work, the median and every loop_ms, steps/s, and the true ||b - A x|| / ||b|| it
reached. --baseline-tree: BiCGStab alone from another built checkout of this project (the parent commit's), the
same way.
The output file starts with the command line and the sha256 of each library measured.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

METHODS = ("idrs4", "idrs8", "bicgstab", "gmres30")


def worker(args):
    """Measures in this process with the package and library of the checkout --tree; one JSON line per system."""
    from bicgstab_vs_gmres import cd_matrix
    sys.path.insert(0, args.tree)
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    methods = args.methods
    for side, prec in ((args.jacobi_side, "jacobi"), (args.ilu0_side, "ilu0")):
        if side <= 0:
            continue
        n = side * side
        dA = psk.DeviceCSR.from_scipy(cd_matrix(side, args.c))
        x = psk.DeviceVector.from_numpy(np.random.default_rng(12345).random(n))
        b = psk.Linear.spmv(dA, x)
        del x
        M = (psk.JacobiPreconditionerType() if prec == "jacobi" else psk.RightILU0()).form(dA)
        sol = psk.DeviceVector(n)
        bh = b.numpy()
        nb = float(np.linalg.norm(bh))

        def run(method, maxiter):
            steps = maxiter // 2 if method == "bicgstab" else maxiter
            ctl = N.PskCtl(maxiter=steps, tau=args.tau, fail_on_maxiter=1, restart=30 if method == "gmres30" else 0,
                           check_every=0, time_kernels=0)
            res = N.PskResult()
            a = (dA.handle, M.device_handle, b._p, sol._p, ctypes.byref(ctl))
            tail = (ctypes.byref(res), None, N.PSK_DEVICE)
            if method.startswith("idrs"):
                rc = N.lib.psk_idrs(*a, int(method[4:]), *tail)
            else:
                rc = {"bicgstab": N.lib.psk_bicgstab, "gmres30": N.lib.psk_gmres}[method](*a, *tail)
            N.check(rc, method)
            return res

        def spmvs(method, r):
            """SpMV launches of the loop (not the true residual's): those that did their work."""
            if method == "gmres30":
                return int(r.iters) + (1 if r.status == N.PSK_MAXITER else 0)
            return int(r.spmv_launches) - (1 if r.exit == N.PSK_EXIT_TOLERANCE else 0)

        for m in methods:
            run(m, 40)                                         # warm-up: code objects, workspace
        runs = {m: [] for m in methods}
        reached = {}
        for _ in range(args.reps):
            for m in methods:                                  # alternating
                r = run(m, args.maxiter)
                tr = float(np.linalg.norm(bh - psk.Linear.spmv(dA, sol).numpy())) / nb
                runs[m].append((float(r.loop_ms), spmvs(m, r), int(r.status), int(r.iters)))
                reached[m] = tr
                print("cd%d/%s %s: %.1f ms, %d SpMVs, %s, %.2e" % (side, prec, m, r.loop_ms, runs[m][-1][1],
                                                                  N.STATUS_NAMES[int(r.status)], tr), file=sys.stderr, flush=True)
        out = {"side": side, "n": n, "precond": prec, "layout": dA.layout, "methods": {}}
        for m in methods:
            ms = [q[0] for q in runs[m]]
            med = statistics.median(ms)
            out["methods"][m] = {"status": N.STATUS_NAMES[runs[m][-1][2]], "met_tau": runs[m][-1][2] == N.PSK_CONVERGED,
                                 "spmv": runs[m][-1][1], "iters": runs[m][-1][3], "loop_ms_median": med,
                                 "loop_ms_all": ms, "steps_per_s": runs[m][-1][1] / (med * 1e-3),
                                 "true_resid_over_normb": reached[m]}
        print("RESULT " + json.dumps(out), flush=True)
        del dA, M, b, sol


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def measure(tree, methods, args):
    """One child process on the checkout `tree`: its RESULT lines, decoded."""
    env = dict(os.environ)
    env.pop("PSK_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--methods", *methods, "--jacobi-side",
           str(args.jacobi_side), "--ilu0-side", str(args.ilu0_side), "--c", str(args.c), "--tau", str(args.tau),
           "--maxiter", str(args.maxiter), "--reps", str(args.reps)]
    p = subprocess.run(cmd, env=env, cwd=os.path.join(REPO, "tools"), stdout=subprocess.PIPE, text=True)   # stderr: progress
    if p.returncode != 0:
        raise SystemExit("worker on %s failed (%d):\n%s" % (tree, p.returncode, p.stdout[-4000:]))
    return [json.loads(l[7:]) for l in p.stdout.splitlines() if l.startswith("RESULT ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jacobi-side", type=int, default=4096)
    ap.add_argument("--ilu0-side", type=int, default=1024)
    ap.add_argument("--c", type=float, default=0.2)
    ap.add_argument("--tau", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=6000, help="steps (SpMVs) a solve may take")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--methods", nargs="+", default=list(METHODS), choices=METHODS)
    ap.add_argument("--baseline-tree", default=None,
                    help="another built checkout of this project: BiCGStab alone is measured on it too")
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "idrs_vs_bicgstab.txt"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    def lib_of(tree):
        return os.path.join(tree, "pysolvers_amd", "_lib", "libpsk.so")

    lines = ["# " + " ".join(["python", "tools/idrs_vs_bicgstab.py"] + sys.argv[1:]),
             "# this library: sha256 %s" % sha256(lib_of(REPO))]
    jobs = [("this", REPO, args.methods)]
    if args.baseline_tree:
        base = os.path.abspath(args.baseline_tree)
        lines.append("# baseline library (BiCGStab only): sha256 %s" % sha256(lib_of(base)))
        jobs.append(("baseline", base, ["bicgstab"]))
    lines.append("# cd m, c = %g, tau = %g, at most %d steps (one step = one SpMV + one preconditioner apply); "
                 "loop_ms: HIP events around the device loop, median of %d" % (args.c, args.tau, args.maxiter, args.reps))
    fmt = "%-8s %-13s %-8s %-9s %6s %9s %8s  %-14s %s"
    lines.append(fmt % ("library", "system", "method", "status", "SpMVs", "loop_ms", "steps/s", "||b-Ax||/||b||",
                        "every loop_ms"))
    for tag, tree, methods in jobs:
        for sysres in measure(tree, methods, args):
            name = "cd%d/%s" % (sysres["side"], sysres["precond"])
            for m in methods:
                e = sysres["methods"].get(m)
                if e is None:
                    continue
                lines.append(fmt % (tag, name, m, e["status"], e["spmv"], "%.2f" % e["loop_ms_median"],
                                    "%.0f" % e["steps_per_s"], "%.2e" % e["true_resid_over_normb"],
                                    " ".join("%.2f" % v for v in e["loop_ms_all"])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
