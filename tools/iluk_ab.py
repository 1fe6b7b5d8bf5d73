#!/usr/bin/env python3
"""RightILUK(k), k = 0..3, against RightILU0 on two 5-point operators, one GPU (DESIGN.md "ILU(k) on the device").

    python tools/iluk_ab.py [--side 1024] [--c 0.2] [--levels 0 1 2 3] [--out profiles/iluk_ab.txt]

Operators: cd m (tools/bicgstab_vs_gmres.py's convection-diffusion operator, the one of tools/idrs_vs_bicgstab.py) and
-FDLaplacian2D(m). b = A x for a random x; operands resident in HBM. The baseline is RightILU0, formed and applied by
the code the parent commit has, in the same process and run. Per operator and preconditioner, JSON lines:
  form      wall time of form() ending in a device synchronise, and its split: symbolic (psk_lab_iluk_timing: sort,
            rounds, padding; 0 for RightILU0), numeric (psk_lab_ilu0_timing: its sort, level planning and the numeric
            launches), planner (value download, L / U split, psk_prec_create_trisolve); rounds and lanes per row
  factors   nnz(F) / nnz(A), dependency levels of L and U, the planner's schedules
  apply     median ms of one M^-1 v over `regions` regions of `reps` applies, exact and with sweeps = 4; the
            preconditioners alternate region by region (the machine is shared), the first region is a warm-up
  solve     iterations, status, loop_ms (HIP events around the device loop) and the true ||b - A x|| / ||b|| for
            GMRES(30) and IDR(4) on cd m, GMRES(30) and PCG on -FD, tau = 1e-8, exact applies and sweeps = 4; a solve
            that does not meet tau within --maxiter steps says so
then a summary table with each figure's ratio to RightILU0's. Every timing ends in a device synchronise or is a
device-event interval; nothing here runs without a GPU.
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
sys.path.insert(0, os.path.join(REPO, "tools"))

SCHEDULES = ("syncfree", "band", "lds", "grid", "part", "levels")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--c", type=float, default=0.2)
    ap.add_argument("--levels", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--tau", type=float, default=1e-8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "iluk_ab.txt"))
    args = ap.parse_args()
    from bicgstab_vs_gmres import cd_matrix
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU"
    lab = N.load_lab()
    open(args.out, "w").close()

    def emit(s):
        print(s, flush=True)
        with open(args.out, "a") as f:           # line by line: a run cut short keeps what it measured
            f.write(s + "\n")

    def say(obj):
        emit(json.dumps(obj))

    def sync():
        N.check(N.lib.psk_synchronize(), "psk_synchronize")

    emit("# python tools/iluk_ab.py --side %d --c %g --levels %s --regions %d --reps %d --maxiter %d --tau %g"
         % (args.side, args.c, " ".join(map(str, args.levels)), args.regions, args.reps, args.maxiter, args.tau))
    m = args.side
    table = []
    for case in ("cd", "negfd"):
        if case == "cd":
            A = cd_matrix(m, args.c)
            dA = psk.DeviceCSR.from_scipy(A)
            methods = ("gmres30", "idrs4")
        else:
            dA0 = psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m)
            A = (-dA0.to_scipy()).tocsr()
            del dA0
            dA = psk.DeviceCSR.from_scipy(A)
            methods = ("gmres30", "pcg")
        n = A.shape[0]
        bh = A @ np.random.default_rng(12345).random(n)
        nb = float(np.linalg.norm(bh))
        bd = psk.DeviceVector.from_numpy(bh)
        vd = psk.DeviceVector.from_numpy(np.random.default_rng(1).standard_normal(n))
        sol = psk.DeviceVector(n)
        say(dict(what="setup", case=case, side=m, n=n, nnz=int(A.nnz), layout=dA.layout, regions=args.regions,
                 reps=args.reps, tau=args.tau, maxiter=args.maxiter))
        precs = {}
        rows = {}
        for name in ["ilu0"] + ["iluk%d" % k for k in args.levels]:
            sync()
            t0 = time.perf_counter()
            M = (psk.RightILU0() if name == "ilu0" else psk.RightILUK(int(name[4:]))).form(dA)
            sync()
            form_ms = (time.perf_counter() - t0) * 1e3
            t = (ctypes.c_double * 7)()
            N.check(lab.psk_lab_ilu0_timing(t), "psk_lab_ilu0_timing")
            rec = dict(what="form", case=case, prec=name, form_ms=form_ms, symbolic_ms=0.0,
                       numeric_ms=t[0] + t[1] + t[2], numeric_launch_ms=t[2], planner_ms=t[3] + t[4],
                       numeric_launches=int(t[5]), numeric_lanes_per_row=int(t[6]))
            if name != "ilu0":
                u = (ctypes.c_double * 7)()
                N.check(lab.psk_lab_iluk_timing(u), "psk_lab_iluk_timing")
                rec.update(symbolic_ms=u[0], rounds=int(u[2]), wide_rounds=int(u[3]), symbolic_lanes_per_row=int(u[4]))
            say(rec)
            info = M.device_info()
            ent = info["nnz_l"] + info["nnz_u"] + n
            fac = dict(what="factors", case=case, prec=name, entries=ent, fill_ratio=ent / A.nnz,
                       levels_l=info["levels_l"], levels_u=info["levels_u"],
                       schedule_l=M.schedule("L")["schedule"], schedule_u=M.schedule("U")["schedule"])
            say(fac)
            precs[name] = M
            rows[name] = dict(form=rec, fac=fac, apply={}, solve={})

        def set_sweeps(M, s):
            M.sweeps("L", s)
            M.sweeps("U", s)

        for mode, s in (("exact", 0), ("sweeps4", 4)):
            ap_ms = {k: [] for k in precs}
            for M in precs.values():
                set_sweeps(M, s)
            for r in range(args.regions + 1):
                for k, M in precs.items():
                    sync()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        N.check(N.lib.psk_prec_apply(M.device_handle, n, vd._p, sol._p, N.PSK_DEVICE), "psk_prec_apply")
                    sync()
                    ap_ms[k].append((time.perf_counter() - t0) * 1e3 / args.reps)
            for k in precs:
                a = ap_ms[k][1:]
                rows[k]["apply"][mode] = statistics.median(a)
                say(dict(what="apply", case=case, prec=k, mode=mode, apply_ms=statistics.median(a),
                         min_max_ms=[min(a), max(a)]))
            for k, M in precs.items():
                for method in methods:
                    ctl = N.PskCtl(maxiter=args.maxiter, tau=args.tau, fail_on_maxiter=1,
                                   restart=30 if method == "gmres30" else 0, check_every=0, time_kernels=0)
                    res = N.PskResult()
                    a = (dA.handle, M.device_handle, bd._p, sol._p, ctypes.byref(ctl))
                    tail = (ctypes.byref(res), None, N.PSK_DEVICE)
                    if method == "idrs4":
                        rc = N.lib.psk_idrs(*a, 4, *tail)
                    else:
                        rc = {"gmres30": N.lib.psk_gmres, "pcg": N.lib.psk_pcg}[method](*a, *tail)
                    N.check(rc, method)
                    tr = float(np.linalg.norm(bh - A @ sol.numpy())) / nb
                    met = res.status == N.PSK_CONVERGED
                    rows[k]["solve"][(mode, method)] = (int(res.iters), float(res.loop_ms), met)
                    say(dict(what="solve", case=case, prec=k, mode=mode, method=method, iters=int(res.iters),
                             status=N.STATUS_NAMES[int(res.status)], met_tau=met, loop_ms=float(res.loop_ms),
                             true_rel_resid=tr))
        for M in precs.values():
            set_sweeps(M, 0)
        table.append((case, methods, rows))
        del precs, M, dA, bd, vd, sol

    # the summary: every figure and its ratio to RightILU0's in the same run
    def ratio(x, base):
        return "%.2fx" % (x / base) if base > 0 else "-"

    emit("")
    emit("# summary, side %d; (x) = ratio to RightILU0 in this run; solve = form-free loop_ms to tau = %g, '!' = tau "
         "not met within %d steps" % (m, args.tau, args.maxiter))
    for case, methods, rows in table:
        base = rows["ilu0"]
        emit("# %s %d^2" % (case, m))
        emit("%-6s %9s %9s %9s %9s %5s %7s %7s %-17s %16s %16s" % ("prec", "form_ms", "symbolic", "numeric", "planner",
                                                                   "fill", "lev_L", "lev_U", "schedules L/U",
                                                                   "apply_ms exact", "apply_ms sweeps4"))
        for k, r in rows.items():
            f, fa = r["form"], r["fac"]
            emit("%-6s %9.1f %9.1f %9.1f %9.1f %5.2f %7d %7d %-17s %8.3f (%s) %8.3f (%s)"
                 % (k, f["form_ms"], f["symbolic_ms"], f["numeric_ms"], f["planner_ms"], fa["fill_ratio"], fa["levels_l"],
                    fa["levels_u"], fa["schedule_l"] + "/" + fa["schedule_u"], r["apply"]["exact"],
                    ratio(r["apply"]["exact"], base["apply"]["exact"]), r["apply"]["sweeps4"],
                    ratio(r["apply"]["sweeps4"], base["apply"]["sweeps4"])))
        for mode in ("exact", "sweeps4"):
            for method in methods:
                emit("%-6s %s, %s applies: iterations, loop_ms (x), form_ms + loop_ms (x)" % ("", method, mode))
                b_it, b_ms, _ = base["solve"][(mode, method)]
                b_all = base["form"]["form_ms"] + b_ms
                for k, r in rows.items():
                    it, ms, met = r["solve"][(mode, method)]
                    tot = r["form"]["form_ms"] + ms
                    emit("%-6s %6d%s %10.1f (%s) %10.1f (%s)" % (k, it, " " if met else "!", ms, ratio(ms, b_ms), tot,
                                                                ratio(tot, b_all)))


if __name__ == "__main__":
    main()
