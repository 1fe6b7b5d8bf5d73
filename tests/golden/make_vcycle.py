#!/usr/bin/env python3
"""Golden fixtures for the standalone AMG V-cycle solver, made by running the REFERENCE itself.

Runs the reference's ``AMGVCycle(...).makeSolver().solve(A, b)`` (VCycleSolver.py:15-95) with reportIter captured,
ASSERTS bit-identity with the CPU restatement (tests/vcycle_oracle.py: the loop over oracle.amg.hierarchy /
oracle.amg.vcycle) and writes inputs and the reference's outputs as data only: tests/golden/vcycle.npz and
tests/golden/manifest_vcycle.json. The manifest also records, as data, the constructor parameters of the
reference's two classes and the lines one verbose solve prints.

Every converging case must keep min_k |hist_k / (tau ||b||) - 1| >= 0.05 (asserted): a residual that far from
the threshold on both sides of the stopping cycle cannot change side on rounding, so the GPU test demands equal
iteration counts on every case. Run only in the build container (the GPU box has no /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vcycle.py
"""
import contextlib
import inspect
import io
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg   # noqa: E402  (installs the PyTab/PyTimer stand-ins and imports the reference)
from vcycle_oracle import vcycle_solve   # noqa: E402

from PySolvers import CommonSolverArgs                                        # noqa: E402
from PySolvers.Linear import AMGVCycle, AMGVCycleSolver                      # noqa: E402
from PySolvers.Linear.ClassicSmoothers import JacobiSmoother                 # noqa: E402

TAU, MAXITER, MIN_MARGIN = 1e-10, 60, 0.05

# (matrix, numLevels, smoother, maxiter, failOnMaxiter, cycles to converge or None)
CASES = [
    ("dh8", 2, "gs", MAXITER, True, 15),
    ("dh8", 3, "gs", MAXITER, True, 16),
    ("dh8", 1, "gs", MAXITER, True, 1),
    ("dh8", 2, "jacobi", MAXITER, True, None),
    ("dh8", 2, "jacobi", MAXITER, False, None),
    ("dh10", 2, "gs", MAXITER, True, 16),
    ("dh10", 3, "gs", MAXITER, True, 29),
    ("negfd16", 2, "gs", MAXITER, True, 11),
    ("negfd16", 3, "gs", MAXITER, True, 11),
    ("negfd32", 2, "gs", MAXITER, True, 12),
    ("negfd32", 3, "gs", MAXITER, True, 15),
    ("negfd32", 2, "jacobi", MAXITER, True, None),
    ("negfd32", 2, "jacobi", MAXITER, False, None),
    ("negfd16", 2, "gs", 3, True, None),
]


def _matrix(name):
    if name.startswith("dh"):
        return sp.csr_matrix(mg._dh(int(name[2:])))
    return sp.csr_matrix(-mg.ref_fd2d(-1.0, 1.0, int(name[5:])))


def _tag(name, L, sm, maxiter, fom):
    t = "%s_L%d_%s" % (name, L, sm)
    if maxiter != MAXITER:
        t += "_maxiter%d" % maxiter
    if not fom:
        t += "_nofail"
    return t


def _run_ref(A, b, L, sm, maxiter, fom, show=False):
    ctl = CommonSolverArgs(maxiter=maxiter, tau=TAU, failOnMaxiter=fom, showIters=show, showFinal=show)
    kw = {"smoother": JacobiSmoother} if sm == "jacobi" else {}
    solver = AMGVCycle(ctl, numLevels=L, **kw).makeSolver()
    hist = []
    if not show:
        solver.reportIter = lambda it, nr, n0: hist.append(float(nr))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = solver.solve(A, b)
    return res, np.array(hist), out.getvalue()


def _params(cls):
    """Constructor parameters as data: name and default (numbers as they are, classes and instances by class name)."""
    out = []
    for p in list(inspect.signature(cls.__init__).parameters.values())[1:]:
        d = p.default
        if isinstance(d, (int, float, str)) or d is None:
            dd = dict(value=d)
        elif inspect.isclass(d):
            dd = dict(cls=d.__name__)
        else:
            dd = dict(instance_of=type(d).__name__)
        out.append(dict(name=p.name, default=dd))
    return out


def main():
    rng = np.random.default_rng(7)
    mats, rhs, fix, index = {}, {}, {}, []
    for name, L, sm, maxiter, fom, want in CASES:
        if name not in mats:
            mats[name] = _matrix(name)
            rhs[name] = rng.standard_normal(mats[name].shape[0])
            for k, v in mg._csr_arrays(mats[name]).items():
                fix["%s_%s" % (name, k)] = v
            fix[name + "_b"] = rhs[name]
        A, b = mats[name], rhs[name]
        tag = _tag(name, L, sm, maxiter, fom)
        res, hist, _ = _run_ref(A, b, L, sm, maxiter, fom)
        orc = vcycle_solve(A, b, num_levels=L, smoother=sm, maxiter=maxiter, tau=TAU, fail_on_maxiter=fom)
        mg._check_same(tag, res, hist, orc)
        assert res.msg() == orc["msg"], tag
        nb = np.linalg.norm(b)
        converged = bool(bool(res.success()) and hist[-1] < TAU * nb)
        assert (res.iters() if converged else None) == want, (tag, res.iters(), converged, want)
        margin = None
        if converged and L > 1:
            margin = float(np.min(np.abs(hist / (TAU * nb) - 1.0)))
            assert margin >= MIN_MARGIN, (tag, margin)
        fix[tag + "_hist"] = hist
        fix[tag + "_soln"] = res.soln()
        fix[tag + "_iters"] = np.int64(res.iters())
        fix[tag + "_success"] = np.int64(bool(res.success()))
        fix[tag + "_resid"] = np.float64(res.resid())
        index.append(dict(tag=tag, matrix=name, n=int(A.shape[0]), num_levels=L, smoother=sm, maxiter=maxiter, tau=TAU,
                          fail_on_maxiter=fom, iters=int(res.iters()), success=bool(res.success()), msg=res.msg(),
                          hist_len=int(len(hist)), converged=converged, margin=margin,
                          rate=None if converged else float((hist[-1] / hist[-11]) ** 0.1) if len(hist) > 10 else None))
        print("%-34s iters=%3d success=%-5s hist=%2d margin=%s" % (tag, res.iters(), res.success(), len(hist), margin))
    # b = 0 (VCycleSolver.py:63-65): iters = 1, x = 0, nothing reported
    res, hist, _ = _run_ref(mats["dh8"], np.zeros(mats["dh8"].shape[0]), 2, "gs", MAXITER, True)
    assert res.iters() == 1 and res.success() and not np.any(res.soln()) and len(hist) == 0
    # what a verbose solve prints (the factory's solver name included)
    _, _, printed = _run_ref(mats["negfd16"], rhs["negfd16"], 2, "gs", 3, True, show=True)
    np.savez_compressed(os.path.join(HERE, "vcycle.npz"), **fix)
    import scipy
    with open(os.path.join(HERE, "manifest_vcycle.json"), "w") as f:
        json.dump(dict(cases=index, zero_rhs=dict(iters=1, success=True, resid=0),
                       signatures=dict(AMGVCycle=_params(AMGVCycle), AMGVCycleSolver=_params(AMGVCycleSolver)),
                       printed=dict(tag=_tag("negfd16", 2, "gs", 3, True),   # the solver's lines, not the setup's chatter
                                    lines=[ln for ln in printed.splitlines() if " iter=" in ln or " solve " in ln]),
                       generator="tests/golden/make_vcycle.py", numpy=np.__version__, scipy=scipy.__version__),
                  f, indent=1)
    print("wrote", len(index), "vcycle cases")


if __name__ == "__main__":
    main()
