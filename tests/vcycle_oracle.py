"""CPU restatement of AMGVCycleSolver.solve (VCycleSolver.py:52-95) over oracle.amg (TEST INFRASTRUCTURE).

The loop around oracle.amg.vcycle, with the reference's stopping test (strict <) and status conventions
(IterativeSolver.py:101-129). tests/golden/make_vcycle.py pins it bitwise against the reference's own runs;
tests/test_gpu_vcycle.py uses it where the reference's quadratic setup is too slow.
"""
import numpy as np

from oracle import amg


def vcycle_solve(A, b, num_levels=2, smoother="gs", maxiter=100, tau=1e-8, fail_on_maxiter=True, tri=False,
                 norm=np.linalg.norm, levels=None):
    """dict(iters, success, msg, hist, soln, resid). levels: a prebuilt (ops, P, R); tri: see oracle.amg.smooth."""
    ops, P, R = levels if levels is not None else amg.hierarchy(A, num_levels)
    aux = [amg.smoother_aux(smoother, M) for M in ops]
    norm_b = norm(b)
    if norm_b == 0.0:                                          # :64-65 handleConvergence(0, zeros, 0, 0)
        return dict(iters=1, success=True, msg=None, hist=np.zeros(0), soln=np.zeros_like(b), resid=0)
    x = np.copy(b)                                             # :69
    hist = []
    for k in range(maxiter):                                   # :79
        x = amg.vcycle(ops, P, R, aux, smoother, b, x, len(ops) - 1, tri=tri)   # :81
        norm_r = norm(b - A * x)                               # :84, :87
        hist.append(float(norm_r))                             # reportIter  :89
        if norm_r < tau * norm_b:                              # :90
            return dict(iters=k + 1, success=True, msg=None, hist=np.array(hist), soln=x, resid=norm_r)
    # handleMaxiter(k = maxiter - 1, ...)  :95, IterativeSolver.py:115-129
    return dict(iters=maxiter - 1, success=not fail_on_maxiter, msg='failure to converge' if fail_on_maxiter else None,
                hist=np.array(hist), soln=x, resid=norm_r)
