"""The AMG V-cycle as a solver of its own: factory ``AMGVCycle`` and solver ``AMGVCycleSolver``
(VCycleSolver.py:15-95).

``AMGVCycle(control, numLevels, nuPre, nuPost, smoother).makeSolver().solve(A, b)`` builds the
smoothed-aggregation hierarchy (an ``AMGPreconditioner``: host setup, every level resident in HBM) and
hands the whole loop of VCycleSolver.py:78-95 to ``psk_vcycle`` (pysolvers_amd/csrc/vcycle.hip):
x0 = copy(b); per cycle x = runCycle(b, x), r = b - A x, reportIter, stop on ||r|| < tau ||b|| (strict).
The device keeps the history and the iterate of the converging cycle; the host only polls a done word.
Status conventions are the reference's: iters = k+1 on convergence, handleMaxiter(maxiter-1, ...) otherwise.

The hierarchy is rebuilt on every solve unless ``freezeMatrix()`` was called and one exists (:71).

As in the reference, the factory does not hand its ``name`` argument to its base class (VCycleSolver.py:20),
so ``AMGVCycle(...).makeSolver()`` names the solver '' unless ``makeSolver(name=...)`` is given one; the
solver class itself defaults to 'AMGVCycle'.
"""
import ctypes

import numpy as np

from .. import _native as N
from ..IterativeSolver import CommonSolverArgs
from .AMGPreconditioner import AMGPreconditioner
from .SmoothedAggregation import check_setup
from .ClassicSmoothers import GaussSeidelSmoother
from .DeviceMatrix import DeviceVector, spmv
from .IterativeLinearSolver import (IterativeLinearSolver, IterativeLinearSolverType, _host_copy, _is_zero_norm,
                                    _like)


class _TakesSetup(type(IterativeLinearSolver)):
    """The product-only keyword ``setup="host" | "device"`` (where the AMG hierarchy is built, AMGPreconditioner.py)
    of the two classes below. Their ``__init__`` signatures stay the reference's, parameter for parameter
    (tests/test_vcycle_api.py pins them against it), so the keyword is taken by the class call:
    ``AMGVCycle(control, numLevels=3, setup="device")``. Anything but "host" or "device" raises ValueError."""

    def __call__(cls, *args, setup="host", **kwargs):
        check_setup(setup)
        obj = super().__call__(*args, **kwargs)
        obj.setup = setup
        return obj


class AMGVCycle(IterativeLinearSolverType, metaclass=_TakesSetup):

    def __init__(self, control=CommonSolverArgs(), numLevels=2, nuPre=2, nuPost=2, smoother=GaussSeidelSmoother,
                 name='AMGVCycle'):
        super().__init__(control=control, precond=None)          # VCycleSolver.py:20 (name not passed on)
        self.setup = "host"                                      # _TakesSetup: where the hierarchy is built
        self.numLevels = numLevels
        self.nuPre = nuPre
        self.nuPost = nuPost
        self.smoother = smoother

    def makeSolver(self, name=None):
        """Creates an AMG V-cycle solver object with the specified parameters (VCycleSolver.py:26-36)."""
        return AMGVCycleSolver(name=self.name() if name is None else name, control=self.control(),
                               numLevels=self.numLevels, nuPre=self.nuPre, nuPost=self.nuPost,
                               smoother=self.smoother, setup=self.setup)


class AMGVCycleSolver(IterativeLinearSolver, metaclass=_TakesSetup):
    _entry = "psk_vcycle"

    def __init__(self, control=CommonSolverArgs(), numLevels=2, nuPre=2, nuPost=2, smoother=GaussSeidelSmoother,
                 name='AMGVCycle'):
        super().__init__(control=control, name=name, precond=None)
        self.setup = "host"        # _TakesSetup: "host" / "device", where the hierarchy is built
        self.numLevels = numLevels
        self.nuPre = nuPre
        self.nuPost = nuPost
        self.smoother = smoother
        self._cycleMgr = None      # the hierarchy (an AMGPreconditioner), VCycleSolver.py:50
        self.check_every = 0       # psk_ctl.check_every (0 = the library's default); results do not depend on it

    def solve(self, A, b):
        n, nc = A.shape
        assert n == nc                                         # VCycleSolver.py:58
        assert n == len(b)                                     # :60
        custom = self._custom_norm()
        normB = 0.0
        if custom:
            normB = float(self.norm(_host_copy(b)))            # self.norm(b)  :63
            zero_b = normB == 0.0
        else:
            zero_b = _is_zero_norm(b, n)
        if zero_b:                                             # :64-65, before the hierarchy is built
            x0 = DeviceVector(n) if isinstance(b, DeviceVector) else np.zeros(n)
            if isinstance(x0, DeviceVector):
                x0.zero()
            return self.handleConvergence(0, _like(b, x0), 0, 0)
        dA = self._device_matrix(A)
        if self._cycleMgr is None or not self.matrixFrozen():  # :71-76
            # numIters and tau are the preconditioner apply's; psk_vcycle takes its own from the control
            self._cycleMgr = AMGPreconditioner(dA, numIters=1, numLevels=self.numLevels, nuPre=self.nuPre,
                                               nuPost=self.nuPost, smoother=self.smoother, tau=0.0,
                                               setup=self.setup)
        if custom:
            return self._host_norm_vcycle(dA, b, normB)
        maxiter = int(self.maxiter())
        ctl = N.PskCtl(maxiter=maxiter, tau=float(self.tau()), fail_on_maxiter=int(bool(self.failOnMaxiter())),
                       restart=0, check_every=int(self.check_every), time_kernels=0, norm_b=0.0)
        res = N.PskResult()
        hist = np.zeros(max(maxiter, 1), dtype=np.float64)
        x, loc, bp = self._solve_vectors(b, n)
        N.check(N.lib.psk_vcycle(self._cycleMgr.device_handle, N.ptr(bp), N.ptr(x), ctypes.byref(ctl),
                                 ctypes.byref(res), N.ptr(hist), 0, loc), "psk_vcycle")
        return self._to_status(res, x, hist[:res.hist_len])

    def _host_norm_vcycle(self, dA, b, normB):
        """The loop of VCycleSolver.py:78-95 with a caller-supplied norm, driven from the host: the reference
        evaluates self.norm(r) on every residual (:87) and that is the caller's host code. One psk_vcycle call
        per cycle (maxiter=1, tau=0, no failure, starting from the current x), r = b - A x through the device
        SpMV, copied to the host for the norm. Same operations and status conventions as the device loop."""
        n = dA.n
        bh = _host_copy(b)
        bd = b if isinstance(b, DeviceVector) else DeviceVector.from_numpy(bh)
        x = DeviceVector.from_numpy(bh)                                # x = copy(b)  :69
        ctl = N.PskCtl(maxiter=1, tau=0.0, fail_on_maxiter=0, restart=0, check_every=0, time_kernels=0, norm_b=0.0)
        res = N.PskResult()

        def result():                                                  # the kind of vector the caller passed
            return x if isinstance(b, DeviceVector) else _like(b, x.numpy())

        hist = []
        for k in range(self.maxiter()):                                # :79
            N.check(N.lib.psk_vcycle(self._cycleMgr.device_handle, bd._p, x._p, ctypes.byref(ctl), ctypes.byref(res),
                                     None, N.PSK_VCYCLE_X0_GIVEN, N.PSK_DEVICE), "psk_vcycle")   # :81
            r = bh - spmv(dA, x).numpy()                               # :84
            normR = float(self.norm(r))                                # :87
            hist.append(normR)
            self.reportIter(k, normR, normB)                           # :89
            if normR < self.tau() * normB:                             # :90
                st = self.handleConvergence(k, result(), normR, normB)
                st.info = dict(status="converged", hist=np.array(hist), norm_b=normB, host_driven=True)
                return st
        st = self.handleMaxiter(k, result(), normR, normB)             # :95 (maxiter <= 0: NameError, as there)
        st.info = dict(status="maxiter", hist=np.array(hist), norm_b=normB, host_driven=True)
        return st
