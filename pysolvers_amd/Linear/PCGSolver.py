"""Preconditioned CG: factory ``PCG`` and solver ``PCGSolver`` (PCGSolver.py:25-142).

``PCG(control, precond, name).makeSolver().solve(A, b)`` runs the whole CG loop
(SpMV, dots, updates, preconditioner apply, convergence test) on the GPU via
``psk_pcg``; results follow the reference's SolveStatus conventions
(iters=k+1 on convergence, k on maxiter failure, breakdown -> soln=None).
``solveMany(A, B)`` solves the columns of a 2-D ``B`` on one matrix through
``psk_pcg_multi``, up to ``PSK_PCG_MULTI_MAX`` columns per device loop.
"""
import ctypes

import numpy as np

from .. import _native as N
from ..IterativeSolver import CommonSolverArgs
from .DeviceMatrix import DeviceCSR
from .IterativeLinearSolver import IterativeLinearSolver, IterativeLinearSolverType
from .PreconditionerType import IdentityPreconditionerType


class PCG(IterativeLinearSolverType):
    def __init__(self, control=CommonSolverArgs(), precond=IdentityPreconditionerType(), name='PCG'):
        super().__init__(control=control, precond=precond, name=name)

    def makeSolver(self, name=None):
        return PCGSolver(self.control(), precond=self.precond(), name=self.name() if name is None else name)


class PCGSolver(IterativeLinearSolver):
    _entry = "psk_pcg"
    _echo_setup = True     # the reference's two setup prints (PCGSolver.py:91,93)

    def __init__(self, control=CommonSolverArgs(), precond=IdentityPreconditionerType(), name='PCG'):
        super().__init__(control=control, precond=precond, name=name)

    def solve(self, A, b):
        return self._device_solve(A, b)

    def solveMany(self, A, B):
        """One SolveStatus per column of the 2-D host array B (any number of columns >= 1), each what
        ``solve(A, B[:, j])`` returns for that column alone: soln(), iters(), resid(), msg() and info["hist"].
        The columns go to psk_pcg_multi in groups of PSK_PCG_MULTI_MAX: one device loop per group, the matrix
        streamed once per iteration for the whole group, every column an independent PCG that stops on its own
        residual. A preconditioner other than the identity or Jacobi, a sharded matrix and a caller's norm
        other than the 2-norm are solved column by column through solve()."""
        assert getattr(B, "ndim", None) == 2, "solveMany: B must be 2-D, one right-hand side per column"
        n, nc = A.shape
        sharded = isinstance(A, DeviceCSR) and A.comm is not None
        if not sharded:
            assert n == nc                                   # PCGSolver.py:79-81
        assert n == B.shape[0] and B.shape[1] >= 1           # PCGSolver.py:83
        Bh = np.asarray(B, dtype=np.float64)
        dA = None if sharded or self._custom_norm() else self._device_matrix(A)
        kind = None
        if dA is not None:
            if self._echo_setup:                             # PCGSolver.py:91
                print('prec frozen = ', self.precFrozen())
            if self.precond is None or not self.precFrozen():   # PCGSolver.py:92-94
                if self._echo_setup:
                    print('building prec')
                self.precond = self.precondType().form(dA)
            kind = getattr(self.precond, "device_kind", None)
        if dA is None:
            return [self.solve(A, np.ascontiguousarray(Bh[:, j])) for j in range(Bh.shape[1])]
        if kind not in (N.PSK_PREC_IDENTITY, N.PSK_PREC_JACOBI):
            # the preconditioner formed above serves every column: solve() on the uploaded matrix with it frozen
            # (and the setup lines, printed once above, not echoed again)
            frozen, echo = self._precFrozen, self._echo_setup
            self._precFrozen, self._echo_setup = True, False
            try:
                return [self.solve(dA, np.ascontiguousarray(Bh[:, j])) for j in range(Bh.shape[1])]
            finally:
                self._precFrozen, self._echo_setup = frozen, echo
        ph = None if kind == N.PSK_PREC_IDENTITY else self.precond.device_handle
        maxiter = int(self.maxiter())
        out = []
        for j0 in range(0, Bh.shape[1], N.PSK_PCG_MULTI_MAX):
            Bg = np.ascontiguousarray(Bh[:, j0:j0 + N.PSK_PCG_MULTI_MAX])
            m = Bg.shape[1]
            ctl = N.PskCtl(maxiter=maxiter, tau=float(self.tau()), fail_on_maxiter=int(bool(self.failOnMaxiter())),
                           restart=0, check_every=0, time_kernels=int(bool(self.time_kernels)), norm_b=0.0)
            res = (N.PskResult * m)()
            hist = np.zeros((m, max(maxiter, 1)), dtype=np.float64)
            X = np.empty_like(Bg)
            N.check(N.lib.psk_pcg_multi(dA.handle, ph, m, N.ptr(Bg), N.ptr(X), ctypes.byref(ctl), res, N.ptr(hist),
                                        N.PSK_HOST), "psk_pcg_multi")
            out += [self._to_status(res[j], np.ascontiguousarray(X[:, j]), hist[j, :res[j].hist_len]) for j in range(m)]
        return out
