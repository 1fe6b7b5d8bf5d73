"""Right-preconditioned IDR(s): factory ``IDRs`` and ``IDRsSolver`` (no reference counterpart).

The short-recurrence Krylov method for nonsymmetric systems between BiCGStab and GMRES: a fixed footprint of about
``2 s + 6`` vectors, one SpMV and one preconditioner apply per step, and for ``s`` = 4..8 matrix-vector counts close
to full GMRES. The whole loop, its dot products, the small triangular solves, the breakdown and convergence tests
and the history run on the GPU (``psk_idrs``; include/psk.h states the recurrence). One step is one SpMV:
``iters()``, ``maxiter`` and the history count steps. A tolerance exit is checked against the true residual
``||b - A x||`` the way BiCGStab's is; ``Mm[k][k]``, ``dot(t,t)`` or ``dot(t,r)`` equal to zero is a breakdown status.
The shadow space is generated from a fixed hash, so two solves give the same bits.
"""
from .. import _native as N
from ..IterativeSolver import CommonSolverArgs
from .IterativeLinearSolver import IterativeLinearSolver, IterativeLinearSolverType
from .PreconditionerType import IdentityPreconditionerType


def _checked_s(s):
    if isinstance(s, bool) or int(s) != s or not 1 <= int(s) <= N.PSK_IDRS_MAX_S:
        raise ValueError("IDR(s): s must be an integer in 1..%d, got %r" % (N.PSK_IDRS_MAX_S, s))
    return int(s)


class IDRs(IterativeLinearSolverType):
    def __init__(self, control=CommonSolverArgs(), precond=IdentityPreconditionerType(), s=4, name='IDRs'):
        super().__init__(control=control, precond=precond, name=name)
        self._s = _checked_s(s)

    def s(self):
        return self._s

    def makeSolver(self, name=None):
        return IDRsSolver(self.control(), precond=self.precond(), s=self._s,
                          name=self.name() if name is None else name)


class IDRsSolver(IterativeLinearSolver):
    _entry = "psk_idrs"
    _method = "IDR(s)"

    def __init__(self, control=CommonSolverArgs(), precond=IdentityPreconditionerType(), s=4, name='IDRs'):
        super().__init__(control=control, precond=precond, name=name)
        self._s = _checked_s(s)

    def s(self):
        return self._s

    def _call_entry(self, A, M, b, x, ctl, res, hist, loc):
        return N.lib.psk_idrs(A, M, b, x, ctl, self._s, res, hist, loc)

    def _to_status(self, res, x, hist):
        st = super()._to_status(res, x, hist)
        st.info["s"] = self._s
        return st

    def solve(self, A, b):
        return self._device_solve(A, b)
