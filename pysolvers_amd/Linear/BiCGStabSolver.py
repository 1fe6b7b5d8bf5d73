"""Right-preconditioned BiCGStab: factory ``BiCGStab`` and ``BiCGStabSolver`` (no reference counterpart).

The short-recurrence Krylov method for nonsymmetric systems: about eight vectors and two SpMVs per
iteration whatever the iteration count, no restart parameter. The whole loop, its dot products, the
breakdown and convergence tests and the history run on the GPU (``psk_bicgstab``, include/psk.h states the
recurrence). A tolerance exit is checked against the true residual ``||b - A x||`` the way GMRES's is;
``dot(rhat,v)``, ``dot(t,t)``, ``omega`` or ``dot(rhat,r)`` equal to zero is a breakdown status.
"""
from ..IterativeSolver import CommonSolverArgs
from .IterativeLinearSolver import IterativeLinearSolver, IterativeLinearSolverType
from .PreconditionerType import IdentityPreconditionerType


class BiCGStab(IterativeLinearSolverType):
    def __init__(self, control=CommonSolverArgs(), precond=IdentityPreconditionerType(), name='BiCGStab'):
        super().__init__(control=control, precond=precond, name=name)

    def makeSolver(self, name=None):
        return BiCGStabSolver(self.control(), precond=self.precond(), name=self.name() if name is None else name)


class BiCGStabSolver(IterativeLinearSolver):
    _entry = "psk_bicgstab"
    _method = "BiCGStab"

    def __init__(self, control=CommonSolverArgs(), precond=IdentityPreconditionerType(), name='BiCGStab'):
        super().__init__(control=control, precond=precond, name=name)

    def solve(self, A, b):
        return self._device_solve(A, b)
