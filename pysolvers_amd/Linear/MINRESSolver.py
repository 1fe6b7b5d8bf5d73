"""Preconditioned MINRES: factory ``MINRES`` and ``MINRESSolver`` (no reference counterpart).

The short-recurrence Krylov method for SYMMETRIC INDEFINITE systems (shifted and Helmholtz-type operators,
saddle-point and KKT matrices), where PCG has no guarantee and GMRES pays a growing basis for a symmetry that
makes a three-term recurrence exact: one SpMV, two dot products and a fixed footprint per iteration, no restart
parameter. The preconditioner must be symmetric positive definite. The whole loop, its dot products, the plane
rotations, the convergence test and the history run on the GPU (``psk_minres``; include/psk.h states the
recurrence, which is scipy.sparse.linalg.minres's with x0 = 0 and no shift).

The norm in which convergence is judged: the history is ``||r_k||`` in the M^-1 norm (``sqrt(r.M^-1 r)``, the
quantity MINRES minimises), scaled so that ``hist[k] / ||b||`` is the relative reduction in that norm; the solve
stops when it is ``<= tau``. With the identity preconditioner that is ``||b - A x_k||_2`` and a tolerance exit is
checked against the true residual the way GMRES's is (a miss is a failure whose message starts "MINRES failure:
true residual"). Under a preconditioner the solve's contract is the preconditioned norm: the status stays
converged, ``resid()`` still reports the true 2-norm residual, and that is bounded by
``||r||_2 / ||b||_2 <= sqrt(cond(M)) * tau``, not by ``tau`` (Jacobi runs on shifted Laplacians end at 1.1-1.2 tau;
that is inherent, not drift). A preconditioner that is not positive definite (``r.M^-1 r < 0``) and ``gamma == 0``
(a singular system) are breakdown statuses.
"""
from .. import _native as N
from ..IterativeSolver import CommonSolverArgs
from .IterativeLinearSolver import IterativeLinearSolver, IterativeLinearSolverType
from .PreconditionerType import IdentityPreconditionerType


class MINRES(IterativeLinearSolverType):
    def __init__(self, control=CommonSolverArgs(), precond=IdentityPreconditionerType(), name='MINRES'):
        super().__init__(control=control, precond=precond, name=name)

    def makeSolver(self, name=None):
        return MINRESSolver(self.control(), precond=self.precond(), name=self.name() if name is None else name)


class MINRESSolver(IterativeLinearSolver):
    _entry = "psk_minres"
    _method = "MINRES"

    def __init__(self, control=CommonSolverArgs(), precond=IdentityPreconditionerType(), name='MINRES'):
        super().__init__(control=control, precond=precond, name=name)

    def _retests_true_residual(self, kind):
        """A caller's norm re-tests the true residual only under the identity: with a preconditioner the
        threshold is one on the M^-1 norm and the 2-norm residual is not held to it."""
        return kind == N.PSK_PREC_IDENTITY

    def solve(self, A, b):
        return self._device_solve(A, b)
