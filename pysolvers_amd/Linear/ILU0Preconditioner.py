"""ILU(0) preconditioners: factors formed AND applied on the GPU (pysolvers_amd/csrc/ilu0.hip).

No reference counterpart: the reference's incomplete factorisations are SuperLU's ``spilu``
(ILUTPreconditioner.py:51-53). ILU(0) keeps A's own pattern — L = strict-lower(F) with a unit diagonal,
U = upper(F), F on the sorted pattern of A — so it adds no fill, its size is limited by HBM rather than by
SuperLU, and a 5-point grid of m lines has 2m - 1 dependency levels. ``form(A)`` takes a scipy matrix or a
``DeviceCSR`` and calls ``psk_prec_create_ilu0``: the numeric factorisation runs on the device, one launch per
dependency level, and the factors go to the triangular-solve chain every other ILU / IC / Gauss-Seidel apply
uses (a ``PSK_PREC_ILU``; the host planner picks each factor's schedule). The arithmetic is defined to the bit
in include/psk.h (``psk_csr_ilu0``). The class layout mirrors ILUTPreconditioner.py: a LEFT ILU(0) is the
identity when applied from the right (Preconditioner.py:39-46).
"""
import ctypes

from .. import _native as N
from .DeviceMatrix import as_device_matrix
from .Preconditioner import DeviceOperator, LeftPreconditioner, Preconditioner, RightPreconditioner
from .PreconditionerType import PreconditionerType
from .TriangularSolve import TriangularSolveChain, apply_sweeps


class LeftILU0(PreconditionerType):
    """sweeps: None (exact triangular solves), an int s or a pair (s_L, s_U): that many Jacobi sweeps replace the
    solve of each factor (TriangularSolveChain.sweeps; 0 keeps a factor exact)."""

    def __init__(self, sweeps=None):
        self.sweeps = sweeps

    def form(self, A):
        return LeftILU0Preconditioner(A, sweeps=self.sweeps)


class RightILU0(PreconditionerType):
    """sweeps: as LeftILU0."""

    def __init__(self, sweeps=None):
        self.sweeps = sweeps

    def form(self, A):
        return RightILU0Preconditioner(A, sweeps=self.sweeps)


class ILU0Preconditioner(DeviceOperator, Preconditioner):
    def __init__(self, A, sweeps=None):
        dA = as_device_matrix(A)
        if dA.comm is not None:
            raise ValueError("ILU(0) of a sharded matrix is not supported")
        h = ctypes.c_void_p()
        N.check(N.lib.psk_prec_create_ilu0(dA.handle, ctypes.byref(h)), "psk_prec_create_ilu0")
        self._h = h
        self.n = dA.n
        self._A = dA        # for factors(); the handle itself borrows nothing
        self._F = None
        apply_sweeps(self, sweeps)

    def factors(self):
        """F as a scipy CSR with sorted rows: L = strict-lower(F) with a unit diagonal, U = upper(F). The chain
        keeps the two factors in its schedules' layouts, so F is factored again (``DeviceCSR.ilu0``: the same
        bits) at the first call and kept."""
        if self._F is None:
            F = self._A.ilu0().to_scipy()
            F.has_sorted_indices = True
            self._F = F
        return self._F

    # schedule('L' | 'U', set=None), grid_info and sweeps('L' | 'U', set=None): psk_prec_trisolve_schedule /
    # _grid_info / _sweeps on the chain
    schedule = TriangularSolveChain.schedule
    grid_info = TriangularSolveChain.grid_info
    sweeps = TriangularSolveChain.sweeps


class LeftILU0Preconditioner(ILU0Preconditioner, LeftPreconditioner):
    """applyRight is the identity (Preconditioner.py:44-45)."""

    device_kind = N.PSK_PREC_IDENTITY
    device_handle = None

    def applyLeft(self, vec):
        return self._device_apply(vec)


class RightILU0Preconditioner(ILU0Preconditioner, RightPreconditioner):
    device_kind = N.PSK_PREC_ILU

    def applyRight(self, vec):
        return self._device_apply(vec)
