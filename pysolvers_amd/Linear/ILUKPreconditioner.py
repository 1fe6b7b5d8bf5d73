"""Level-of-fill ILU(k) preconditioners: pattern, factors and applies all on the GPU (pysolvers_amd/csrc/iluk.hip).

No reference counterpart: the reference's incomplete factorisations are SuperLU's ``spilu``
(ILUTPreconditioner.py:51-53). ILU(k) first adds to A's pattern every fill entry of level <= k (include/psk.h,
``psk_csr_iluk_pattern``: a stored entry has level 0, a fill entry (i, j) the smallest lev(i,c) + lev(c,j) + 1 over
the pivots c that create it), in k row-parallel rounds on the device, and pads A with zeros onto that pattern; the
numeric factorisation is then ILU(0)'s on the padded matrix, kernel and bits unchanged, and the factors go to the
triangular-solve chain every other ILU / IC / Gauss-Seidel apply uses (a ``PSK_PREC_ILU``). ``k = 0`` is RightILU0 to
the bit; a larger k buys fewer Krylov iterations for more entries and more dependency levels (DESIGN.md has the
measured trade). The class layout mirrors ILU0Preconditioner.py: a LEFT ILU(k) is the identity when applied from
the right (Preconditioner.py:39-46).
"""
import ctypes
import numbers

from .. import _native as N
from .DeviceMatrix import as_device_matrix
from .Preconditioner import DeviceOperator, LeftPreconditioner, Preconditioner, RightPreconditioner
from .PreconditionerType import PreconditionerType
from .TriangularSolve import TriangularSolveChain, apply_sweeps

ILUK_MAX_LEVEL = 8   # PSK_ILUK_MAX_LEVEL


def check_level(k):
    """k as an int in [0, ILUK_MAX_LEVEL]; ValueError for a bool, a non-integer or a value out of range."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral):
        raise ValueError("the ILU(k) level must be an integer, not %r" % (k,))
    if not 0 <= int(k) <= ILUK_MAX_LEVEL:
        raise ValueError("the ILU(k) level must lie in [0, %d], not %d" % (ILUK_MAX_LEVEL, int(k)))
    return int(k)


class LeftILUK(PreconditionerType):
    """k: the level of fill (0 .. 8). sweeps: None (exact triangular solves), an int s or a pair (s_L, s_U): that
    many Jacobi sweeps replace the solve of each factor (TriangularSolveChain.sweeps; 0 keeps a factor exact)."""

    def __init__(self, k=1, sweeps=None):
        self.k = check_level(k)
        self.sweeps = sweeps

    def form(self, A):
        return LeftILUKPreconditioner(A, k=self.k, sweeps=self.sweeps)


class RightILUK(PreconditionerType):
    """k, sweeps: as LeftILUK."""

    def __init__(self, k=1, sweeps=None):
        self.k = check_level(k)
        self.sweeps = sweeps

    def form(self, A):
        return RightILUKPreconditioner(A, k=self.k, sweeps=self.sweeps)


class ILUKPreconditioner(DeviceOperator, Preconditioner):
    def __init__(self, A, k=1, sweeps=None):
        k = check_level(k)
        dA = as_device_matrix(A)
        if dA.comm is not None:
            raise ValueError("ILU(k) of a sharded matrix is not supported")
        h = ctypes.c_void_p()
        N.check(N.lib.psk_prec_create_iluk(dA.handle, k, ctypes.byref(h)), "psk_prec_create_iluk")
        self._h = h
        self.n = dA.n
        self.level = k
        self._A = dA        # for factors(); the handle itself borrows nothing
        self._F = None
        info = self.device_info()
        self.fill_ratio = (info["nnz_l"] + info["nnz_u"] + self.n) / float(dA.nnz)   # nnz(F) / nnz(A)
        apply_sweeps(self, sweeps)

    def factors(self):
        """F as a scipy CSR with sorted rows on the ILU(k) pattern: L = strict-lower(F) with a unit diagonal,
        U = upper(F). The chain keeps the two factors in its schedules' layouts, so the pattern is built and factored
        again (``DeviceCSR.iluk_pattern(k).ilu0()``: the same bits) at the first call and kept."""
        if self._F is None:
            F = self._A.iluk_pattern(self.level).ilu0().to_scipy()
            F.has_sorted_indices = True
            self._F = F
        return self._F

    # schedule('L' | 'U', set=None), grid_info and sweeps('L' | 'U', set=None): psk_prec_trisolve_schedule /
    # _grid_info / _sweeps on the chain
    schedule = TriangularSolveChain.schedule
    grid_info = TriangularSolveChain.grid_info
    sweeps = TriangularSolveChain.sweeps


class LeftILUKPreconditioner(ILUKPreconditioner, LeftPreconditioner):
    """applyRight is the identity (Preconditioner.py:44-45)."""

    device_kind = N.PSK_PREC_IDENTITY
    device_handle = None

    def applyLeft(self, vec):
        return self._device_apply(vec)


class RightILUKPreconditioner(ILUKPreconditioner, RightPreconditioner):
    device_kind = N.PSK_PREC_ILU

    def applyRight(self, vec):
        return self._device_apply(vec)
