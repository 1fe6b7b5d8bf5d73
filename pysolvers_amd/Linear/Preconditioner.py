"""Preconditioner plugin classes (same hierarchy as Linear/Preconditioner.py:3-68).

Preconditioners that run inside the device Krylov loop expose a ``device_kind``
and a ``device_handle`` (a libpsk psk_prec*). ``applyLeft/applyRight`` keep the
reference's host-callable contract: they take and return a vector.
"""
import ctypes
from abc import ABC, abstractmethod

import numpy as np

from .. import _native as N
from .DeviceMatrix import DeviceVector, as_device_matrix, is_device_vector, matmat, torch_stream_ready


class Preconditioner(ABC):
    """Two-sided preconditioner interface (Preconditioner.py:3-18)."""

    device_kind = None

    @abstractmethod
    def applyLeft(self, vec):
        ...

    @abstractmethod
    def applyRight(self, vec):
        ...


class GenericPreconditioner(Preconditioner):
    """Same operator on either side (Preconditioner.py:20-36)."""

    @abstractmethod
    def apply(self, vec):
        ...

    def applyLeft(self, vec):
        return self.apply(vec)

    def applyRight(self, vec):
        return self.apply(vec)


class LeftPreconditioner(Preconditioner):
    """applyRight is the identity (Preconditioner.py:39-46)."""

    def applyRight(self, vec):
        return vec


class RightPreconditioner(Preconditioner):
    """applyLeft is the identity (Preconditioner.py:49-56)."""

    def applyLeft(self, vec):
        return vec


class IdentityPreconditioner:
    """Returns its argument itself (Preconditioner.py:58-68); duck-typed like the reference."""

    device_kind = N.PSK_PREC_IDENTITY
    device_handle = None

    def applyLeft(self, vec):
        return vec

    def applyRight(self, vec):
        return vec


class DeviceOperator:
    """Mixin for preconditioners backed by a libpsk psk_prec handle (self._h, size self.n).

    ``_device_apply`` takes a DeviceVector, a CUDA float64 tensor or a host array and returns the
    same kind; the operator itself always runs on the GPU.
    """

    _h = None
    device_kind = None

    @property
    def device_handle(self):
        return self._h

    def _device_apply(self, vec):
        if isinstance(vec, DeviceVector):
            out = DeviceVector(self.n)
            N.check(N.lib.psk_prec_apply(self._h, self.n, vec._p, out._p, N.PSK_DEVICE), "psk_prec_apply")
            return out
        if is_device_vector(vec):
            import torch
            out = torch.empty_like(vec)
            torch_stream_ready(vec, out)
            N.check(N.lib.psk_prec_apply(self._h, self.n, N.ptr(vec), N.ptr(out), N.PSK_DEVICE), "psk_prec_apply")
            return out
        v = np.ascontiguousarray(vec, dtype=np.float64)
        out = np.empty_like(v)
        N.check(N.lib.psk_prec_apply(self._h, self.n, N.ptr(v), N.ptr(out), N.PSK_HOST), "psk_prec_apply")
        return out

    def device_info(self):
        """kind / size / triangular-solve nnz and dependency levels (psk_prec_info)."""
        return N.prec_info(self._h)

    def __del__(self):
        try:
            if self._h:
                N.lib.psk_prec_destroy(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass


class JacobiPreconditioner(DeviceOperator, GenericPreconditioner):
    """M^-1 v = DInv * v with DInv = reciprocal(diag(A)) formed on the device.

    The reference has Jacobi only as a smoother (ClassicSmoothers.py:5-16:
    ``DInv = np.reciprocal(A.diagonal())``; ``np.multiply(DInv, r)``); this is
    the same operator behind the PreconditionerType plugin API, as config 2 of
    the benchmark needs (PCG + Jacobi).
    """

    device_kind = N.PSK_PREC_JACOBI

    def __init__(self, A):
        self._A = as_device_matrix(A)        # keep the matrix alive as long as DInv
        h = ctypes.c_void_p()
        N.check(N.lib.psk_prec_create(self._A.handle, N.PSK_PREC_JACOBI, ctypes.byref(h)), "psk_prec_create")
        self._h = h
        self.n = self._A.n

    def apply(self, vec):
        return self._device_apply(vec)


class ChebyshevPreconditioner(DeviceOperator, GenericPreconditioner):
    """M^-1 v = the degree-``degree`` Chebyshev polynomial in D^-1 A applied to D^-1 v, D = diag(A), for the
    eigenvalues of D^-1 A in [lmax/ratio, lmax] (psk_prec_create_chebyshev, pysolvers_amd/csrc/cheby.hip).

    No reference counterpart (the reference's smoothers are Jacobi and Gauss-Seidel, ClassicSmoothers.py:5-36):
    the strong smoother without a triangular solve. One pass over A per degree beyond the first, no dependency
    chain; symmetric for symmetric A, so PCG may use it on its own or inside the AMG V-cycle. ``lmax=None`` takes
    the Gershgorin bound of D^-1 A (a true upper bound, loose on badly scaled matrices: pass an estimate of
    the largest eigenvalue then). ``degree=1`` is Jacobi scaled by 1/theta.
    """

    device_kind = N.PSK_PREC_CHEBYSHEV

    def __init__(self, A, degree=3, lmax=None, ratio=30.0):
        self._A = as_device_matrix(A)        # borrowed by the handle: keep it alive
        h = ctypes.c_void_p()
        N.check(N.lib.psk_prec_create_chebyshev(self._A.handle, int(degree), 0.0 if lmax is None else float(lmax),
                                                float(ratio), ctypes.byref(h)), "psk_prec_create_chebyshev")
        self._h = h
        self.n = self._A.n
        self.ratio = float(ratio)

    def _info(self):
        k, hi, lo = N.I32(), N.F64(), N.F64()
        N.check(N.lib.psk_prec_chebyshev_info(self._h, ctypes.byref(k), ctypes.byref(hi), ctypes.byref(lo), None),
                "psk_prec_chebyshev_info")
        return k.value, hi.value, lo.value

    @property
    def degree(self):
        return self._info()[0]

    @property
    def lmax(self):
        """Upper end of the interval: the caller's, or the Gershgorin bound of D^-1 A."""
        return self._info()[1]

    @property
    def lmin(self):
        """lmax / ratio."""
        return self._info()[2]

    @property
    def coefficients(self):
        """c0, then (alpha_k, beta_k) for k = 1..degree-1: 2*degree - 1 doubles (include/psk.h)."""
        c = np.empty(2 * self.degree - 1, dtype=np.float64)
        N.check(N.lib.psk_prec_chebyshev_info(self._h, None, None, None, N.ptr(c)), "psk_prec_chebyshev_info")
        return c

    def apply(self, vec):
        return self._device_apply(vec)


class FSAIPreconditioner(DeviceOperator, GenericPreconditioner):
    """M^-1 v = G^T (G v) with the factorized sparse approximate inverse G ~ L^-1 of a symmetric definite A
    (sign A = L L^T) on the pattern of tril(A^power) (psk_prec_create_fsai, pysolvers_amd/csrc/fsai.hip).

    No reference counterpart: the preconditioner that is formed by n independent small Cholesky factorisations on
    the device and applied as two SpMVs, with no triangular solve, no level schedule and no eigenvalue bound. sign
    M^-1 is symmetric positive definite by construction, so PCG and MINRES may use it. ``power=1`` takes A's own
    pattern, ``power=2`` the pattern of A A (the device SpGEMM); a pattern row may hold at most PSK_FSAI_ROW_CAP
    lower entries. A negative definite A (``sign`` = -1) is taken as Jacobi takes it.
    """

    device_kind = N.PSK_PREC_FSAI

    def __init__(self, A, power=1):
        if power not in (1, 2):
            raise ValueError("FSAIPreconditioner: power must be 1 or 2")
        dA = as_device_matrix(A)
        pattern = matmat(dA, dA) if power == 2 else None     # read during the setup only
        h = ctypes.c_void_p()
        N.check(N.lib.psk_prec_create_fsai(dA.handle, None if pattern is None else pattern.handle, 0,
                                           ctypes.byref(h)), "psk_prec_create_fsai")
        self._h = h
        self.n = dA.n
        self.power = int(power)

    def _info(self):
        s, nnz, mr = N.I32(), N.I64(), N.I32()
        N.check(N.lib.psk_prec_fsai_info(self._h, ctypes.byref(s), ctypes.byref(nnz), ctypes.byref(mr)),
                "psk_prec_fsai_info")
        return s.value, nnz.value, mr.value

    @property
    def sign(self):
        """+1 / -1: the sign of A (of row 0's diagonal entry)."""
        return self._info()[0]

    @property
    def nnz(self):
        """Stored entries of G."""
        return self._info()[1]

    @property
    def max_row(self):
        """Longest row of G: the size of the largest dense problem of the setup."""
        return self._info()[2]

    def apply(self, vec):
        return self._device_apply(vec)


class MulticolorGSPreconditioner(DeviceOperator, GenericPreconditioner):
    """M^-1 v = ``sweeps`` Gauss-Seidel sweeps for A z = v from z = 0 in a colour ordering of the rows
    (psk_prec_create_mcgs, pysolvers_amd/csrc/mcgs.hip; the colouring is psk_color_plan's, first-fit greedy on the
    structure of A + A^T).

    No reference counterpart (the reference's Gauss-Seidel is spsolve(triu(A), .), ClassicSmoothers.py:28-36): rows of
    one colour do not reference each other, so a colour updates in one streaming launch, with no dependency level,
    no spin wait and no grid sum; a sweep reads A once. ``symmetric=True`` runs the colours forward then backward
    (symmetric Gauss-Seidel, 2C-1 launches per sweep): the operator is then symmetric positive definite for an SPD A,
    so PCG and MINRES may use it. ``symmetric=False`` is the forward sweep alone (GMRES, BiCGStab, AMG smoothing). A
    matrix that needs more than PSK_MCGS_MAX_COLORS colours, or has a zero, missing or non-finite diagonal entry,
    raises PskError. The arithmetic is stated to the bit in include/psk.h.
    """

    device_kind = N.PSK_PREC_MCGS

    def __init__(self, A, sweeps=1, symmetric=True):
        dA = as_device_matrix(A)             # read during the setup only: the handle owns a grouped copy
        h = ctypes.c_void_p()
        flags = N.PSK_MCGS_SYMMETRIC if symmetric else 0
        N.check(N.lib.psk_prec_create_mcgs(dA.handle, int(sweeps), flags, ctypes.byref(h)), "psk_prec_create_mcgs")
        self._h = h
        self.n = dA.n
        self.sweeps = int(sweeps)
        self.symmetric = bool(symmetric)

    @property
    def ncolors(self):
        """Colours of the ordering (2 on the 5-point stencil)."""
        c = N.I32()
        N.check(N.lib.psk_prec_mcgs_info(self._h, ctypes.byref(c), None, None, None), "psk_prec_mcgs_info")
        return c.value

    @property
    def color_rows(self):
        """Rows of each colour: ``ncolors`` counts (int64)."""
        rows = np.zeros(N.PSK_MCGS_MAX_COLORS, dtype=np.int64)
        c = N.I32()
        N.check(N.lib.psk_prec_mcgs_info(self._h, ctypes.byref(c), None, None, N.ptr(rows)), "psk_prec_mcgs_info")
        return rows[:c.value].copy()

    def apply(self, vec):
        return self._device_apply(vec)
