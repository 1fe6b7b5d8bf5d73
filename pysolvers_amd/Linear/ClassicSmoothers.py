"""Relaxation smoothers of the AMG V-cycle (ClassicSmoothers.py:1-36), on the GPU.

Both of the reference's smoothers are a sweep x <- x + S^-1 (f - A x):
* JacobiSmoother      S^-1 r = DInv * r, DInv = reciprocal(diag A)      (:5-14)
* GaussSeidelSmoother S^-1 r = spsolve(triu(A), r)                      (:28-36)
* ChebyshevSmoother   S^-1 r = p(D^-1 A) D^-1 r, p the Chebyshev polynomial of a degree (no reference counterpart)
* MulticolorGaussSeidelSmoother S^-1 r = Gauss-Seidel sweeps from 0 in a colour ordering (no reference counterpart)
Each class builds that S^-1 as a device operator (``.operator``); the V-cycle itself runs inside
libpsk (psk_prec_create_amg). ``apply(f, x, nu)`` keeps the reference's host-callable contract.
"""
import numpy as np
import scipy.sparse as sp

from .DeviceMatrix import DeviceCSR, spmv
from .Preconditioner import ChebyshevPreconditioner, JacobiPreconditioner, MulticolorGSPreconditioner
from .TriangularSolve import TriangularSolveChain


def _host(A):
    return A.to_scipy() if isinstance(A, DeviceCSR) else sp.csr_matrix(A)


class _Smoother:
    def __init__(self, A, device_A=None):
        self.A = A
        self._dA = device_A if device_A is not None else (A if isinstance(A, DeviceCSR) else DeviceCSR.from_scipy(A))

    def apply(self, f, x, nu):
        """nu sweeps from x (host arrays): r = f - A*x; x = x + S^-1 r."""
        x = np.asarray(x, dtype=np.float64)
        for _ in range(nu):
            r = np.asarray(f, dtype=np.float64) - spmv(self._dA, x)
            x = x + self.operator.apply(r)
        return x


class JacobiSmoother(_Smoother):
    def __init__(self, A, device_A=None):
        super().__init__(A, device_A)
        self.operator = JacobiPreconditioner(self._dA)


class GaussSeidelSmoother(_Smoother):
    def __init__(self, A, device_A=None):
        super().__init__(A, device_A)
        self.U = sp.triu(_host(A)).tocsr()              # :33
        self.operator = TriangularSolveChain(self.U.shape[0], U=self.U, u_unit=False)


class ChebyshevSmoother(_Smoother):
    """S^-1 r = the Chebyshev polynomial of ``degree`` in D^-1 A applied to D^-1 r (ChebyshevPreconditioner on the
    level's device matrix). No reference counterpart: a smoother without a triangular solve. The class itself
    means degree 2, ratio 30 and the Gershgorin bound; ``ChebyshevSmoother.of(...)`` gives a configured subclass
    (``smoother=`` takes a class)."""

    degree, ratio, lmax = 2, 30.0, None

    def __init__(self, A, device_A=None):
        super().__init__(A, device_A)
        self.operator = ChebyshevPreconditioner(self._dA, degree=self.degree, lmax=self.lmax, ratio=self.ratio)

    @classmethod
    def of(cls, degree=2, ratio=30.0, lmax=None):
        """A subclass with these settings. One lmax serves every level: leave it None (each level's own
        Gershgorin bound) unless the levels share a bound."""
        name = "ChebyshevSmoother_d%d" % int(degree)
        return type(name, (cls,), dict(degree=int(degree), ratio=float(ratio), lmax=lmax))


class MulticolorGaussSeidelSmoother(_Smoother):
    """S^-1 r = Gauss-Seidel sweeps for A z = r from z = 0 in a colour ordering (MulticolorGSPreconditioner on the
    level's device matrix), so the smoother sweep x <- x + S^-1 (f - A x) with one sweep is a Gauss-Seidel sweep from
    x in the colour order: one streaming launch per colour instead of the triangular solve of GaussSeidelSmoother.
    No reference counterpart. The class itself means one symmetric sweep; ``MulticolorGaussSeidelSmoother.of(...)``
    gives a configured subclass (``smoother=`` takes a class)."""

    sweeps, symmetric = 1, True

    def __init__(self, A, device_A=None):
        super().__init__(A, device_A)
        self.operator = MulticolorGSPreconditioner(self._dA, sweeps=self.sweeps, symmetric=self.symmetric)

    @classmethod
    def of(cls, sweeps=1, symmetric=True):
        """A subclass with these settings."""
        name = "MulticolorGaussSeidelSmoother_s%d%s" % (int(sweeps), "" if symmetric else "_fwd")
        return type(name, (cls,), dict(sweeps=int(sweeps), symmetric=bool(symmetric)))
