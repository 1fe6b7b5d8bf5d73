"""Preconditioner factories (PreconditionerType.py:4-19): ``form(A)`` builds the operator."""
from abc import ABC, abstractmethod

from .Preconditioner import (ChebyshevPreconditioner, FSAIPreconditioner, IdentityPreconditioner,
                             JacobiPreconditioner, MulticolorGSPreconditioner)


class PreconditionerType(ABC):
    @abstractmethod
    def form(self, A):
        ...


class IdentityPreconditionerType(PreconditionerType):
    """PreconditionerType.py:13-19."""

    def form(self, A):
        return IdentityPreconditioner()


class JacobiPreconditionerType(PreconditionerType):
    """Point-Jacobi (DInv = 1/diag(A)), the preconditioner of benchmark config 2."""

    def form(self, A):
        return JacobiPreconditioner(A)


# short factory name in the style of RightILUT()/RightIC()/AMG()
Jacobi = JacobiPreconditionerType


class ChebyshevPreconditionerType(PreconditionerType):
    """Chebyshev polynomial preconditioner of ``degree`` in D^-1 A (ChebyshevPreconditioner); ``lmax=None``:
    the Gershgorin bound."""

    def __init__(self, degree=3, lmax=None, ratio=30.0):
        self.degree = degree
        self.lmax = lmax
        self.ratio = ratio

    def form(self, A):
        return ChebyshevPreconditioner(A, degree=self.degree, lmax=self.lmax, ratio=self.ratio)


Chebyshev = ChebyshevPreconditionerType


class FSAIPreconditionerType(PreconditionerType):
    """Factorized sparse approximate inverse on the pattern of tril(A^power) (FSAIPreconditioner), power 1 or 2."""

    def __init__(self, power=1):
        self.power = power

    def form(self, A):
        return FSAIPreconditioner(A, power=self.power)


FSAI = FSAIPreconditionerType


class MulticolorGSPreconditionerType(PreconditionerType):
    """Gauss-Seidel sweeps in a colour ordering (MulticolorGSPreconditioner); ``symmetric=True`` for PCG / MINRES."""

    def __init__(self, sweeps=1, symmetric=True):
        self.sweeps = sweeps
        self.symmetric = symmetric

    def form(self, A):
        return MulticolorGSPreconditioner(A, sweeps=self.sweeps, symmetric=self.symmetric)


MulticolorGS = MulticolorGSPreconditionerType
