"""CPU tests of the Chebyshev polynomial preconditioner: the oracle's own properties, the ABI, the smoother types.

Bars (written here, not inferred):
* the operator B of tests/cheby_oracle.py on FD 8^2 and on -FD 8^2, degrees 1..4: B symmetric to 1e-14 relative
  (it is a polynomial in D^-1 A times D^-1 with D = d I here; only roundings break the symmetry, a few 1e-16),
  B definite with the sign of A (the Gershgorin bound is a true upper bound of the spectrum of D^-1 A, so the
  polynomial has no root in it), spectral radius of I - B A below 1.
  FDLaplacian2D itself is NEGATIVE definite (diagonal -4/h^2), so "sign" below is the factor in A = sign * FD and
  the definite matrix is -sign * B: positive definite exactly when A is.
* PCG with the oracle operator on FD 32^2, b = ones, tau = 1e-8: degree 1 (Jacobi times a scalar) takes Jacobi's
  iteration count, and the counts fall strictly from degree 2 on.
"""
import ctypes

import numpy as np
import pytest

import cheby_oracle
from oracle import fdlap, krylov

from pysolvers_amd.Linear import AMGPreconditioner, Chebyshev, ChebyshevPreconditioner, ChebyshevSmoother


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_oracle_operator_is_symmetric_definite_and_contracts(sign, degree):
    A = (sign * fdlap.fd_laplacian_2d(-1.0, 1.0, 8)).tocsr()
    op = cheby_oracle.Chebyshev(A, degree=degree)
    assert op.lmax <= 2.0 + 1e-14 and op.lmax > 1.0          # Gershgorin of D^-1 A for the 5-point stencil
    B = op.matrix()
    asym = np.linalg.norm(B - B.T) / np.linalg.norm(B)
    ev = np.linalg.eigvalsh(0.5 * (B + B.T))
    a_sign = np.sign(np.linalg.eigvalsh(A.toarray()))
    assert np.all(a_sign == a_sign[0]) and a_sign[0] == -sign
    rad = np.max(np.abs(np.linalg.eigvals(np.eye(A.shape[0]) - B @ A.toarray())))
    print("sign %+d degree %d: lmax %.6f asym %.2e eig(B) [%.3e, %.3e] rho(I-BA) %.6f"
          % (sign, degree, op.lmax, asym, ev.min(), ev.max(), rad))
    assert asym <= 1e-14
    assert np.all(a_sign[0] * ev > 0.0)
    assert rad < 1.0


def test_oracle_pcg_iterations_fall_with_the_degree():
    A = fdlap.fd_laplacian_2d(-1.0, 1.0, 32).tocsr()
    b = np.ones(A.shape[0])
    jac = krylov.pcg(A, b, maxiter=500, tau=1e-8, precond=krylov.jacobi_form(A))
    its = []
    for degree in (1, 2, 3, 4):
        st = krylov.pcg(A, b, maxiter=500, tau=1e-8, precond=cheby_oracle.Chebyshev(A, degree=degree))
        assert st["success"]
        its.append(st["iters"])
    print("PCG FD 32^2: Jacobi %d, Chebyshev degrees 1..4 %s" % (jac["iters"], its))
    assert jac["success"] and its[0] == jac["iters"]
    assert its[1] < its[0] and its[2] < its[1] and its[3] < its[2]


def test_oracle_scalars():
    """Degree 1 is c0 = 1/theta alone; the caller's lmax is taken as it is; the coefficient count is 2*degree-1."""
    lmin, c = cheby_oracle.scalars(2.0, 30.0, 1)
    assert lmin == 2.0 / 30.0 and c.shape == (1,) and c[0] == 1.0 / ((2.0 + 2.0 / 30.0) / 2.0)
    for degree in (2, 5):
        assert cheby_oracle.scalars(1.7, 10.0, degree)[1].shape == (2 * degree - 1,)
    A = fdlap.fd_laplacian_2d(-1.0, 1.0, 4).tocsr()
    assert cheby_oracle.Chebyshev(A, degree=2, lmax=1.25).lmax == 1.25


def test_abi_exports_and_binds_the_new_symbols():
    from pysolvers_amd import _native as N
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ("psk_prec_create_chebyshev", "psk_prec_chebyshev_info"):
        assert hasattr(lib, name) and name in N.SIGNATURES
        assert getattr(N.lib, name).argtypes == N.SIGNATURES[name][1]
    assert N.PSK_PREC_CHEBYSHEV == 5 and N.lib.psk_abi_version() == 4
    assert ChebyshevPreconditioner.device_kind == N.PSK_PREC_CHEBYSHEV
    # argument errors are reported before any device work
    h = ctypes.c_void_p()
    assert N.lib.psk_prec_create_chebyshev(None, 2, 0.0, 30.0, ctypes.byref(h)) == N.PSK_ERR_ARG
    assert N.lib.psk_prec_chebyshev_info(None, None, None, None, None) == N.PSK_ERR_ARG


def test_factory_and_smoother_classes():
    t = Chebyshev()
    assert (t.degree, t.lmax, t.ratio) == (3, None, 30.0)
    t = Chebyshev(degree=5, lmax=1.9, ratio=10.0)
    assert (t.degree, t.lmax, t.ratio) == (5, 1.9, 10.0)
    assert (ChebyshevSmoother.degree, ChebyshevSmoother.ratio, ChebyshevSmoother.lmax) == (2, 30.0, None)
    S = ChebyshevSmoother.of(degree=3, ratio=20.0)
    assert issubclass(S, ChebyshevSmoother) and S is not ChebyshevSmoother
    assert (S.degree, S.ratio, S.lmax) == (3, 20.0, None)
    assert (ChebyshevSmoother.degree, ChebyshevSmoother.ratio) == (2, 30.0)    # the class itself is untouched


@pytest.mark.parametrize("bad", ["gs", object, int, None, cheby_oracle.Chebyshev])
def test_amg_still_refuses_what_is_not_a_smoother(bad):
    """The type check comes first: no hierarchy is built and no device is touched."""
    A = -fdlap.fd_laplacian_2d(-1.0, 1.0, 4)
    with pytest.raises(TypeError):
        AMGPreconditioner(A, smoother=bad)


def test_amg_refuses_the_abstract_smoother_base():
    from pysolvers_amd.Linear.ClassicSmoothers import _Smoother
    with pytest.raises(TypeError):
        AMGPreconditioner(-fdlap.fd_laplacian_2d(-1.0, 1.0, 4), smoother=_Smoother)
