"""CPU restatement of the Chebyshev polynomial preconditioner / smoother (TEST INFRASTRUCTURE).

The operator include/psk.h states for psk_prec_create_chebyshev, in numpy float64 with one rounding per operation
and the row sums through the oracle's csr_matvec (oracle.krylov.mvmult = scipy's stored-order sums of rounded
products). It has no reference counterpart (the reference smooths with Jacobi and Gauss-Seidel), so this file is
the definition the device code is pinned to, bit for bit:

    dinv = 1/diag(A);  lmax given, or the Gershgorin bound max_i (sum_j |a_ij|) |dinv_i| of D^-1 A
    lmin = lmax/ratio, theta = (lmax+lmin)/2, delta = (lmax-lmin)/2, sigma = theta/delta, rho_0 = 1/sigma,
    c0 = 1/theta; k = 1..degree-1: rho_k = 1/(2 sigma - rho_{k-1}), alpha_k = rho_k rho_{k-1}, beta_k = 2 rho_k/delta
    z = M^-1 v:  d = c0 (dinv v), z = d;  k = 1..degree-1: d = alpha_k d + beta_k (dinv (v - A z)), z = z + d

Also the few lines of the V-cycle (VCycleManager.py:31-62) and of its two loops (AMGPreconditioner.py:46-51,
VCycleSolver.py:52-95) with S^-1 given as a callable per level: oracle.amg takes its smoother by name only.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import krylov


def gershgorin(A, dinv):
    """max_i (sum_j |a_ij|) |dinv_i|, the row sums in stored order from 0.0 (A itself is left as it is:
    abs(A) would sort it in place)."""
    absA = sp.csr_matrix((np.abs(A.data), np.copy(A.indices), np.copy(A.indptr)), shape=A.shape)
    absA.has_sorted_indices = False
    rows = krylov.mvmult(absA, np.ones(A.shape[0]))
    return float(np.max(rows * np.abs(dinv)))


def scalars(lmax, ratio, degree):
    """(lmin, coeffs) with coeffs = [c0, alpha_1, beta_1, ..., alpha_{degree-1}, beta_{degree-1}] in plain
    double arithmetic."""
    lmax, ratio = float(lmax), float(ratio)
    lmin = lmax / ratio
    theta = (lmax + lmin) / 2.0
    delta = (lmax - lmin) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    coeffs = [1.0 / theta]
    for _ in range(1, degree):
        rk = 1.0 / (2.0 * sigma - rho)
        coeffs += [rk * rho, 2.0 * rk / delta]
        rho = rk
    return lmin, np.array(coeffs, dtype=np.float64)


class Chebyshev:
    """The operator as a callable, with the product's introspection names (degree, lmax, lmin, coefficients)."""

    def __init__(self, A, degree=3, lmax=None, ratio=30.0):
        self.A = A
        self.degree = int(degree)
        self.dinv = np.reciprocal(A.diagonal())
        self.lmax = float(lmax) if lmax is not None and lmax > 0 else gershgorin(A, self.dinv)
        self.lmin, self.coefficients = scalars(self.lmax, ratio, self.degree)

    def __call__(self, v):
        v = np.asarray(v, dtype=np.float64)
        c = self.coefficients
        d = c[0] * (self.dinv * v)
        z = np.copy(d)
        for k in range(1, self.degree):
            res = v - krylov.mvmult(self.A, z)
            d = c[2 * k - 1] * d + c[2 * k] * (self.dinv * res)
            z = z + d
        return z

    def matrix(self):
        """The operator as a dense matrix (small A only)."""
        n = self.A.shape[0]
        return np.column_stack([self(e) for e in np.eye(n)])


# ---- the V-cycle with S^-1 as a callable per level ---------------------------------------------------------------

def smooth(A, S, f, x, nu):
    """nu sweeps x <- x + S^-1 (f - A x) (ClassicSmoothers.py:11-14 with any S^-1)."""
    for _ in range(nu):
        r = f - A * x
        x = x + S(r)
    return x


def vcycle(ops, P, R, S, f, x, lev, nu_pre=2, nu_post=2):
    """VCycleManager.runLevel (VCycleManager.py:31-62); S[lev] = that level's S^-1."""
    if lev == 0:
        return spla.spsolve(ops[0], f)
    x = smooth(ops[lev], S[lev], f, x, nu_pre)
    r2 = R[lev - 1] * (f - ops[lev] * x)
    x2 = vcycle(ops, P, R, S, r2, np.zeros_like(r2), lev - 1, nu_pre, nu_post)
    x = x + P[lev - 1] * x2
    return smooth(ops[lev], S[lev], f, x, nu_post)


def level_smoothers(ops, degree=2, ratio=30.0):
    """[None, Chebyshev(ops[1]), ...]: each level's own Gershgorin bound, as ChebyshevSmoother builds them."""
    return [None] + [Chebyshev(M, degree=degree, ratio=ratio) for M in ops[1:]]


def amg_apply(A, levels, S, b, num_iters=5, nu_pre=2, nu_post=2, tau=1e-8):
    """AMGPreconditioner.apply (AMGPreconditioner.py:46-51): num_iters cycles from x = copy(b), early exit."""
    ops, P, R = levels
    nb = np.linalg.norm(b)
    if nb == 0.0:
        return np.zeros_like(b)
    x = np.copy(b)
    for _ in range(num_iters):
        x = vcycle(ops, P, R, S, b, x, len(ops) - 1, nu_pre, nu_post)
        if np.linalg.norm(b - A * x) < tau * nb:
            return x
    return x


def vcycle_solve(A, levels, S, b, maxiter=100, tau=1e-8, nu_pre=2, nu_post=2):
    """AMGVCycleSolver.solve (VCycleSolver.py:52-95) for b != 0: dict(iters, converged, hist, soln)."""
    ops, P, R = levels
    nb = np.linalg.norm(b)
    x = np.copy(b)
    hist = []
    for k in range(maxiter):
        x = vcycle(ops, P, R, S, b, x, len(ops) - 1, nu_pre, nu_post)
        nr = np.linalg.norm(b - A * x)
        hist.append(float(nr))
        if nr < tau * nb:
            return dict(iters=k + 1, converged=True, hist=np.array(hist), soln=x)
    return dict(iters=maxiter - 1, converged=False, hist=np.array(hist), soln=x)
