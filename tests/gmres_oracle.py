"""CPU restatement of one GMRES Arnoldi cycle that keeps its internals, and the extended-precision measures the
Arnoldi tests apply to them (TEST INFRASTRUCTURE).

`cycle` is oracle/krylov.py:gmres_cycle statement for statement (the same temporaries, the same strided columns of
a C-ordered Q), except that the dot product is pluggable, as in tests/bicgstab_oracle.py: the device sums its dots
in its gridsum order, so the three CPU orders (np.dot, math.fsum, 512-element chunks) measure what the summation
order alone does. A norm is the square root of a dot (numpy's norm of a vector is sqrt(x.dot(x))), so with
dot_numpy every array is bit-identical to krylov.gmres / gmres_cycle (tests/test_gmres_oracle_cpu.py). It returns
what krylov.gmres_cycle discards: Q, the unrotated Hessenberg columns H, the rotated ones R, CS, g, y.

The measures are written once, in np.longdouble, and take plain arrays: the tests apply the same function to the
oracle's arrays and to the device's (psk_lab_gmres_internals).
"""
import math

import numpy as np
import numpy.linalg as npla

import bicgstab_oracle as bo
from oracle import krylov

LD = np.longdouble
EPS = 2.0 ** -53           # unit roundoff of float64


def gamma(m):
    """gamma_m = m eps / (1 - m eps): the bound on a dot of m terms in any order, with or without FMA
    (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 and 3.5)."""
    return LD(m) * LD(EPS) / (LD(1) - LD(m) * LD(EPS))


def cycle(A, r0, K, thresh, precond=krylov.identity_apply, dot=bo.dot_numpy):
    """At most K Arnoldi steps of GMRESSolver.py:87-158 from r0 (krylov.gmres_cycle). dict(k, conv, brk, hist, dx,
    y, Q, H, R, CS, g): k = the last step, H / R = the unrotated / rotated (K+1) x K Hessenberg matrix."""
    n = A.shape[0]
    Q = np.zeros([n, K + 1])                             # :77
    HBar = np.zeros([K + 1, K])                          # :80 (rotated in place, as the reference does)
    H = np.zeros([K + 1, K])                             # the columns before their rotations
    CS = np.zeros([K, 2])                                # :83
    beta = math.sqrt(dot(r0, r0))                        # :90
    Q[:, 0] = r0 / beta                                  # :91
    e1 = np.zeros(K + 1)                                 # :95
    e1[0] = 1.0
    g = beta * e1                                        # :97
    hist = []
    for k in range(K):                                   # :104
        u = krylov.mvmult(A, precond(Q[:, k]))           # :107
        for j in range(k + 1):                           # :110-112
            HBar[j, k] = dot(Q[:, j], u)
            u -= HBar[j, k] * Q[:, j]
        HBar[k + 1, k] = math.sqrt(dot(u, u))            # :115
        hLastColNorm = npla.norm(HBar[0:k + 1, k])       # :121
        brk = abs(HBar[k + 1, k]) <= 1.0e-16 * hLastColNorm   # :122
        if not brk:
            Q[:, k + 1] = u / HBar[k + 1, k]             # :125
        H[:, k] = HBar[:, k]
        for j in range(k):                               # :133-135
            krylov.apply_givens_in_place(HBar[:, k], CS[j, 0], CS[j, 1], j)
        CS[k, :] = krylov.find_givens_coefficients(HBar[:, k], k)         # :140
        krylov.apply_givens_in_place(HBar[:, k], CS[k, 0], CS[k, 1], k)   # :145
        krylov.apply_givens_in_place(g, CS[k, 0], CS[k, 1], k)            # :148
        norm_r_k = np.abs(g[k + 1])                      # :152
        hist.append(norm_r_k)
        if brk or norm_r_k <= thresh or k == K - 1:      # :158 (or the cycle's last step)
            y = npla.solve(HBar[0:k + 1, 0:k + 1], g[0:k + 1])   # :159
            dx = precond(np.dot(Q[:, 0:k + 1], y))       # :160
            return dict(k=k, conv=bool(brk or norm_r_k <= thresh), brk=bool(brk), hist=hist, dx=dx, y=y, Q=Q, H=H,
                        R=HBar, CS=CS, g=g)
    raise ValueError("cycle: K must be >= 1")


def solve(A, b, restart=0, maxiter=100, tau=1.0e-8, precond=krylov.identity_apply, dot=bo.dot_numpy):
    """GMRES (restart = 0: one cycle of maxiter steps) or GMRES(restart) as krylov.gmres_restarted runs its cycles.
    dict(iters, conv, hist, x, cycles): cycles = every cycle's dict, the last one being what the device's workspace
    holds after the same solve."""
    norm_b = math.sqrt(dot(b, b))
    thresh = tau * norm_b
    K = restart if 0 < restart < maxiter else maxiter
    it, r, x, hist, cycles = 0, b, None, [], []
    while True:
        c = cycle(A, r, min(maxiter - it, K), thresh, precond, dot)
        cycles.append(c)
        hist += c["hist"]
        x = c["dx"] if x is None else x + c["dx"]
        if c["conv"]:
            return dict(iters=it + c["k"] + 1, conv=True, hist=np.array(hist), x=x, cycles=cycles)
        it += min(maxiter - it, K)
        if it >= maxiter:
            return dict(iters=maxiter - 1, conv=False, hist=np.array(hist), x=x, cycles=cycles)
        r = b - krylov.mvmult(A, x)


# ---- extended-precision measures ------------------------------------------------------------------------------------

def matvec_ld(A, x):
    """A x with every product and every row sum in longdouble (CSR, any entry order)."""
    A = A.tocsr()
    prod = A.data.astype(LD) * np.asarray(x, dtype=LD)[A.indices]
    out = np.zeros(A.shape[0], dtype=LD)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    np.add.at(out, rows, prod)
    return out


def _u0(A, minv, Q, k):
    """A (M^-1 q_k): M^-1 the double-rounded operation the solver applies, the product in longdouble."""
    return matvec_ld(A, minv(np.ascontiguousarray(Q[:, k])))


def arnoldi_residuals(A, minv, Q, H, ncols):
    """rho_k = ||A M^-1 q_k - Q[:, :k+2] H[:k+2, k]|| / ||A M^-1 q_k|| for the ncols built columns. After a
    breakdown H[k+1, k] = 0 and q_{k+1} was never written: it takes no part."""
    Ql = np.asarray(Q, dtype=LD)
    Hl = np.asarray(H, dtype=LD)
    rho = np.zeros(ncols, dtype=LD)
    for k in range(ncols):
        u0 = _u0(A, minv, Q, k)
        m = k + 2 if H[k + 1, k] != 0.0 else k + 1
        d = u0 - Ql[:, :m] @ Hl[:m, k]
        rho[k] = np.sqrt(d @ d) / np.sqrt(u0 @ u0)
    return rho


def orthogonality(Q, m):
    """omega = max_ij |q_i.q_j - delta_ij| over the first m columns."""
    Ql = np.asarray(Q[:, :m], dtype=LD)
    G = Ql.T @ Ql
    return np.max(np.abs(G - np.eye(m, dtype=LD)))


def mgs_dot_errors(A, minv, Q, H, ncols):
    """Every MGS dot of the ncols built columns against its exact value, from the given Q and H:
    u_0 = A M^-1 q_k, u_{j+1} = u_j - h_jk q_j in longdouble. (worst_h, worst_norm): the largest
    |h_jk - q_j.u_j| / (gamma_{n+2} |q_j|^T|u_j|) and |h_{k+1,k}^2 - u.u| / (2 gamma_{n+2} u.u); each must be <= 1.
    A dot whose terms are all zero must be exactly zero (ratio inf otherwise)."""
    n = Q.shape[0]
    Ql = np.asarray(Q, dtype=LD)
    gm = gamma(n + 2)
    worst_h = worst_n = LD(0)

    def ratio(err, bound):
        if bound == 0:
            return LD(0) if err == 0 else LD(np.inf)
        return err / bound

    for k in range(ncols):
        u = _u0(A, minv, Q, k)
        for j in range(k + 1):
            h = LD(H[j, k])
            worst_h = max(worst_h, ratio(abs(h - Ql[:, j] @ u), gm * (np.abs(Ql[:, j]) @ np.abs(u))))
            u = u - h * Ql[:, j]
        uu = u @ u
        hk = LD(H[k + 1, k])
        worst_n = max(worst_n, ratio(abs(hk * hk - uu), 2 * gm * uu))
    return worst_h, worst_n


def givens_replay(H, beta, ncols):
    """The rotations of krylov.gmres_cycle (:133-148) on the given unrotated columns, column by column, in float64:
    (R, CS, g, hist) with hist[k] = |g[k+1]|; beta None: no g (a later cycle, whose beta is not in hand)."""
    K = H.shape[1]
    R = np.zeros_like(H)
    CS = np.zeros([K, 2])
    g = None
    if beta is not None:
        e1 = np.zeros(K + 1)
        e1[0] = 1.0
        g = beta * e1
    hist = []
    for k in range(ncols):
        col = np.array(H[:, k], dtype=np.float64)
        for j in range(k):
            krylov.apply_givens_in_place(col, CS[j, 0], CS[j, 1], j)
        CS[k, :] = krylov.find_givens_coefficients(col, k)
        krylov.apply_givens_in_place(col, CS[k, 0], CS[k, 1], k)
        R[:, k] = col
        if g is not None:
            krylov.apply_givens_in_place(g, CS[k, 0], CS[k, 1], k)
            hist.append(np.abs(g[k + 1]))
    return R, CS, g, np.array(hist)


def update_x_error(Q, y, x, m, dinv=None):
    """x = [DInv] (Q[:, :m] y): max_i |x_i - dinv_i sum_j Q_ij y_j| / (gamma_{m+1} |dinv_i| sum_j |Q_ij||y_j|),
    which must be <= 1 (m products accumulated in any order, with or without FMA, and the scaling)."""
    Ql = np.asarray(Q[:, :m], dtype=LD)
    yl = np.asarray(y[:m], dtype=LD)
    s = Ql @ yl
    bound = gamma(m + 1) * (np.abs(Ql) @ np.abs(yl))
    if dinv is not None:
        s = np.asarray(dinv, dtype=LD) * s
        bound = np.abs(np.asarray(dinv, dtype=LD)) * bound
    err = np.abs(np.asarray(x, dtype=LD) - s)
    assert np.all(err[bound == 0] == 0)
    nz = bound > 0
    return np.max(err[nz] / bound[nz]) if nz.any() else LD(0)


def triangular_error(R, y, g, m):
    """max_i |R[:m,:m] y - g[:m]|_i / (gamma_m |R||y|)_i, which must be <= 1: the componentwise backward error of
    the least-squares solve (an LU whose multipliers are the rotated columns' residual subdiagonals, then back
    substitution)."""
    Rl = np.asarray(R[:m, :m], dtype=LD)
    yl = np.asarray(y[:m], dtype=LD)
    err = np.abs(Rl @ yl - np.asarray(g[:m], dtype=LD))
    bound = gamma(m) * (np.abs(Rl) @ np.abs(yl))
    return np.max(err / bound)
