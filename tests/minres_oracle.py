"""CPU restatement of preconditioned MINRES (TEST INFRASTRUCTURE).

The recurrence include/psk.h states for psk_minres — Paige-Saunders MINRES in the operation order of
scipy.sparse.linalg.minres, SPD preconditioner M, x0 = 0, no shift — in numpy float64 with one rounding per
elementwise operation and the row sums through the oracle's csr_matvec. The method has no reference counterpart, so
this file is the definition the device code is pinned to (tests/test_minres_cpu.py pins it to scipy's own
iterates). Only the dot products differ on the device (gridsum order), so the dot is pluggable and `spread` measures
what the summation order alone does to a history; parity with the device is asserted only over the prefix on which
three CPU summation orders agree.

    r1 = b; z = M(r1); beta1^2 = r1.z (< 0, or == 0 with b != 0: refused; b.b == 0: x = 0)
    normB = sqrt(b.b) (or norm_b > 0); scale = normB / beta1
    oldb = 0; beta = beta1; dbar = epsln = 0; phibar = beta1; cs = -1; sn = 0; w = w2 = 0; r2 = r1
    k:  s = 1/beta; v = s z
        y = A v;  k >= 1: y = y - (beta/oldb) r1
        alfa = v.y;  y = y - (alfa/beta) r2;  r1 = r2;  r2 = y;  z = M(r2)
        oldb = beta;  beta^2 = r2.z (< 0: refused);  beta = sqrt(.)
        oldeps = epsln; delta = cs dbar + sn alfa; gbar = sn dbar - cs alfa; epsln = sn beta; dbar = -cs beta
        gamma = sqrt(gbar^2 + beta^2) (== 0: breakdown)
        cs = gbar/gamma; sn = beta/gamma; phi = cs phibar; phibar = sn phibar
        w1 = w2; w2 = w; w = (v - oldeps w1 - delta w2) (1/gamma);  x = x + phi w
        hist[k] = scale phibar;  hist[k] <= tau normB or (k == maxiter-1 and not fail_on_maxiter): converged at k
"""
import math

import numpy as np

from oracle import krylov

CHUNK = 512
SPREAD_CAP = 2e-11     # of ||b||: the three dot orders "agree" on a history entry within this

MSG_NOT_PD = "preconditioner not positive definite"
MSG_GAMMA = "breakdown gamma==0"


def dot_numpy(a, b):
    return float(np.dot(a, b))


def dot_fsum(a, b):
    return math.fsum(a * b)


def dot_chunked(a, b):
    """512-element chunk sums added in order."""
    s = 0.0
    for i in range(0, len(a), CHUNK):
        s = s + float(np.sum(a[i:i + CHUNK] * b[i:i + CHUNK]))
    return s


DOTS = (dot_numpy, dot_fsum, dot_chunked)


def identity(v):
    return v


def minres(A, b, M=identity, maxiter=100, tau=1.0e-8, fail_on_maxiter=True, dot=dot_numpy, norm_b=0.0, on_iter=None):
    """dict(status, success, iters, exit, hist, soln, resid, norm_b, msg) in the conventions of psk_result as the
    Python layer reports them: converged at k -> iters = k + 1; breakdown at k -> iters = k; maxiter -> iters =
    maxiter - 1. resid: the true ||b - A x||_2 on a tolerance exit, else the last history entry; on a tolerance
    exit under the identity (M is `identity`) a true residual above tau normB is a failure, under a preconditioner
    it is not (the test was made in the M^-1 norm). on_iter(k, x) sees every iterate."""
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    x = np.zeros(n)
    r1 = b
    z = M(r1)
    bz = dot(r1, z)
    bb = dot(b, b)
    normB = float(norm_b) if norm_b > 0 else math.sqrt(bb)
    out = dict(status="converged", success=True, iters=1, exit="none", hist=np.zeros(0), soln=x, resid=0.0,
               norm_b=normB, msg=None)
    hist = []

    def done(**kw):
        out.update(kw)
        out["hist"] = np.array(hist, dtype=np.float64)
        return out

    def breakdown(k, msg):
        return done(status="breakdown", success=False, iters=k, exit="breakdown", soln=None, resid=float("nan"),
                    msg=msg)

    if bb == 0.0:
        return out
    if bz <= 0.0:
        return breakdown(0, MSG_NOT_PD)
    beta1 = math.sqrt(bz)
    thresh = tau * normB
    scale = normB / beta1
    oldb, beta, dbar, epsln, phibar, cs, sn = 0.0, beta1, 0.0, 0.0, beta1, -1.0, 0.0
    w = np.zeros(n)
    w2 = np.zeros(n)
    r2 = r1
    for k in range(maxiter):
        s = 1.0 / beta
        v = s * z
        y = krylov.mvmult(A, v)
        if k >= 1:
            y = y - (beta / oldb) * r1
        alfa = dot(v, y)
        y = y - (alfa / beta) * r2
        r1 = r2
        r2 = y
        z = M(r2)
        oldb = beta
        b2 = dot(r2, z)
        if b2 < 0.0:
            return breakdown(k, MSG_NOT_PD)
        beta = math.sqrt(b2)
        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = -cs * beta
        gamma = math.sqrt(gbar * gbar + beta * beta)
        if gamma == 0.0:
            return breakdown(k, MSG_GAMMA)
        cs = gbar / gamma
        sn = beta / gamma
        phi = cs * phibar
        phibar = sn * phibar
        denom = 1.0 / gamma
        w1 = w2
        w2 = w
        w = ((v - oldeps * w1) - delta * w2) * denom
        x = x + phi * w
        h = scale * phibar
        hist.append(h)
        if on_iter is not None:
            on_iter(k, x)
        if h <= thresh:
            tr = float(np.linalg.norm(b - krylov.mvmult(A, x)))
            ok = tr <= thresh or M is not identity
            return done(status="converged" if ok else "true residual above tolerance", success=ok, iters=k + 1,
                        exit="tolerance", soln=x, resid=tr)
        if k == maxiter - 1 and not fail_on_maxiter:
            return done(iters=k + 1, exit="maxiter", soln=x, resid=h)
    return done(status="maxiter", success=False, iters=max(maxiter - 1, 0), exit="maxiter", soln=x,
                resid=hist[-1] if hist else normB, msg="failure to converge")


def spread(A, b, M=identity, tau=1.0e-10, maxiter=1000):
    """The oracle under the three dot orders: (results, prefix). prefix = the longest k such that the three
    histories all have entries 0..k-1 and differ there, pairwise, by at most SPREAD_CAP ||b||."""
    res = [minres(A, b, M=M, maxiter=maxiter, tau=tau, dot=d) for d in DOTS]
    nb = float(np.linalg.norm(b))
    hs = [r["hist"] for r in res]
    m = min(len(h) for h in hs)
    prefix = 0
    for k in range(m):
        vals = [h[k] for h in hs]
        if max(vals) - min(vals) > SPREAD_CAP * nb:
            break
        prefix = k + 1
    return res, prefix


def counts_comparable(res, tau):
    """Equal iteration counts may be asserted: the three CPU runs agree, and no history entry of any of them
    lies within a relative 1e-6 of tau ||b||."""
    if len({r["iters"] for r in res}) != 1 or len({r["status"] for r in res}) != 1:
        return False
    for r in res:
        th = tau * r["norm_b"]
        if np.any(np.abs(r["hist"] - th) <= 1e-6 * th):
            return False
    return True


# ---- matrices ----------------------------------------------------------------------------------------------------

def laplacian_2d(m):
    """L = kron(I, T) + kron(T, I), T = tridiag(-1, 2, -1), unscaled, CSR with sorted rows."""
    import scipy.sparse as sp
    I = sp.identity(m, format="csr")
    T = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], [-1, 0, 1], format="csr")
    L = (sp.kron(I, T) + sp.kron(T, I)).tocsr()
    L.sort_indices()
    return L


def widest_gap_shift(m):
    """sigma: the midpoint of the widest of the 12 gaps between consecutive distinct eigenvalues of laplacian_2d(m)
    (eigvalsh, rounded to 9 places; the 2-D operator repeats most of them) starting at the first one >= 1.0."""
    ev = np.unique(np.round(np.linalg.eigvalsh(laplacian_2d(m).toarray()), 9))
    i0 = int(np.searchsorted(ev, 1.0, side="left"))
    gaps = ev[i0 + 1:i0 + 13] - ev[i0:i0 + 12]
    j = int(np.argmax(gaps))
    return float(0.5 * (ev[i0 + j] + ev[i0 + j + 1]))


def shifted_fd(m, scaled, sigma=None):
    """(A, b): A = L - sigma I (symmetric indefinite), sigma = widest_gap_shift(m) unless given. scaled: A is
    replaced by S A S with S = diag(uniform(0.5, 2)) from default_rng(m), drawn before b: still symmetric and
    indefinite, with a varying diagonal (positive for sigma < 4), so Jacobi is SPD and not a multiple of I."""
    import scipy.sparse as sp
    n = m * m
    if sigma is None:
        sigma = widest_gap_shift(m)
    A = (laplacian_2d(m) - sigma * sp.identity(n, format="csr")).tocsr()
    rng = np.random.default_rng(m)
    if scaled:
        S = sp.diags(rng.uniform(0.5, 2.0, size=n))
        A = (S @ A @ S).tocsr()
    A.sort_indices()
    b = rng.standard_normal(n)
    return A, b


def rand_sym_indef(n, seed):
    """(A, b): B + B^T with about 6 entries per row, plus a diagonal of alternating sign and magnitude
    (off-diagonal row sum + 1): symmetric, indefinite, strictly diagonally dominant; rows left unsorted
    (columns shuffled inside every row)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), 3)
    cols = rng.integers(0, n, size=rows.shape[0])
    keep = rows != cols
    B = sp.coo_matrix((rng.standard_normal(int(keep.sum())), (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    S = (B + B.T).tocsr()
    off = np.asarray(abs(S).sum(axis=1)).ravel()
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    A = (S + sp.diags(sign * (off + 1.0))).tocsr()
    A.sort_indices()
    ip, ix, dt = A.indptr, A.indices.copy(), A.data.copy()
    for i in range(n):
        p = rng.permutation(ip[i + 1] - ip[i])
        ix[ip[i]:ip[i + 1]] = ix[ip[i]:ip[i + 1]][p]
        dt[ip[i]:ip[i + 1]] = dt[ip[i]:ip[i + 1]][p]
    A = sp.csr_matrix((dt, ix, ip), shape=(n, n))
    A.has_sorted_indices = False
    b = rng.standard_normal(n)
    return A, b
