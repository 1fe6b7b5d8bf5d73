"""CPU restatement of right-preconditioned BiCGStab (TEST INFRASTRUCTURE).

The recurrence include/psk.h states for psk_bicgstab, in numpy float64 with one rounding per elementwise
operation and the row sums through the oracle's csr_matvec. The method has no reference counterpart, so this
file is the definition the device code is pinned to: the same operations in the same order. Only the dot
products differ (the device sums in its gridsum order), so the dot is pluggable and `spread` measures what the
summation order alone does to a history: BiCGStab amplifies rounding, and parity with the device is asserted
only over the prefix on which three CPU summation orders agree.

    r = b; rhat = b; p = b; normB = sqrt(b.b) (or norm_b > 0); rho = rhat.r;  b.b == 0: x = 0
    k:  ph = M^-1 p; v = A ph; rv = rhat.v (== 0: breakdown); alpha = rho / rv
        s = r - alpha v; ns = sqrt(s.s); ns <= tau normB: x = x + alpha ph, hist[k] = ns, converged at k
        sh = M^-1 s; t = A sh; ts = t.s; tt = t.t (== 0: breakdown); omega = ts / tt (== 0: breakdown)
        x = (x + alpha ph) + omega sh; r = s - omega t; nr = sqrt(r.r); hist[k] = nr
        nr <= tau normB or (k == maxiter-1 and not fail_on_maxiter): converged at k
        rho_new = rhat.r (== 0: breakdown); beta = (rho_new / rho) (alpha / omega); rho = rho_new
        p = r + beta (p - omega v)
"""
import math

import numpy as np

from oracle import krylov

CHUNK = 512
SPREAD_CAP = 2e-11     # of ||b||: the three dot orders "agree" on a history entry within this


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


def bicgstab(A, b, M=identity, maxiter=100, tau=1.0e-8, fail_on_maxiter=True, dot=dot_numpy, norm_b=0.0):
    """dict(status, success, iters, exit, half, hist, soln, resid, norm_b, msg) in the conventions of psk_result as
    the Python layer reports them: converged at k -> iters = k + 1; breakdown at k -> iters = k; maxiter ->
    iters = maxiter - 1. resid: the true ||b - A x|| on a tolerance exit, else the last recursive one. half: the
    tolerance exit was the half step's (||s||), which runs one SpMV of its iteration, not two."""
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    x = np.zeros(n)
    bb = dot(b, b)
    normB = float(norm_b) if norm_b > 0 else math.sqrt(bb)
    out = dict(status="converged", success=True, iters=1, exit="none", half=False, hist=np.zeros(0), soln=x,
               resid=0.0, norm_b=normB, msg=None)
    if bb == 0.0:
        return out
    thresh = tau * normB
    r, rhat, p = b, b, b
    rho = bb                                         # rhat.r with r = rhat = b
    hist = []

    def done(**kw):
        out.update(kw)
        out["hist"] = np.array(hist, dtype=np.float64)
        return out

    def breakdown(k, what):
        return done(status="breakdown", success=False, iters=k, exit="breakdown", soln=None, resid=float("nan"),
                    msg="breakdown " + what)

    def tolerance_exit(k, x, half=False):
        tr = float(np.linalg.norm(b - krylov.mvmult(A, x)))
        ok = tr <= thresh
        return done(status="converged" if ok else "true residual above tolerance", success=ok, iters=k + 1,
                    exit="tolerance", half=half, soln=x, resid=tr)

    for k in range(maxiter):
        ph = M(p)
        v = krylov.mvmult(A, ph)
        rv = dot(rhat, v)
        if rv == 0.0:
            return breakdown(k, "dot(rhat,v)==0")
        alpha = rho / rv
        s = r - alpha * v
        ns = math.sqrt(dot(s, s))
        if ns <= thresh:
            x = x + alpha * ph
            hist.append(ns)
            return tolerance_exit(k, x, half=True)
        sh = M(s)
        t = krylov.mvmult(A, sh)
        ts = dot(t, s)
        tt = dot(t, t)
        if tt == 0.0:
            return breakdown(k, "dot(t,t)==0")
        omega = ts / tt
        if omega == 0.0:
            return breakdown(k, "omega==0")
        x = (x + alpha * ph) + omega * sh
        r = s - omega * t
        nr = math.sqrt(dot(r, r))
        hist.append(nr)
        if nr <= thresh:
            return tolerance_exit(k, x)
        if k == maxiter - 1 and not fail_on_maxiter:
            return done(iters=k + 1, exit="maxiter", soln=x, resid=nr)
        rho_new = dot(rhat, r)
        if rho_new == 0.0:
            return breakdown(k, "dot(rhat,r)==0")
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        p = r + beta * (p - omega * v)
    return done(status="maxiter", success=False, iters=max(maxiter - 1, 0), exit="maxiter", soln=x,
                resid=hist[-1] if hist else normB, msg="failure to converge")


def spread(A, b, M=identity, tau=1.0e-10, maxiter=1000):
    """The oracle under the three dot orders: (results, prefix). prefix = the longest k such that the three
    histories all have entries 0..k-1 and differ there, pairwise, by at most SPREAD_CAP ||b||."""
    res = [bicgstab(A, b, M=M, maxiter=maxiter, tau=tau, dot=d) for d in DOTS]
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


LONG_ROW = 500        # the full row of random_nonsym


def random_nonsym(n=1100, seed=7):
    """Nonsymmetric, strictly row-diagonally dominant with a positive diagonal: 1 to about 20 entries per row (rows
    0..4 hold their diagonal alone), row LONG_ROW holding every column from 5 on (at n = 1100 its SpMV tile is more
    than one 1280-entry chunk), columns shuffled inside every row. tests/test_gpu_cheby.py's _random_spd without
    the symmetrisation."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    per = rng.integers(0, 16, size=n)
    per[:5] = 0
    rows = np.repeat(np.arange(n), per)
    cols = rng.integers(5, n, size=rows.shape[0])
    keep = rows != cols
    S = sp.coo_matrix((rng.standard_normal(keep.sum()), (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    full = sp.coo_matrix((rng.standard_normal(n - 5), (np.full(n - 5, LONG_ROW), np.arange(5, n))),
                         shape=(n, n)).tocsr()
    S = (S + full).tolil()
    S.setdiag(0.0)
    S = S.tocsr()
    S.eliminate_zeros()
    d = np.asarray(abs(S).sum(axis=1)).ravel() + 1.0 + rng.random(n)
    A = (S + sp.diags(d)).tocsr()
    A.sort_indices()
    ip, ix, dt = A.indptr, A.indices.copy(), A.data.copy()
    for i in range(n):
        p = rng.permutation(ip[i + 1] - ip[i])
        ix[ip[i]:ip[i + 1]] = ix[ip[i]:ip[i + 1]][p]
        dt[ip[i]:ip[i + 1]] = dt[ip[i]:ip[i + 1]][p]
    B = sp.csr_matrix((dt, ix, ip), shape=(n, n))
    B.has_sorted_indices = False
    return B


def cd_matrix(m, c):
    """cd m: the m x m five-point convection-diffusion operator kron(I, tridiag(-1-c, 2, -1+c)) +
    kron(tridiag(-1, 2, -1), I), CSR."""
    import scipy.sparse as sp
    I = sp.identity(m, format="csr")
    T1 = sp.diags([np.full(m - 1, -1.0 - c), np.full(m, 2.0), np.full(m - 1, -1.0 + c)], [-1, 0, 1], format="csr")
    T2 = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], [-1, 0, 1], format="csr")
    A = (sp.kron(I, T1) + sp.kron(T2, I)).tocsr()
    A.sort_indices()
    return A
