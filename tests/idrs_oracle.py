"""CPU restatement of right-preconditioned IDR(s) (TEST INFRASTRUCTURE).

The recurrence include/psk.h states for psk_idrs, in numpy float64 with one rounding per elementwise operation, the
row sums through the oracle's csr_matvec and the small triangular solves as scalar loops. The method has no reference
counterpart, so this file is the definition the device code is pinned to: the same operations in the same order. Only
the dot products differ (the device sums in its gridsum order), so the dot is pluggable, one of
bicgstab_oracle.DOTS, and `spread` measures what the summation order alone does to a history. One STEP is one SpMV:
hist has one entry per step, and iters and maxiter count steps.

    P[i][j] = double(splitmix64(i*s + j) >> 11) * 2^-52 - 1.0          (shadow(n, s); exact, never random at run time)
    x = 0; r = b; normB = sqrt(b.b) (or norm_b > 0); thr = tau normB; G = U = 0 (n x s); Mm = I_s; om = 1; j = 0
    cycle:
      f_i = p_i.r, i = 0..s-1
      for k = 0..s-1:
        c_i, i = k..s-1:  t = f_i;  t = t - Mm[i][l] c_l, l = k..i-1;  c_i = t / Mm[i][i]
        v = r;  v = v - c_i g_i, i = k..s-1;  v = M^-1 v;  u = om v;  u = u + c_i u_i, i = k..s-1
        g = A u                                                           (step j's SpMV)
        q_i = p_i.g, i = 0..s-1
        a_i, i = 0..k-1:  t = q_i;  t = t - Mm[i][l] a_l, l = 0..i-1;  a_i = t / Mm[i][i]
        g = g - a_i g_i, u = u - a_i u_i, i = 0..k-1;  g_k = g;  u_k = u
        Mm[i][k], i = k..s-1:  t = q_i;  t = t - Mm[i][l] a_l, l = 0..k-1;  Mm[i][k] = t
        Mm[k][k] == 0: breakdown
        beta = f_k / Mm[k][k];  r = r - beta g;  x = x + beta u;  hist[j] = sqrt(r.r);  stop test;  j++
        f_i = f_i - beta Mm[i][k], i = k+1..s-1
      v = M^-1 r;  t = A v                                                (step j's SpMV)
      tt = t.t;  ts = t.r;  rr = the r.r of the previous step;  tt == 0 or ts == 0: breakdown
      rho = ts / (sqrt(tt) sqrt(rr));  om = ts / tt;  |rho| < 0.7: om = (om 0.7) / |rho|
      x = x + om v;  r = r - om t;  hist[j] = sqrt(r.r);  stop test;  j++
    stop test: hist[j] <= thr, or j == maxiter-1 and not fail_on_maxiter
"""
import functools
import math

import numpy as np

import bicgstab_oracle as bo
from oracle import krylov

MAX_S = 8
_M64 = (1 << 64) - 1


def splitmix64(t):
    z = (t + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


@functools.lru_cache(maxsize=8)
def shadow(n, s):
    """The n x s shadow space P (read-only, cached): every entry in [-1, 1), exact in float64."""
    P = np.empty((n, s))
    for i in range(n):
        for j in range(s):
            P[i, j] = float(splitmix64(i * s + j) >> 11) * 2.0 ** -52 - 1.0
    P.setflags(write=False)
    return P


def idrs(A, b, s=4, M=bo.identity, maxiter=100, tau=1.0e-8, fail_on_maxiter=True, dot=bo.dot_numpy, norm_b=0.0):
    """dict(status, success, iters, exit, hist, soln, resid, norm_b, msg, s) in the conventions of psk_result as the
    Python layer reports them: stopped at step j -> iters = j + 1; breakdown at step j -> iters = j; maxiter ->
    iters = maxiter - 1. resid: the true ||b - A x|| on a tolerance exit, else the last recursive one."""
    if not 1 <= s <= MAX_S:
        raise ValueError("s must be 1..%d" % MAX_S)
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    x = np.zeros(n)
    bb = dot(b, b)
    normB = float(norm_b) if norm_b > 0 else math.sqrt(bb)
    out = dict(status="converged", success=True, iters=1, exit="none", hist=np.zeros(0), soln=x, resid=0.0,
               norm_b=normB, msg=None, s=s)
    if bb == 0.0:
        return out
    thr = tau * normB
    P = shadow(n, s)
    r = b.copy()
    G, U = np.zeros((n, s)), np.zeros((n, s))
    Mm = [[1.0 if i == l else 0.0 for l in range(s)] for i in range(s)]
    om = 1.0
    rr = bb
    hist = []

    def done(**kw):
        out.update(kw)
        out["hist"] = np.array(hist, dtype=np.float64)
        return out

    def breakdown(j, what):
        return done(status="breakdown", success=False, iters=j, exit="breakdown", soln=None, resid=float("nan"),
                    msg="breakdown " + what)

    def stop(j, x, nr):
        """The result when step j ends the solve, else None."""
        if nr <= thr:
            tr = float(np.linalg.norm(b - krylov.mvmult(A, x)))
            ok = tr <= thr
            return done(status="converged" if ok else "true residual above tolerance", success=ok, iters=j + 1,
                        exit="tolerance", soln=x, resid=tr)
        if j == maxiter - 1 and not fail_on_maxiter:
            return done(iters=j + 1, exit="maxiter", soln=x, resid=nr)
        return None

    def out_of_steps():
        return done(status="maxiter", success=False, iters=max(maxiter - 1, 0), exit="maxiter", soln=x,
                    resid=hist[-1] if hist else normB, msg="failure to converge")

    j = 0
    while True:
        if j >= maxiter:
            return out_of_steps()
        f = [dot(P[:, i], r) for i in range(s)]
        for k in range(s):
            if j >= maxiter:
                return out_of_steps()
            c = [0.0] * s
            for i in range(k, s):
                t = f[i]
                for l in range(k, i):
                    t = t - Mm[i][l] * c[l]
                c[i] = t / Mm[i][i]
            v = r
            for i in range(k, s):
                v = v - c[i] * G[:, i]
            v = M(v)
            u = om * v
            for i in range(k, s):
                u = u + c[i] * U[:, i]
            g = krylov.mvmult(A, u)
            q = [dot(P[:, i], g) for i in range(s)]
            a = [0.0] * s
            for i in range(k):
                t = q[i]
                for l in range(i):
                    t = t - Mm[i][l] * a[l]
                a[i] = t / Mm[i][i]
            for i in range(k):
                g = g - a[i] * G[:, i]
                u = u - a[i] * U[:, i]
            G[:, k] = g
            U[:, k] = u
            for i in range(k, s):
                t = q[i]
                for l in range(k):
                    t = t - Mm[i][l] * a[l]
                Mm[i][k] = t
            if Mm[k][k] == 0.0:
                return breakdown(j, "Mm[k][k]==0")
            beta = f[k] / Mm[k][k]
            r = r - beta * g
            x = x + beta * u
            rr = dot(r, r)
            nr = math.sqrt(rr)
            hist.append(nr)
            end = stop(j, x, nr)
            if end is not None:
                return end
            j += 1
            for i in range(k + 1, s):
                f[i] = f[i] - beta * Mm[i][k]
        if j >= maxiter:
            return out_of_steps()
        v = M(r)
        t = krylov.mvmult(A, v)
        tt = dot(t, t)
        ts = dot(t, r)
        if tt == 0.0:
            return breakdown(j, "dot(t,t)==0")
        if ts == 0.0:
            return breakdown(j, "dot(t,r)==0")
        rho = ts / (math.sqrt(tt) * math.sqrt(rr))
        om = ts / tt
        if abs(rho) < 0.7:
            om = (om * 0.7) / abs(rho)
        x = x + om * v
        r = r - om * t
        rr = dot(r, r)
        nr = math.sqrt(rr)
        hist.append(nr)
        end = stop(j, x, nr)
        if end is not None:
            return end
        j += 1


def spread(A, b, s=4, M=bo.identity, tau=1.0e-10, maxiter=1000):
    """The oracle under the three dot orders: (results, prefix), as bicgstab_oracle.spread: prefix = the longest k such
    that the three histories all have entries 0..k-1 and differ there, pairwise, by at most SPREAD_CAP ||b||."""
    res = [idrs(A, b, s=s, M=M, maxiter=maxiter, tau=tau, dot=d) for d in bo.DOTS]
    nb = float(np.linalg.norm(b))
    hs = [r["hist"] for r in res]
    m = min(len(h) for h in hs)
    prefix = 0
    for k in range(m):
        vals = [h[k] for h in hs]
        if max(vals) - min(vals) > bo.SPREAD_CAP * nb:
            break
        prefix = k + 1
    return res, prefix


counts_comparable = bo.counts_comparable


def breakdown_system():
    """A 2 x 2 system whose first step breaks down: A b = 0 exactly, so g = A u = 0, every q_i = 0 and Mm[0][0] = 0."""
    import scipy.sparse as sp
    return sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 1.0]])), np.array([1.0, 0.0])
