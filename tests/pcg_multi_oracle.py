"""CPU restatement of the multi-column PCG loop (TEST INFRASTRUCTURE): numpy + scipy, nothing from pysolvers_amd.

psk_pcg_multi (include/psk.h) runs several right-hand sides in one loop: iteration k is one pass over ALL columns, each
column an independent PCG with the recurrence of oracle.krylov.pcg (PCGSolver.py:97-138) and its own scalars, threshold,
history and exit; a column that has stopped is frozen and the loop ends when every column has stopped or at maxiter.
This file states exactly that, in lock step, so that freezing and the per-column result conventions are written down
once: column j of pcg_multi must equal oracle.krylov.pcg on column j alone, bit for bit, under the same dot function
(tests/test_pcg_multi_cpu.py). Only the dot products of the device differ (it sums in its gridsum order), so the dot is
pluggable, as in bicgstab_oracle: np.dot, math.fsum of the rounded products, or 512-element chunks added in order.

Also here: the inputs of tests/test_gpu_pcg_multi.py (matrices from tests/pcg_replay.py plus the "arrow" matrices and
the mixed-stopping columns), so that the CPU tests can show what those inputs do before the GPU tests rely on it.
"""
import math

import numpy as np
import scipy.sparse as sp

import pcg_replay as pr
from bicgstab_oracle import DOTS, dot_chunked, dot_fsum, dot_numpy  # noqa: F401  (re-exported: the three orders)

MULTI_MAX = 4          # PSK_PCG_MULTI_MAX
TILE = 256             # rows of a tile of the multi-column kernels (kMultiTile; the SpMM's tile_rows of these matrices)


def pcg_multi(A, B, dinv=None, maxiter=100, tau=1.0e-8, fail_on_maxiter=True, dot=dot_numpy):
    """B: (n, nrhs). dinv: None (identity) or the Jacobi DInv array. Returns a list of nrhs dicts in the conventions of
    oracle.krylov.pcg (success, iters, soln, resid, msg, hist) plus status ("converged" / "maxiter" / "breakdown"),
    exit ("none" / "tolerance" / "maxiter" / "breakdown"), norm_b and x (the column's iterate when it stopped: soln is
    None after a breakdown, as the reference reports it, but the device still holds x)."""
    B = np.asarray(B, dtype=np.float64)
    n, m = B.shape
    apply = (lambda v: v) if dinv is None else (lambda v: np.multiply(dinv, v))
    cols = []
    for j in range(m):
        b = np.ascontiguousarray(B[:, j])
        c = dict(b=b, hist=[], done=False, out=None, x=np.zeros_like(b))     # x = np.zeros_like(b)  :100
        c["normB"] = math.sqrt(dot(b, b))                                    # self.norm(b)  :86
        if c["normB"] == 0.0:                                                # :87-88
            _stop(c, status="converged", exit="none", success=True, iters=1, soln=c["x"], resid=0, msg=None)
        else:
            c["r"] = np.copy(b)                                              # :97
            c["p"] = apply(c["r"])                                           # :98
            c["u"] = np.copy(c["p"])                                         # :99
            c["udr"] = dot(c["u"], c["r"])                                   # :102
            if c["udr"] == 0.0:                                              # :104-105
                _stop(c, status="breakdown", exit="breakdown", success=False, iters=0, soln=None, resid=None,
                      msg="breakdown dot(u,r)==0")
        cols.append(c)
    for k in range(maxiter):
        if all(c["done"] for c in cols):                                     # the loop ends with its last column
            break
        for c in cols:
            if c["done"]:
                continue                                                     # frozen: nothing of it is touched
            Ap = A @ c["p"]                                                  # :111
            pTAp = dot(c["p"], Ap)                                           # :113
            if pTAp == 0.0:                                                  # :114-115
                _stop(c, status="breakdown", exit="breakdown", success=False, iters=k, soln=None, resid=None,
                      msg="breakdown dot(p, Ap)==0")
                continue
            alpha = c["udr"] / pTAp                                          # :118
            c["x"] = c["x"] + alpha * c["p"]                                 # :121
            c["r"] = c["r"] - alpha * Ap                                     # :122
            c["u"] = apply(c["r"])                                           # :123
            normR = math.sqrt(dot(c["r"], c["r"]))                           # :125
            c["hist"].append(normR)
            tol = normR <= tau * c["normB"]
            if tol or ((not fail_on_maxiter) and k == maxiter - 1):          # :129-131
                _stop(c, status="converged", exit="tolerance" if tol else "maxiter", success=True, iters=k + 1,
                      soln=c["x"], resid=normR, msg=None)
                continue
            new = dot(c["u"], c["r"])                                        # :134
            beta = new / c["udr"]                                            # :135
            c["udr"] = new                                                   # :136
            c["p"] = c["u"] + beta * c["p"]                                  # :138
    for c in cols:
        if not c["done"]:                                                    # handleMaxiter(maxiter - 1, ...)
            last = c["hist"][-1] if c["hist"] else None
            _stop(c, status="maxiter", exit="maxiter", success=not fail_on_maxiter, iters=max(maxiter - 1, 0),
                  soln=c["x"], resid=last, msg="failure to converge" if fail_on_maxiter else None)
    return [c["out"] for c in cols]


def _stop(c, **kw):
    c["done"] = True
    c["out"] = dict(kw, hist=np.array(c["hist"], dtype=np.float64), norm_b=c["normB"], x=c["x"])


def spread(results):
    """max over the entries the runs share of the largest pairwise history difference, over ||b||."""
    L = min(len(r["hist"]) for r in results)
    if L == 0:
        return 0.0
    H = np.array([r["hist"][:L] for r in results])
    return float(np.max(H.max(axis=0) - H.min(axis=0)) / results[0]["norm_b"])


def counts_comparable(res, tau):
    """Equal iteration counts may be asserted: the runs (one per dot order) agree on status and iters, and no history
    entry of any of them lies within a relative 1e-6 of tau ||b|| (the dot orders move an entry by ~1e-13 of it)."""
    if len({r["iters"] for r in res}) != 1 or len({r["status"] for r in res}) != 1:
        return False
    for r in res:
        th = tau * r["norm_b"]
        if th > 0 and np.any(np.abs(r["hist"] - th) <= 1e-6 * th):
            return False
    return True


# ---- the inputs of tests/test_gpu_pcg_multi.py --------------------------------------------------------------------
# random SPD: n = 1, 2, the tile edges T - 1, T, T + 1, 2T + 1 and the smallest n of 257 tiles (the first two-level
# gridsum); FD sides 17 and 363; the arrow matrices
RAND_N = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 256 * TILE + 1)
CASES = ["rand%d" % n for n in RAND_N] + ["fd17", "fd363", "arrow1100", "arrow1500"]
PRECS = ("identity", "jacobi")
DEPTHS = (1, 2, 9)


def arrow(n, hub=5, seed=11):
    """Symmetric, strictly diagonally dominant, row and column `hub` full: one row of n entries (n = 1100: the hub's
    tile holds more entries than one staging chunk of 1280; n = 1500: the hub row alone does), its entries stored
    in shuffled order, the other rows [diagonal, hub]."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, size=n)
    v[hub] = 0.0
    i = np.arange(n)
    off = sp.coo_matrix((np.concatenate([v, v]), (np.concatenate([np.full(n, hub), i]), np.concatenate([i, np.full(n, hub)]))),
                        shape=(n, n)).tocsr()
    off.eliminate_zeros()
    d = np.asarray(abs(off).sum(axis=1)).ravel() + rng.uniform(0.5, 1.5, size=n)
    A = (off + sp.diags(d)).tocsr()
    A.sort_indices()
    ip, ind, dat = A.indptr, A.indices.copy(), A.data.copy()
    s, e = ip[hub], ip[hub + 1]
    perm = rng.permutation(e - s)
    ind[s:e], dat[s:e] = ind[s:e][perm], dat[s:e][perm]
    A = sp.csr_matrix((dat, ind, ip.copy()), shape=(n, n))
    A.has_sorted_indices = False
    return A


def matrix(name):
    if name.startswith("arrow"):
        return arrow(int(name[5:]))
    return pr.matrix(name)


def size(name):
    return int(name[2:]) ** 2 if name.startswith("fd") else int(name[5:] if name.startswith("arrow") else name[4:])


def columns(name, m=MULTI_MAX):
    """(n, m): column 0 is pcg_replay.rhs for the generator's cases; the others independent normal vectors of other
    scales (a column's scale must not matter to its neighbours)."""
    n = size(name)
    rng = np.random.default_rng(1000 + 7 * n + len(name))
    B = rng.standard_normal((n, m)) * np.array([1.0, 3.0, 0.25, 100.0])[:m]
    if not name.startswith("arrow"):
        B[:, 0] = pr.rhs(name)
    return np.ascontiguousarray(B)


def depths(n):
    """DEPTHS capped by n, as pcg_replay.depths does."""
    return [K for K in DEPTHS if K <= n]


def fd_eigenvector(m, p=2, q=3):
    """sin(p pi i / (m+1)) sin(q pi j / (m+1)) on the m x m grid: an eigenvector of the 5-point stencil with Dirichlet
    boundaries, so CG on it stops after its first iteration."""
    t = np.arange(1, m + 1) * np.pi / (m + 1)
    return np.ascontiguousarray(np.outer(np.sin(q * t), np.sin(p * t)).ravel())


def mixed_columns(m=17):
    """[random, 0, an eigenvector (stops at iteration 1), random scaled by 1e-200] on FD m^2."""
    n = m * m
    rng = np.random.default_rng(4242)
    B = np.zeros((n, 4))
    B[:, 0] = rng.standard_normal(n)
    B[:, 2] = fd_eigenvector(m)
    B[:, 3] = rng.standard_normal(n) * 1e-200
    return B


def indefinite_diagonal(n=290):
    """diag(+2, -2, +2, ...): under Jacobi DInv = +-1/2 exactly and b = ones has u.r = sum(+-1/2) = 0 exactly in any
    summation order: the dot(u,r) == 0 breakdown at the start."""
    d = np.where(np.arange(n) % 2 == 0, 2.0, -2.0)
    return sp.diags(d).tocsr()


def breakdown_columns(n=290):
    """[random, ones (u.r == 0 under Jacobi on indefinite_diagonal), 0]"""
    rng = np.random.default_rng(99)
    B = np.zeros((n, 3))
    B[:, 0] = rng.standard_normal(n)
    B[:, 1] = 1.0
    return B
