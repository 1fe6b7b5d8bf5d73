"""CPU restatement of the Jacobi-sweep triangular apply (TEST INFRASTRUCTURE).

The operator include/psk.h states for psk_prec_trisolve_sweeps, in numpy float64. It has no reference counterpart
(the reference's triangular applies are exact), so this file is the definition the device code is compared with:

    T = D + N (N the off-diagonal entries, d the diagonal; a unit factor has d = 1 and its stored diagonal is ignored)
    x0 = b / d;   x(j) = (b - N x(j-1)) / d,  j = 1..s;   x = x(s)          (unit: no division)

N x is scipy's csr_matvec: a row's rounded products added in stored order. The device adds the same products with
fma in 1, 4, 16 or 64 lane partial sums, so the two agree to the rounding of a row sum (the project's apply bar,
1e-12 of max|x|), not bit for bit.

A chain is (gather_in, L, U, gather_out) as psk_prec_create_trisolve takes it:
out = (U^-1 L^-1 v[gather_in])[gather_out], each factor exact (spsolve_triangular) or swept.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def split(T, unit=False):
    """(N, d): the off-diagonal entries of T as CSR in T's stored order, and the diagonal (None for a unit factor)."""
    T = sp.csr_matrix(T)
    n = T.shape[0]
    rows = np.repeat(np.arange(n), np.diff(T.indptr))
    off = T.indices != rows
    counts = np.bincount(rows[off], minlength=n)
    ip = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    N = sp.csr_matrix((T.data[off].astype(np.float64), T.indices[off].astype(np.int32), ip), shape=(n, n))
    N.has_sorted_indices = False
    return N, (None if unit else np.asarray(T.diagonal(), dtype=np.float64))


def sweep_solve(T, b, s, unit=False):
    """x(s) for T x = b."""
    N, d = split(T, unit)
    b = np.asarray(b, dtype=np.float64)
    x = np.copy(b) if d is None else b / d
    for _ in range(int(s)):
        r = b - N @ x
        x = r if d is None else r / d
    return x


def exact_solve(T, b, lower, unit=False):
    return spla.spsolve_triangular(sp.csr_matrix(T), np.asarray(b, dtype=np.float64), lower=lower, unit_diagonal=unit)


def levels(T, lower):
    """The number of dependency levels of T's off-diagonal pattern (1 for a diagonal factor)."""
    N, _ = split(T)
    n = N.shape[0]
    lev = np.zeros(n, dtype=np.int64)
    ip, ix = N.indptr, N.indices
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        c = ix[ip[i]:ip[i + 1]]
        if c.size:
            lev[i] = lev[c].max() + 1
    return int(lev.max()) + 1 if n else 0


class Chain:
    """out = (U^-1 L^-1 v[gather_in])[gather_out] with s_l / s_u sweeps in place of a solve (0: exact)."""

    def __init__(self, L=None, l_unit=False, U=None, u_unit=False, gather_in=None, gather_out=None, s_l=0, s_u=0):
        self.L, self.l_unit, self.U, self.u_unit = L, l_unit, U, u_unit
        self.gather_in, self.gather_out, self.s_l, self.s_u = gather_in, gather_out, int(s_l), int(s_u)

    def __call__(self, v):
        x = np.asarray(v, dtype=np.float64)
        if self.gather_in is not None:
            x = x[np.asarray(self.gather_in)]
        if self.L is not None:
            x = (sweep_solve(self.L, x, self.s_l, self.l_unit) if self.s_l > 0
                 else exact_solve(self.L, x, True, self.l_unit))
        if self.U is not None:
            x = (sweep_solve(self.U, x, self.s_u, self.u_unit) if self.s_u > 0
                 else exact_solve(self.U, x, False, self.u_unit))
        if self.gather_out is not None:
            x = x[np.asarray(self.gather_out)]
        return np.array(x)


def ilu0_chain(F, s_l=0, s_u=0):
    """The chain of an ILU(0) factor F (tests/ilu0_oracle.py): L = strict-lower(F) with a unit diagonal, U = upper(F)."""
    n = F.shape[0]
    L = (sp.tril(F, k=-1) + sp.identity(n)).tocsr()
    U = sp.triu(F, k=0).tocsr()
    return Chain(L=L, l_unit=True, U=U, u_unit=False, s_l=s_l, s_u=s_u)


def superlu_chain(ilu, s_l=0, s_u=0):
    """The chain of a SuperLU object as psk_prec_create_ilu builds it: bb[perm_r[i]] = v[i], unit L, U,
    out[i] = z[perm_c[i]]."""
    pinv = np.empty_like(ilu.perm_r)
    pinv[ilu.perm_r] = np.arange(ilu.perm_r.shape[0])
    return Chain(L=ilu.L.tocsr(), l_unit=True, U=ilu.U.tocsr(), u_unit=False, gather_in=pinv, gather_out=ilu.perm_c,
                 s_l=s_l, s_u=s_u)
