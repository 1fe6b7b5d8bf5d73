"""CPU restatement of ILU(0) as include/psk.h defines it for psk_csr_ilu0 (TEST INFRASTRUCTURE).

The method has no reference counterpart, so this file is the definition the device code is pinned to, statement by
statement in the header's order and in Python floats (IEEE doubles, one rounding per operation, no FMA):

    work on the copy of A whose rows are in ascending column order, values v; for i = 0 .. n-1:
      for each entry e of row i with column k < i, in ascending k:
        l = v[e] / v[diag(k)];  v[e] = l
        for each entry f of row k with column j > k, in ascending j:
          if row i stores column j at q:  v[q] = v[q] - l * v[f]
      the pivot v[diag(i)] is in error when it is 0.0 or not finite

F has A's sorted pattern; L = strict-lower(F) with a unit diagonal, U = upper(F) with the diagonal.
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


class PivotError(ArithmeticError):
    def __init__(self, row):
        super().__init__("zero or non-finite pivot in row %d" % row)
        self.row = row


def sorted_copy(A):
    """A's entries with every row in ascending column order (a stable sort of each row; no entry summed or dropped)."""
    A = sp.csr_matrix(A)
    ip = A.indptr
    rows = np.repeat(np.arange(A.shape[0]), np.diff(ip))
    perm = np.lexsort((A.indices, rows))
    S = sp.csr_matrix((A.data[perm].astype(np.float64), A.indices[perm].astype(np.int32), ip.astype(np.int32)),
                      shape=A.shape)
    S.has_sorted_indices = True
    return S


def ilu0(A):
    """F (scipy CSR, sorted rows). Raises ValueError for a non-square matrix, a duplicate column or a missing
    diagonal, PivotError for a zero or non-finite pivot."""
    S = sorted_copy(A)
    n, nc = S.shape
    if n != nc or n == 0:
        raise ValueError("ILU(0) needs a square, non-empty matrix")
    rp, ci, v = S.indptr.tolist(), S.indices.tolist(), S.data.tolist()
    diag = [-1] * n
    for i in range(n):
        for e in range(rp[i], rp[i + 1]):
            if e > rp[i] and ci[e] == ci[e - 1]:
                raise ValueError("duplicate column in row %d" % i)
            if ci[e] == i:
                diag[i] = e
        if diag[i] < 0:
            raise ValueError("row %d has no stored diagonal entry" % i)
    for i in range(n):
        pos = {ci[q]: q for q in range(rp[i], rp[i + 1])}
        for e in range(rp[i], diag[i]):              # columns k < i, ascending
            k = ci[e]
            l = v[e] / v[diag[k]]
            v[e] = l
            for f in range(diag[k] + 1, rp[k + 1]):  # columns j > k of row k, ascending
                q = pos.get(ci[f])
                if q is not None:
                    p = l * v[f]                     # the product rounded,
                    v[q] = v[q] - p                  # then the difference
        piv = v[diag[i]]
        if piv == 0.0 or not math.isfinite(piv):
            raise PivotError(i)
    F = sp.csr_matrix((np.array(v, dtype=np.float64), S.indices, S.indptr), shape=S.shape)
    F.has_sorted_indices = True
    return F


def split(F):
    """(L, U): strict-lower(F) plus a unit diagonal, and upper(F) with the diagonal, both CSR."""
    n = F.shape[0]
    L = (sp.tril(F, k=-1) + sp.identity(n)).tocsr()
    U = sp.triu(F, k=0).tocsr()
    return L, U


def apply(F):
    """v -> U^-1 (L^-1 v) through scipy's spsolve_triangular (L unit-lower, then U)."""
    L, U = split(F)

    def M(v):
        y = spla.spsolve_triangular(L, np.asarray(v, dtype=np.float64), lower=True, unit_diagonal=True)
        return spla.spsolve_triangular(U, y, lower=False)

    return M
