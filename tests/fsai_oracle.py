"""CPU restatement of the factorized sparse approximate inverse (TEST INFRASTRUCTURE).

The arithmetic include/psk.h states for psk_csr_fsai, in numpy float64 with one rounding per operation. It has no
reference counterpart, so this file is the definition the device code is pinned to, bit for bit:

    s = sign of row 0's stored diagonal entry; the factorisation runs on s A (an exact flip)
    row i: J = the pattern row's columns <= i, ascending, m = |J| <= ROW_CAP, i in J
      B[a][b] = s * (A[J[a], J[b]] or 0.0)                                   0 <= b <= a < m (A's lower triangle)
      b = 0..m-1, a = b..m-1: t = B[a][b]; t = t - C[a][k] * C[b][k], k = 0..b-1 ascending
                              a == b: t > 0 and finite, C[b][b] = sqrt(t); else C[a][b] = t / C[b][b]
      g[m-1] = 1 / C[m-1][m-1]; a = m-2..0: u = 0.0; u = u + C[b][a] * g[b], b = a+1..m-1 ascending;
                                            g[a] = (-u) / C[a][a]
      row i of G = (J, g)
    apply(v) = (s G^T)(G v), both products as scipy's csr_matvec (stored-order sums of rounded products)

The elementwise steps over `a` (one column of the Cholesky factor, the products of one back-substitution step) are
numpy array operations: each element is still one IEEE multiply, subtract or divide, rounded once, so the bits are
those of the scalar loops; every SUM runs as an explicit ascending loop of scalar adds.
"""
import math

import numpy as np
import scipy.sparse as sp

from oracle import krylov

ROW_CAP = 64


class PivotError(ValueError):
    """A pivot of some row's small Cholesky factorisation is not positive and finite: s A is not positive definite
    on that row's index set."""

    def __init__(self, row):
        super().__init__("not positive definite (row %d)" % row)
        self.row = row


def _sorted_rows(M, what):
    """(indptr, indices, data) of M with every row in ascending column order; duplicates are refused."""
    M = M.tocsr()
    ip = np.asarray(M.indptr, dtype=np.int64)
    ix = np.array(M.indices, dtype=np.int64)
    dt = np.array(M.data, dtype=np.float64)
    for i in range(M.shape[0]):
        lo, hi = ip[i], ip[i + 1]
        o = np.argsort(ix[lo:hi], kind="stable")
        ix[lo:hi] = ix[lo:hi][o]
        dt[lo:hi] = dt[lo:hi][o]
        if np.any(np.diff(ix[lo:hi]) == 0):
            raise ValueError("duplicate column in row %d of %s" % (i, what))
    return ip, ix, dt


def sign_of(A):
    """+1 / -1 from row 0's stored diagonal entry (zero, missing or non-finite: ValueError)."""
    A = A.tocsr()
    lo, hi = A.indptr[0], A.indptr[1]
    hit = np.nonzero(A.indices[lo:hi] == 0)[0]
    if hit.size != 1:
        raise ValueError("row 0 has no (single) stored diagonal entry")
    d = float(A.data[lo + hit[0]])
    if d == 0.0 or not math.isfinite(d):
        raise ValueError("row 0's diagonal entry is zero or not finite")
    return 1 if d > 0.0 else -1


def fsai_row(sa, J, rows):
    """g for one index set J (ascending, the row itself last); rows(r) = (columns, values) of A's sorted row r.
    Returns None when a pivot fails."""
    m = len(J)
    B = np.zeros((m, m), dtype=np.float64)
    for a in range(m):
        cols, vals = rows(J[a])
        want = J[:a + 1]
        pos = np.searchsorted(cols, want)
        ok = pos < len(cols)
        ok[ok] = cols[pos[ok]] == want[ok]
        x = np.zeros(a + 1, dtype=np.float64)
        x[ok] = vals[pos[ok]]
        B[a, :a + 1] = sa * x
    C = np.zeros((m, m), dtype=np.float64)
    for b in range(m):
        t = B[b:, b].copy()
        for k in range(b):
            t = t - C[b:, k] * C[b, k]
        piv = float(t[0])
        if not (piv > 0.0 and math.isfinite(piv)):
            return None
        C[b, b] = math.sqrt(piv)
        C[b + 1:, b] = t[1:] / C[b, b]
    g = np.zeros(m, dtype=np.float64)
    g[m - 1] = 1.0 / C[m - 1, m - 1]
    for a in range(m - 2, -1, -1):
        prod = C[a + 1:, a] * g[a + 1:]
        u = 0.0
        for q in prod.tolist():
            u = u + q
        g[a] = (-u) / C[a, a]
    return g


def fsai(A, pattern=None):
    """(G, sign): G as scipy CSR, row i = (J ascending, g). pattern=None: A's own pattern."""
    A = A.tocsr()
    n, nc = A.shape
    if n != nc or n == 0:
        raise ValueError("A must be square and not empty")
    aip, aix, adt = _sorted_rows(A, "A")
    if pattern is None:
        pip, pix = aip, aix
    else:
        if pattern.shape != A.shape:
            raise ValueError("the pattern must have A's shape")
        pip, pix, _ = _sorted_rows(pattern, "the pattern")
    s = sign_of(A)
    sa = float(s)

    def rows(r):
        return aix[aip[r]:aip[r + 1]], adt[aip[r]:aip[r + 1]]

    gp = np.zeros(n + 1, dtype=np.int32)
    gi, gv = [], []
    for i in range(n):
        row = pix[pip[i]:pip[i + 1]]
        J = row[row <= i]
        if J.size == 0 or J[-1] != i:
            raise ValueError("pattern row %d does not hold its diagonal" % i)
        if J.size > ROW_CAP:
            raise OverflowError("pattern row %d has %d lower entries (cap %d)" % (i, J.size, ROW_CAP))
        g = fsai_row(sa, J, rows)
        if g is None:
            raise PivotError(i)
        gi.append(J)
        gv.append(g)
        gp[i + 1] = gp[i] + J.size
    G = sp.csr_matrix((np.concatenate(gv), np.concatenate(gi).astype(np.int32), gp), shape=(n, n))
    return G, s


class FSAI:
    """The operator as a callable, with the product's introspection names (sign, nnz, max_row)."""

    def __init__(self, A, power=1):
        if power == 1:
            pattern = None
        elif power == 2:
            pattern = (A.tocsr() @ A.tocsr()).tocsr()
        else:
            raise ValueError("power must be 1 or 2")
        self.A = A
        self.G, self.sign = fsai(A, pattern)
        self.Gt = self.G.T.tocsr()
        self.Gt.data = float(self.sign) * self.Gt.data
        self.nnz = self.G.nnz
        self.max_row = int(np.max(np.diff(self.G.indptr)))

    def __call__(self, v):
        v = np.asarray(v, dtype=np.float64)
        return krylov.mvmult(self.Gt, krylov.mvmult(self.G, v))


def apply(G, sign, v):
    """(sign G^T)(G v) for a G from fsai()."""
    Gt = G.T.tocsr()
    Gt.data = float(sign) * Gt.data
    return krylov.mvmult(Gt, krylov.mvmult(G, np.asarray(v, dtype=np.float64)))
