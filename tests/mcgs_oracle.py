"""CPU oracle of the multicolour Gauss-Seidel preconditioner (psk_color_plan, psk_prec_create_mcgs): the colouring as
plain Python and the apply in numpy, one rounded operation at a time in the order include/psk.h states.

Colouring: first-fit greedy in natural row order on the structure of A + A^T (stored zeros count, duplicates and
unsorted rows are fine). Apply: z = 0; ``sweeps`` times, for colour k in ORDER, for every row i of colour k:
acc = 0.0; acc = acc + a_ij * z_j over the row's stored entries in stored order (diagonal included);
z_i = z_i + DInv_i * (v_i - acc), with DInv_i = 1.0 / (the sum of the row's col == row entries in stored order).

``apply_scalar`` is that text literally, one Python float operation at a time. ``MCGS.__call__`` runs the same
operations with numpy across the rows of a colour (entry slot by entry slot: elementwise multiply, then elementwise
add, each rounded once and never fused), which gives every row the same sequence of roundings; test_mcgs_cpu.py checks
the two agree bit for bit.
"""
import numpy as np

MAX_COLORS = 64


def coloring(A):
    """(color, ncolors) for a square scipy CSR A."""
    A = A.tocsr()
    n = A.shape[0]
    ip, ix = A.indptr, A.indices
    nbr = [set() for _ in range(n)]
    for i in range(n):
        for j in ix[ip[i]:ip[i + 1]]:
            if j != i:
                nbr[i].add(int(j))
                nbr[int(j)].add(i)
    color = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        used = {color[j] for j in nbr[i] if color[j] >= 0}
        c = 0
        while c in used:
            c += 1
        color[i] = c
    return color, int(color.max()) + 1


def order(ncolors, symmetric):
    fwd = list(range(ncolors))
    return fwd + fwd[-2::-1] if symmetric else fwd


def dinv(A):
    """1.0 / (sum of row i's col == row entries in stored order); ValueError naming the first bad row."""
    A = A.tocsr()
    n = A.shape[0]
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        d = np.float64(0.0)
        for e in range(A.indptr[i], A.indptr[i + 1]):
            if A.indices[e] == i:
                d = d + A.data[e]
        if d == 0.0 or not np.isfinite(d):
            raise ValueError("the diagonal entry of row %d is zero, missing or not finite" % i)
        out[i] = np.float64(1.0) / d
    return out


def apply_scalar(A, v, sweeps=1, symmetric=True):
    """The definition, one scalar operation at a time."""
    A = A.tocsr()
    ip, ix, dt = A.indptr, A.indices, A.data.astype(np.float64)
    color, nc = coloring(A)
    di = dinv(A)
    v = np.asarray(v, dtype=np.float64)
    z = np.zeros(A.shape[0], dtype=np.float64)
    for _ in range(sweeps):
        for k in order(nc, symmetric):
            for i in np.flatnonzero(color == k):
                acc = np.float64(0.0)
                for e in range(ip[i], ip[i + 1]):
                    acc = acc + dt[e] * z[ix[e]]
                z[i] = z[i] + di[i] * (v[i] - acc)
    return z


class MCGS:
    """The operator as a callable (usable as ``precond=`` of oracle.krylov), with the product's introspection names."""

    def __init__(self, A, sweeps=1, symmetric=True):
        A = A.tocsr()
        if A.shape[0] != A.shape[1] or A.shape[0] == 0:
            raise ValueError("A must be square and not empty")
        if sweeps < 1:
            raise ValueError("sweeps must be >= 1")
        self.n = A.shape[0]
        self.sweeps, self.symmetric = int(sweeps), bool(symmetric)
        self.color, self.ncolors = coloring(A)
        if self.ncolors > MAX_COLORS:
            raise OverflowError("the colouring needs %d colours (cap %d)" % (self.ncolors, MAX_COLORS))
        self.color_rows = np.bincount(self.color, minlength=self.ncolors).astype(np.int64)
        self.dinv = dinv(A)
        ip, ix, dt = A.indptr, A.indices, A.data.astype(np.float64)
        length = np.diff(ip)
        # per colour: its rows (ascending) and, per entry slot s, the rows that have a slot s with its column and value
        self._plan = []
        for k in range(self.ncolors):
            rows = np.flatnonzero(self.color == k)
            slots = []
            for s in range(int(length[rows].max()) if rows.size else 0):
                sel = np.flatnonzero(length[rows] > s)
                e = ip[rows[sel]] + s
                slots.append((sel, ix[e].astype(np.int64), dt[e]))
            self._plan.append((rows, slots))

    def __call__(self, v):
        v = np.asarray(v, dtype=np.float64)
        z = np.zeros(self.n, dtype=np.float64)
        for _ in range(self.sweeps):
            for k in order(self.ncolors, self.symmetric):
                rows, slots = self._plan[k]
                acc = np.zeros(rows.size, dtype=np.float64)
                for sel, cols, vals in slots:
                    prod = vals * z[cols]              # rounded product
                    acc[sel] = acc[sel] + prod         # then the add, in stored order per row
                res = v[rows] - acc
                upd = self.dinv[rows] * res
                z[rows] = z[rows] + upd
        return z
