"""The matrices the multicolour Gauss-Seidel tests share (test_mcgs_cpu.py, test_gpu_mcgs.py), by name."""
import functools
import os

import numpy as np
import scipy.io
import scipy.sparse as sp

from conftest import GOLDEN
from oracle import fdlap


def _shuffle_rows(A, seed):
    """The same matrix with every row's entries stored in a shuffled order."""
    A = A.tocsr()
    rng = np.random.default_rng(seed)
    ix, dt = A.indices.copy(), A.data.copy()
    for i in range(A.shape[0]):
        a, b = A.indptr[i], A.indptr[i + 1]
        p = rng.permutation(b - a)
        ix[a:b], dt[a:b] = A.indices[a:b][p], A.data[a:b][p]
    return sp.csr_matrix((dt, ix, A.indptr.copy()), shape=A.shape)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The named matrix, built once. Its arrays are read-only: some scipy conversions (tolil, sum_duplicates) sort a
    CSR matrix's rows in place, which would silently change the stored order between two users of the cache."""
    A = _build(name)
    for a in (A.data, A.indices, A.indptr):
        a.setflags(write=False)
    return A


def _build(name):
    if name.startswith("negfd"):
        return (-fdlap.fd_laplacian_2d(-1.0, 1.0, int(name[5:]))).tocsr()
    if name in ("dh8", "dh10"):
        return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-%s.mtx" % name[2:])).tocsr()
    if name == "diag":          # 1 colour
        return sp.csr_matrix(sp.diags(np.linspace(1.0, 3.0, 37)))
    if name == "one":           # 1 x 1
        return sp.csr_matrix(np.array([[2.5]]))
    if name == "nonsym":        # 300 rows, a pattern that is not symmetric, rows diagonally dominant
        rng = np.random.default_rng(7)
        R = sp.random(300, 300, density=0.02, random_state=rng, data_rvs=lambda k: rng.uniform(-1.0, 1.0, k)).tocsr()
        R.setdiag(0.0)
        R.eliminate_zeros()
        A = (R + sp.diags(np.asarray(abs(R).sum(axis=1)).ravel() + 1.0)).tocsr()
        assert (A != A.T).nnz > 0 and ((A != 0) != (A.T != 0)).nnz > 0
        return A
    if name == "shuffled":      # -FD 16^2 with shuffled rows, a stored zero on an edge of A and one off its pattern
        A = matrix("negfd16").tocoo()
        assert np.count_nonzero((A.row == 5) & (A.col == 6)) == 1
        rows = np.concatenate([A.row, [0]])
        cols = np.concatenate([A.col, [34]])
        vals = np.concatenate([A.data, [0.0]])
        vals[(rows == 5) & (cols == 6)] = 0.0
        B = sp.csr_matrix((vals, (rows, cols)), shape=A.shape)      # keeps explicit zeros
        B = _shuffle_rows(B, 11)
        assert B.nnz == matrix("negfd16").nnz + 1 and np.count_nonzero(B.data == 0.0) == 2
        return B
    if name == "longrow":       # tridiagonal, and row 7 holds 1500 entries: more than a wave and more than one chunk
        n = 1600
        T = sp.diags([-np.ones(n - 1), 4.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tolil()
        rng = np.random.default_rng(5)
        T[7, :1500] = rng.uniform(-1.0, 1.0, 1500) / 1500.0
        T[7, 7] = 4.0
        return _shuffle_rows(T.tocsr(), 13)
    if name == "dense70":       # needs 70 colours
        return sp.csr_matrix(np.ones((70, 70)) + 70.0 * np.eye(70))
    raise KeyError(name)
