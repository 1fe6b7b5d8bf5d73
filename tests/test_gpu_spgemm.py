"""GPU tests of the device-side operator construction (pysolvers_amd/csrc/spgemm.hip): psk_csr_matmat,
psk_csr_transpose and psk_sa_prolongator.

The bar is equality, written here and not inferred: every result, downloaded with to_scipy(), has the indptr, the
indices and the BIT PATTERNS of the data of scipy's own result on the same stored arrays (`A @ B`,
`A.transpose().tocsr()`, SmoothedAggregation.SA_coarsen). Entry order is part of the contract: every SpMV of the
library sums a row in stored order.
"""
import ctypes
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    return pysolvers_amd


@pytest.fixture(scope="module")
def N():
    from pysolvers_amd import _native
    return _native


def _dev(psk, A):
    return psk.DeviceCSR.from_scipy(A, rectangular=True)


def _same(C, ref):
    """indptr, indices and the data's bit patterns (and the shape) of two CSR matrices."""
    assert C.shape == ref.shape
    assert np.array_equal(C.indptr, ref.indptr)
    assert np.array_equal(C.indices, ref.indices)
    assert np.array_equal(np.asarray(C.data, dtype=np.float64).view(np.int64),
                          np.asarray(ref.data, dtype=np.float64).view(np.int64))


def _raw(shape, rows):
    """CSR from per-row lists of (column, value), kept exactly as given (order, duplicates, zeros)."""
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    indices = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    data = np.array([v for r in rows for _, v in r], dtype=np.float64)
    A = sp.csr_matrix((data, indices, indptr), shape=shape)
    assert A.nnz == len(data)
    return A


def _random(rng, m, n, density, small_ints):
    """Random m x n CSR, every row's entries shuffled into unsorted stored order. small_ints: values in
    {-2, ..., 2} (exact cancellations in products, explicit zeros stored), else standard normal."""
    A = sp.random(m, n, density=density, random_state=rng, format="csr")
    A.sort_indices()
    data = (rng.integers(-2, 3, size=A.nnz).astype(np.float64) if small_ints else rng.standard_normal(A.nnz))
    indices = A.indices.copy()
    for i in range(m):
        p = rng.permutation(A.indptr[i + 1] - A.indptr[i]) + A.indptr[i]
        indices[A.indptr[i]:A.indptr[i + 1]] = A.indices[p]
    out = sp.csr_matrix((data, indices, A.indptr.copy()), shape=(m, n))
    out.has_sorted_indices = False
    return out


@pytest.fixture(scope="module")
def operands():
    """(A, B) for the two random cases, shared and never modified."""
    out = {}
    for name, ints in (("normal", False), ("ints", True)):
        rng = np.random.default_rng(20251 if ints else 20250)
        out[name] = (_random(rng, 200, 150, 0.08, ints), _random(rng, 150, 180, 0.08, ints))
    return out


@pytest.mark.parametrize("name", ["normal", "ints"])
def test_matmat_random_rectangular(psk, operands, name):
    A, B = operands[name]
    ref = A @ B
    if name == "ints":   # the case is about cancellation: explicit zeros stored, and sums that cancel dropped
        assert (A.data == 0).any() and (B.data == 0).any()
        ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices.copy(), M.indptr.copy()), shape=M.shape)
        assert ref.nnz < (ones(A) @ ones(B)).nnz         # the structural product (on copies: A and B stay as stored)
    C = psk.Linear.matmat(_dev(psk, A), _dev(psk, B))
    assert (C.n, C.ncols, C.nnz) == (200, 180, ref.nnz)
    _same(C.to_scipy(), ref)


def _edge_operands(N, extra=0):
    """A (rows with chosen product counts) and B. B's rows: 0: 1 entry, 1: 63, 2: 64, 3: 65, 4: 32, 5: five entries
    all on column 7 (duplicates in a row of B), 6: duplicates mixed with others, 7: empty."""
    cap = N.PSK_SPGEMM_ROW_CAP
    assert cap == 1024
    rng = np.random.default_rng(7)
    nb = 90

    def brow(k):
        cols = rng.permutation(nb)[:k]
        return [(int(c), float(v)) for c, v in zip(cols, rng.standard_normal(k))]

    B = [brow(1), brow(63), brow(64), brow(65), brow(32), [(7, 0.5), (7, -1.25), (7, 3.0), (7, 0.125), (7, -2.0)],
         [(3, 1.0), (11, 2.0), (3, -1.0), (11, 0.5), (4, 4.0), (3, 0.25)], []]
    v = lambda k: [float(x) for x in rng.standard_normal(k)]
    A = [[],                                             # 0 entries
         [(0, 2.0)],                                     # 1 product
         [(1, -1.5)],                                    # 63
         [(2, 0.75)],                                    # 64
         [(3, 1.25)],                                    # 65
         [(4, x) for x in v(cap // 32)],                 # cap products: 32 duplicates of one column of A
         [(2, x) for x in v(cap // 64)],                 # cap products again, 16 x 64
         [(5, 1.0), (5, -3.0), (5, 0.5)],                # every product on the single column 7
         [(7, 1.0)],                                     # an entry of A naming an empty row of B: 0 products
         [(6, 1.0), (1, 2.0), (6, -1.0)],                # duplicates in a row of A and in a row of B; cancels
         [(2, x) for x in v(4)],                         # 256: the last row of the small bin
         [(2, x) for x in v(4)] + [(0, 1.0)],            # 257: the first of the large bin
         []]
    if extra:
        A.append([(4, x) for x in v(cap // 32)] + [(0, 1.0)] * extra)   # cap + extra products
    return _raw((len(A), len(B)), A), _raw((len(B), nb), B)


def test_matmat_row_edges(psk, N):
    A, B = _edge_operands(N)
    prods = [sum(B.indptr[c + 1] - B.indptr[c] for c in A.indices[A.indptr[i]:A.indptr[i + 1]])
             for i in range(A.shape[0])]
    assert prods == [0, 1, 63, 64, 65, 1024, 1024, 15, 0, 75, 256, 257, 0]
    ref = A @ B
    assert ref.indptr[8] - ref.indptr[7] == 1            # the single-column row
    _same(psk.Linear.matmat(_dev(psk, A), _dev(psk, B)).to_scipy(), ref)


def test_matmat_cap_overflow_is_unsupported(psk, N):
    A, B = _edge_operands(N, extra=1)
    dA, dB = _dev(psk, A), _dev(psk, B)
    h = ctypes.c_void_p(0x5A5A)
    assert N.lib.psk_csr_matmat(dA.handle, dB.handle, ctypes.byref(h)) == N.PSK_ERR_UNSUPPORTED
    assert h.value == 0x5A5A                             # *C untouched
    with pytest.raises(N.PskError) as e:
        psk.Linear.matmat(dA, dB)
    assert e.value.code == N.PSK_ERR_UNSUPPORTED


def test_matmat_shape_mismatch_is_arg_error(psk, N, operands):
    A, B = operands["normal"]
    dA = _dev(psk, A)
    h = ctypes.c_void_p(0x5A5A)
    assert N.lib.psk_csr_matmat(dA.handle, dA.handle, ctypes.byref(h)) == N.PSK_ERR_ARG   # 200x150 by 200x150
    assert h.value == 0x5A5A
    with pytest.raises(ValueError):
        psk.Linear.matmat(dA, dA)


def _dups():
    return _raw((5, 4), [[(2, 1.0), (0, 2.0), (2, 3.0)], [], [(3, -1.0), (3, 0.0), (1, 5.0)], [(2, 7.0)],
                         [(0, 0.5), (1, 0.25), (0, -0.5), (3, 8.0)]])


@pytest.mark.parametrize("which", ["normal_A", "normal_B", "ints_A", "dups", "edge_A"])
def test_transpose(psk, N, operands, which):
    M = {"normal_A": operands["normal"][0], "normal_B": operands["normal"][1], "ints_A": operands["ints"][0],
         "dups": _dups(), "edge_A": _edge_operands(N)[0]}[which]
    T = _dev(psk, M).transpose()
    ref = M.transpose().tocsr()
    assert (T.n, T.ncols, T.nnz) == (M.shape[1], M.shape[0], M.nnz)
    _same(T.to_scipy(), ref)
    # twice: the rows sorted by column, entries of one column in their stored order (a stable sort of each row)
    TT = T.transpose().to_scipy()
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    order = np.lexsort((np.arange(M.nnz), M.indices, rows))
    _same(TT, sp.csr_matrix((M.data[order], M.indices[order], M.indptr), shape=M.shape))
    assert all(np.all(np.diff(TT.indices[TT.indptr[i]:TT.indptr[i + 1]]) >= 0) for i in range(M.shape[0]))


def _negfd(m):
    from oracle import fdlap
    return sp.csr_matrix(-fdlap.fd_laplacian_2d(-1.0, 1.0, m))


def _dh8():
    return sp.csr_matrix(scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr())


@pytest.mark.parametrize("which", ["fd24", "dh8"])
def test_sa_prolongator(psk, N, which):
    from pysolvers_amd.Linear import SmoothedAggregation as SA
    A = _negfd(24) if which == "fd24" else _dh8()
    ref, agg_ref = SA.SA_coarsen(A)
    agg, count, afv = SA.BuildAggregates(A)
    assert np.array_equal(agg, agg_ref)
    dA = psk.DeviceCSR.from_scipy(A)
    h = ctypes.c_void_p()
    N.check(N.lib.psk_sa_prolongator(dA.handle, N.ptr(agg), count, N.ptr(afv), 2 / 3, N.PSK_HOST, ctypes.byref(h)),
            "psk_sa_prolongator")
    P = psk.DeviceCSR._adopt(h, count)
    assert (P.n, P.ncols) == ref.shape
    _same(P.to_scipy(), ref)


def test_results_are_deterministic(psk, operands):
    A, B = operands["ints"]
    dA, dB = _dev(psk, A), _dev(psk, B)
    C1, C2 = psk.Linear.matmat(dA, dB).to_scipy(), psk.Linear.matmat(dA, dB).to_scipy()
    _same(C1, C2)
    _same(dA.transpose().to_scipy(), dA.transpose().to_scipy())


def test_matmat_takes_scipy_operands_and_feeds_spmv(psk, operands):
    """Linear.matmat uploads scipy operands itself, and its result is a matrix like any other: y = C x has the
    bits of scipy's csr_matvec on the downloaded arrays (the creation path's layout choice ran)."""
    A, B = operands["normal"]
    C = psk.Linear.matmat(A, B)
    x = np.random.default_rng(3).standard_normal(C.ncols)
    y = psk.Linear.spmv(C, x)
    assert np.array_equal(y.view(np.int64), (C.to_scipy() @ x).view(np.int64))


def test_more_rows_than_one_grid_dimension_holds(psk):
    """2^24 + 5 output rows, one wave each: 2^24 workgroups of 256 threads are the 2^32 threads a single grid
    dimension cannot hold (the launch is refused), so the row kernels lay their workgroups out in two dimensions.
    One entry per row keeps it to a few hundred MB and a second or two; both the product and the transpose whose
    RESULT has that many rows are checked against scipy."""
    n = (1 << 24) + 5
    rows = np.arange(n)
    A = sp.csr_matrix((1.0 + (rows % 7) * 0.25, (rows % 8).astype(np.int32), np.arange(n + 1, dtype=np.int32)),
                      shape=(n, 8))
    B = _random(np.random.default_rng(11), 8, 5, 0.7, False)
    _same(psk.Linear.matmat(A, B).to_scipy(), A @ B)
    W = sp.csr_matrix((A.data, (n - 1 - rows).astype(np.int32), np.arange(n + 1, dtype=np.int32)), shape=(n, n))
    _same(_dev(psk, W).transpose().to_scipy(), W.transpose().tocsr())   # a transpose with n rows as well
