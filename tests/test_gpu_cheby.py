"""GPU tests of the Chebyshev polynomial preconditioner and AMG smoother (psk_prec_create_chebyshev, cheby.hip).

Bars (written here, not inferred):
* apply against tests/cheby_oracle.py: BITWISE (np.array_equal on the bits), and so are lmax, lmin and every
  coefficient the info call returns: both sides round every operation once, in the same order, with the row sums in
  stored order from 0.0 and rounded products (the SpMV's contract).
* PCG / GMRES with it against oracle.krylov with the oracle operator: equal iteration counts, residual histories
  within RTOL_RESID = 1e-10 of ||b|| (the project's solver-parity bar; the dot products round differently).
* one AMG apply with ChebyshevSmoother against the V-cycle restated with the oracle operator as S^-1: 1e-12 relative
  (the bar the existing AMG tests give the dense coarse solve, the only part that rounds differently).
* run to run, apply after apply, and host / DeviceVector / CUDA-tensor inputs: bitwise.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import cheby_oracle
from conftest import GOLDEN
from oracle import amg, fdlap, krylov

from pysolvers_amd import _native as N
from pysolvers_amd.Linear import (AMGPreconditioner, AMGVCycleSolver, Chebyshev, ChebyshevPreconditioner,
                                  ChebyshevSmoother, Communicator, DeviceCSR, DeviceVector, GaussSeidelSmoother,
                                  fd_laplacian_2d_sharded)

pytestmark = pytest.mark.gpu

RTOL_RESID = 1e-10
LONG_ROW = 500        # row of the random matrix that is full: its tile's entries exceed one LDS chunk (1280)


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _ctl(**kw):
    from pysolvers_amd import CommonSolverArgs
    kw.setdefault("showIters", False)
    kw.setdefault("showFinal", False)
    return CommonSolverArgs(**kw)


def _random_spd(n=1100, seed=7):
    """Symmetric, strictly diagonally dominant with a positive diagonal (so SPD), 1 to about 40 entries per row
    (rows 0..4 hold their diagonal alone), row LONG_ROW holding every column from 5 on (with its tile more than one
    1280-entry chunk, the row itself crossing the chunk boundary), columns shuffled inside every row."""
    rng = np.random.default_rng(seed)
    per = rng.integers(0, 16, size=n)
    per[:5] = 0
    rows = np.repeat(np.arange(n), per)
    cols = rng.integers(5, n, size=rows.shape[0])
    keep = rows != cols
    S = sp.coo_matrix((rng.standard_normal(keep.sum()), (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    full = sp.coo_matrix((rng.standard_normal(n - 5), (np.full(n - 5, LONG_ROW), np.arange(5, n))),
                         shape=(n, n)).tocsr()
    S = S + full
    S = (S + S.T).tolil()
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


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name == "fd17":
        return fdlap.fd_laplacian_2d(-1.0, 1.0, 17).tocsr()
    if name == "negfd17":
        return (-fdlap.fd_laplacian_2d(-1.0, 1.0, 17)).tocsr()
    if name == "dh8":
        return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr()
    if name == "rand":
        return _random_spd()
    if name == "one":
        return sp.csr_matrix(np.array([[-2.5]]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _vector(name):
    return np.random.default_rng(len(name) + 17).standard_normal(_matrix(name).shape[0])


@functools.lru_cache(maxsize=None)
def _reference(name, degree):
    """(oracle operator, its output for _vector(name)): computed once, shared, never written to."""
    op = cheby_oracle.Chebyshev(_matrix(name), degree=degree)
    y = op(_vector(name))
    y.setflags(write=False)
    return op, y


def test_random_matrix_has_the_shape_the_kernel_paths_need():
    A = _matrix("rand").copy()
    per = np.diff(A.indptr)
    assert per.min() == 1 and per[LONG_ROW] == A.shape[0] - 5 > 1024
    assert np.sort(per)[-2] <= 48 and np.median(per) <= 40
    assert any(np.any(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) < 0) for i in range(10, 40))   # unsorted
    assert abs(A - A.T).max() == 0.0 and np.linalg.eigvalsh(A.toarray()).min() > 0.0
    # rows per SpMV tile (psk::tile_rows_for): the long row's tile holds more than one 1280-entry chunk, and
    # the row itself lies across the chunk boundary
    r, avg = 256, A.nnz / A.shape[0]
    while r > 32 and avg * r > 1280:
        r >>= 1
    t0 = LONG_ROW // r * r
    e0 = A.indptr[t0]
    assert A.indptr[min(t0 + r, A.shape[0])] - e0 > 1280
    assert A.indptr[LONG_ROW] - e0 < 1280 < A.indptr[LONG_ROW + 1] - e0


@pytest.mark.parametrize("name", ["fd17", "negfd17", "dh8", "rand", "one"])
@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5])
def test_apply_is_bitwise_the_oracle(name, degree):
    import torch
    A, v = _matrix(name), _vector(name)
    op, y_ref = _reference(name, degree)
    dA = DeviceCSR.from_scipy(A)
    M = ChebyshevPreconditioner(dA, degree=degree)
    assert M.degree == degree
    assert M.device_info()["kind"] == N.PSK_PREC_CHEBYSHEV and M.device_info()["n"] == A.shape[0]
    assert M.lmax == op.lmax and M.lmin == op.lmin
    assert np.array_equal(_bits(M.coefficients), _bits(op.coefficients))
    y = M.apply(v)
    assert np.array_equal(_bits(y), _bits(y_ref))
    yd = M.apply(DeviceVector.from_numpy(v))
    assert isinstance(yd, DeviceVector) and np.array_equal(_bits(yd.numpy()), _bits(y_ref))
    yt = M.apply(torch.from_numpy(v).to("cuda"))
    assert yt.is_cuda and np.array_equal(_bits(yt.cpu().numpy()), _bits(y_ref))
    assert np.array_equal(_bits(M.applyLeft(v)), _bits(y_ref)) and np.array_equal(_bits(M.applyRight(v)), _bits(y_ref))


@pytest.mark.parametrize("name,degree", [("rand", 4), ("fd17", 3)])
def test_callers_lmax_and_ratio_are_honoured(name, degree):
    A, v = _matrix(name), _vector(name)
    op = cheby_oracle.Chebyshev(A, degree=degree, lmax=1.625, ratio=12.0)
    M = Chebyshev(degree=degree, lmax=1.625, ratio=12.0).form(A)
    assert isinstance(M, ChebyshevPreconditioner)
    assert M.lmax == 1.625 and M.lmin == 1.625 / 12.0 == op.lmin
    assert np.array_equal(_bits(M.coefficients), _bits(op.coefficients))
    assert np.array_equal(_bits(M.apply(v)), _bits(op(v)))
    assert not np.array_equal(_bits(M.apply(v)), _bits(_reference(name, degree)[1]))   # not the Gershgorin one


def _create_rc(dA, degree, lmax, ratio):
    h = ctypes.c_void_p()
    rc = N.lib.psk_prec_create_chebyshev(dA.handle, degree, lmax, ratio, ctypes.byref(h))
    if rc == N.PSK_OK:
        N.lib.psk_prec_destroy(h)
    return rc


def test_bad_arguments_are_refused():
    dA = DeviceCSR.from_scipy(_matrix("fd17"))
    assert _create_rc(dA, 2, 0.0, 30.0) == N.PSK_OK
    assert _create_rc(dA, 0, 0.0, 30.0) == N.PSK_ERR_ARG
    assert _create_rc(dA, -3, 0.0, 30.0) == N.PSK_ERR_ARG
    assert _create_rc(dA, 2, 0.0, 1.0) == N.PSK_ERR_ARG
    assert _create_rc(dA, 2, 0.0, 0.5) == N.PSK_ERR_ARG
    assert _create_rc(dA, 2, float("nan"), 30.0) == N.PSK_ERR_ARG
    rect = DeviceCSR.from_scipy(sp.csr_matrix(np.array([[1.0, 2.0, 0.0], [0.0, 3.0, 4.0]])), rectangular=True)
    assert _create_rc(rect, 2, 0.0, 30.0) == N.PSK_ERR_ARG
    nodiag = DeviceCSR.from_scipy(sp.csr_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 2.0]])))
    assert _create_rc(nodiag, 2, 0.0, 30.0) == N.PSK_ERR_ARG
    assert _create_rc(nodiag, 2, 1.5, 30.0) == N.PSK_ERR_ARG          # whatever the bound
    with pytest.raises(N.PskError) as e:
        ChebyshevPreconditioner(dA, degree=0)
    assert e.value.code == N.PSK_ERR_ARG
    # the info call is for this kind only
    J = __import__("pysolvers_amd").JacobiPreconditioner(dA)
    assert N.lib.psk_prec_chebyshev_info(J.device_handle, None, None, None, None) == N.PSK_ERR_ARG


def test_sharded_matrix_is_unsupported():
    comm = Communicator(1, 0, dry=True)
    try:
        A = fd_laplacian_2d_sharded(-1.0, 1.0, 8, comm)
        assert _create_rc(A, 2, 0.0, 30.0) == N.PSK_ERR_UNSUPPORTED
        with pytest.raises(N.PskError) as e:
            ChebyshevPreconditioner(A)
        assert e.value.code == N.PSK_ERR_UNSUPPORTED
        del A
    finally:
        comm.destroy()


@pytest.mark.parametrize("name,degree", [("rand", 5), ("dh8", 3), ("negfd17", 2)])
def test_deterministic_and_stateless(name, degree):
    """Two handles give the same bits; one handle applied to v, to another vector, and to v again gives v's bits
    again: nothing of an apply is left in d or the z buffers."""
    A, v = _matrix(name), _vector(name)
    _, y_ref = _reference(name, degree)
    dA = DeviceCSR.from_scipy(A)
    M1, M2 = ChebyshevPreconditioner(dA, degree=degree), ChebyshevPreconditioner(dA, degree=degree)
    y1 = M1.apply(v)
    assert np.array_equal(_bits(y1), _bits(M2.apply(v))) and np.array_equal(_bits(y1), _bits(y_ref))
    assert np.array_equal(_bits(M1.apply(v)), _bits(y1))
    w = np.random.default_rng(99).standard_normal(A.shape[0]) * 1e3
    yw = M1.apply(w)
    assert np.array_equal(_bits(yw), _bits(cheby_oracle.Chebyshev(A, degree=degree)(w)))
    assert np.array_equal(_bits(M1.apply(v)), _bits(y1))


def test_pcg_with_chebyshev3_matches_the_oracle():
    import pysolvers_amd as psk
    m = 64
    A = fdlap.fd_laplacian_2d(-1.0, 1.0, m).tocsr()
    b = A @ np.random.default_rng(12345).random(m * m)
    st = psk.PCG(control=_ctl(maxiter=500, tau=1e-8), precond=psk.Chebyshev(3)).makeSolver().solve(A, b)
    ref = krylov.pcg(A, b, maxiter=500, tau=1e-8, precond=cheby_oracle.Chebyshev(A, degree=3))
    jac = krylov.pcg(A, b, maxiter=500, tau=1e-8, precond=krylov.jacobi_form(A))
    nb = np.linalg.norm(b)
    dev = np.max(np.abs(st.info["hist"] - ref["hist"])) / nb
    print("PCG+Chebyshev(3) FD 64^2: iters %d (oracle %d, Jacobi %d) hist dev %.3e" % (st.iters(), ref["iters"],
                                                                                      jac["iters"], dev))
    assert st.success() and ref["success"] and st.iters() == ref["iters"] < jac["iters"]
    assert len(st.info["hist"]) == len(ref["hist"]) and dev <= RTOL_RESID
    assert np.linalg.norm(st.soln() - ref["soln"]) <= 1e-9 * np.linalg.norm(ref["soln"])


def test_gmres_with_chebyshev2_matches_the_oracle():
    import pysolvers_amd as psk
    m = 32
    A = fdlap.fd_laplacian_2d(-1.0, 1.0, m).tocsr()
    b = A @ np.random.default_rng(12345).random(m * m)
    st = psk.GMRES(control=_ctl(maxiter=200, tau=1e-8), precond=psk.Chebyshev(2)).makeSolver().solve(A, b)
    ref = krylov.gmres(A, b, maxiter=200, tau=1e-8, precond=cheby_oracle.Chebyshev(A, degree=2))
    nb = np.linalg.norm(b)
    dev = np.max(np.abs(st.info["hist"] - ref["hist"])) / nb
    print("GMRES+Chebyshev(2) FD 32^2: iters %d (oracle %d) hist dev %.3e" % (st.iters(), ref["iters"], dev))
    assert st.success() and ref["success"] and st.iters() == ref["iters"]
    assert len(st.info["hist"]) == len(ref["hist"]) and dev <= RTOL_RESID


@functools.lru_cache(maxsize=None)
def _negfd64():
    """(-FD 64^2, the oracle's 3-level hierarchy): built once."""
    A = (-fdlap.fd_laplacian_2d(-1.0, 1.0, 64)).tocsr()
    return A, amg.hierarchy(A, 3)


@pytest.mark.parametrize("smoother,degree", [(ChebyshevSmoother, 2), (ChebyshevSmoother.of(degree=3), 3)])
def test_amg_apply_with_chebyshev_smoother(smoother, degree):
    A, levels = _negfd64()
    v = np.random.default_rng(64).standard_normal(A.shape[0])
    M = AMGPreconditioner(A, numIters=2, numLevels=3, smoother=smoother)
    assert all(isinstance(s, ChebyshevSmoother) and isinstance(s.operator, ChebyshevPreconditioner)
               and s.operator.degree == degree for s in M._S[1:])
    S = cheby_oracle.level_smoothers(levels[0], degree=degree)
    # (the level matrices are the oracle's up to the order of a row's entries, so to an ulp or two)
    assert all(abs(s.operator.lmax - o.lmax) <= 1e-14 * o.lmax for s, o in zip(M._S[1:], S[1:]))
    y = M.apply(v)
    y_ref = cheby_oracle.amg_apply(A, levels, S, v, num_iters=2)
    rel = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
    print("AMG apply, Chebyshev degree %d smoother, -FD 64^2 L=3: rel %.3e" % (degree, rel))
    assert rel <= 1e-12
    assert np.array_equal(_bits(M.apply(v)), _bits(y))
    # the smoother's host-callable contract (x <- x + S^-1 (f - A x), nu sweeps) against the oracle's sweeps
    f, x0 = v[:levels[0][1].shape[0]], np.zeros(levels[0][1].shape[0])
    xs = M._S[1].apply(f, x0, 2)
    assert np.linalg.norm(xs - cheby_oracle.smooth(levels[0][1], S[1], f, x0, 2)) <= 1e-12 * np.linalg.norm(xs)


def test_amg_factory_takes_the_smoother():
    """AMG(...) hands the smoother class through: the same operator as AMGPreconditioner built directly, and PCG
    runs with it inside the device loop (a fixed number of iterations, the protocol of tools/bench_amg.py: PCG with
    the reference's V-cycle apply, which starts from x = copy(v), does not converge on this matrix with any
    smoother), its history equal to the oracle loop's within RTOL_RESID."""
    import pysolvers_amd as psk
    A, levels = _negfd64()
    M = psk.AMG(numIters=2, numLevels=3, smoother=psk.ChebyshevSmoother).form(A)
    assert all(type(s) is ChebyshevSmoother for s in M._S[1:])
    v = np.random.default_rng(64).standard_normal(A.shape[0])
    D = AMGPreconditioner(A, numIters=2, numLevels=3, smoother=ChebyshevSmoother, coarse_refine=0)   # AMG()'s default
    assert np.array_equal(_bits(M.apply(v)), _bits(D.apply(v)))
    b = A @ np.random.default_rng(5).random(A.shape[0])
    st = psk.PCG(control=_ctl(maxiter=6, tau=0.0, failOnMaxiter=False),
                 precond=psk.AMG(numIters=2, numLevels=3, smoother=psk.ChebyshevSmoother)).makeSolver().solve(A, b)
    S = cheby_oracle.level_smoothers(levels[0], degree=2)
    ref = krylov.pcg(A, b, maxiter=6, tau=0.0, fail_on_maxiter=False,
                     precond=lambda r: cheby_oracle.amg_apply(A, levels, S, r, num_iters=2))
    dev = np.max(np.abs(st.info["hist"] - ref["hist"])) / np.linalg.norm(b)
    print("PCG+AMG(Chebyshev 2) -FD 64^2, 6 iterations: hist dev %.3e" % dev)
    assert st.iters() == ref["iters"] == 6 and len(st.info["hist"]) == 6 and dev <= RTOL_RESID


def test_vcycle_solver_with_chebyshev_smoother_converges_like_the_oracle_loop():
    A, levels = _negfd64()
    b = A @ np.random.default_rng(12345).random(A.shape[0])
    S3 = ChebyshevSmoother.of(degree=3)
    st = AMGVCycleSolver(_ctl(maxiter=100, tau=1e-8), numLevels=3, smoother=S3).solve(A, b)
    ref = cheby_oracle.vcycle_solve(A, levels, cheby_oracle.level_smoothers(levels[0], degree=3), b, maxiter=100,
                                    tau=1e-8)
    print("AMGVCycle Chebyshev(3) -FD 64^2 L=3: cycles %d (oracle %d)" % (st.iters(), ref["iters"]))
    assert st.success() and ref["converged"] and st.iters() == ref["iters"]
    assert np.linalg.norm(b - A @ st.soln()) < 1e-8 * np.linalg.norm(b)
    assert np.max(np.abs(st.info["hist"] - ref["hist"])) <= RTOL_RESID * np.linalg.norm(b)
    import pysolvers_amd as psk
    st2 = psk.AMGVCycle(_ctl(maxiter=100, tau=1e-8), numLevels=3, smoother=S3).makeSolver().solve(A, b)
    assert st2.iters() == st.iters() and np.array_equal(_bits(st2.soln()), _bits(st.soln()))


def test_gauss_seidel_smoother_is_unchanged():
    """The default smoother takes the path it took: a triangular-solve chain per level (PSK_PREC_ILU), the same
    bits whether the smoother is named or left to the default, and the reference's apply within the AMG bar
    (1e-10, test_gpu_amg.py)."""
    from pysolvers_amd.Linear import TriangularSolveChain
    A, levels = _negfd64()
    v = np.random.default_rng(3).standard_normal(A.shape[0])
    M0 = AMGPreconditioner(A, numIters=2, numLevels=3)
    M1 = AMGPreconditioner(A, numIters=2, numLevels=3, smoother=GaussSeidelSmoother)
    for M in (M0, M1):
        assert all(type(s) is GaussSeidelSmoother and isinstance(s.operator, TriangularSolveChain) for s in M._S[1:])
        assert all(s.operator.device_info()["kind"] == N.PSK_PREC_ILU for s in M._S[1:])
    y0, y1 = M0.apply(v), M1.apply(v)
    assert np.array_equal(_bits(y0), _bits(y1))
    y_ref = amg.AMGApply(A, num_iters=2, num_levels=3, smoother="gs", levels=levels)(v)
    assert np.linalg.norm(y0 - y_ref) <= 1e-10 * np.linalg.norm(y_ref)
