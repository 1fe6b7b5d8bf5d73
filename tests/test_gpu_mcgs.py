"""GPU tests of the multicolour Gauss-Seidel preconditioner and AMG smoother (psk_color_plan, psk_prec_create_mcgs,
mcgs.hip).

Bars (written here, not inferred):
* colouring, colour count and rows per colour against tests/mcgs_oracle.py: equal (integers).
* apply against the oracle: BITWISE, for 1 and 2 sweeps, with and without PSK_MCGS_SYMMETRIC, for host arrays,
  DeviceVector and CUDA tensors, handle to handle and apply after apply: both sides round every operation once in the
  same order (the row sum is the SpMV's; the update is one subtract, one multiply, one add).
* PCG / GMRES with it against oracle.krylov with the oracle operator: equal iteration counts, residual histories
  within RTOL_RESID = 1e-10 of ||b|| (the project's solver-parity bar; the dot products round differently), the
  solution within 1e-9 relative; PCG counts below the oracle's Jacobi count, and the counts the oracle records:
  -FD 64^2 89 (1 sweep) and 63 (2 sweeps) against Jacobi's 177, DH-10 52 against 103.
* MINRES with it on an SPD matrix: converged.
* one AMG apply (numIters 2, 3 levels, -FD 32^2) with MulticolorGaussSeidelSmoother against the V-cycle restated on the
  CPU with the oracle operator as S^-1: 1e-10 relative, the AMG tests' bar.
* PCG + AMG(numIters 5, 3 levels) on -FD 32^2 converges (five cycles, because the reference's V-cycle apply starts from
  x = copy(v) and is a usable PCG operator only once it is close to A^-1; the CPU restatement takes 4 iterations with
  this smoother and 4 with the reference's Gauss-Seidel). The two counts are printed side by side; no bar on which
  is lower.
"""
import ctypes
import functools

import numpy as np
import pytest

import cheby_oracle
import mcgs_oracle as mo
from mcgs_cases import matrix
from oracle import amg, krylov

from pysolvers_amd import _native as N
from pysolvers_amd.Linear import (AMGPreconditioner, Communicator, DeviceCSR, DeviceVector, GaussSeidelSmoother,
                                  MulticolorGS, MulticolorGSPreconditioner, MulticolorGaussSeidelSmoother,
                                  fd_laplacian_2d_sharded)

pytestmark = pytest.mark.gpu

RTOL_RESID = 1e-10
APPLY_CASES = ["negfd16", "negfd33", "dh8", "dh10", "nonsym", "one", "diag", "longrow", "shuffled"]


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _ctl(**kw):
    from pysolvers_amd import CommonSolverArgs
    kw.setdefault("showIters", False)
    kw.setdefault("showFinal", False)
    return CommonSolverArgs(**kw)


@functools.lru_cache(maxsize=None)
def _oracle(name, sweeps, symmetric):
    return mo.MCGS(matrix(name), sweeps, symmetric)


@functools.lru_cache(maxsize=None)
def _vector(name):
    v = np.random.default_rng(31).standard_normal(matrix(name).shape[0])
    if v.size > 2:
        v[1] = -0.0                                   # a signed zero must come out as the definition has it
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("name", APPLY_CASES)
def test_coloring_and_info_equal_the_oracle(name):
    A = matrix(name)
    ref = _oracle(name, 1, True)
    dA = DeviceCSR.from_scipy(A)
    color, nc = dA.coloring()
    assert nc == ref.ncolors and color.dtype == np.int32 and np.array_equal(color, ref.color)
    M = MulticolorGSPreconditioner(dA, sweeps=2, symmetric=False)
    assert M.ncolors == ref.ncolors and np.array_equal(M.color_rows, ref.color_rows)
    assert M.color_rows.dtype == np.int64 and M.color_rows.sum() == A.shape[0]
    c, s, f = N.I32(), N.I32(), N.I32()
    assert N.lib.psk_prec_mcgs_info(M.device_handle, ctypes.byref(c), ctypes.byref(s), ctypes.byref(f), None) == N.PSK_OK
    assert (c.value, s.value, f.value) == (ref.ncolors, 2, 0)
    info = M.device_info()
    assert info["kind"] == N.PSK_PREC_MCGS == 7 and info["n"] == A.shape[0]
    assert info["nnz_l"] == info["nnz_u"] == A.nnz and info["levels_l"] == info["levels_u"] == ref.ncolors


def test_colour_counts():
    for name, want in (("negfd16", 2), ("negfd33", 2), ("dh8", 3), ("dh10", 3), ("diag", 1), ("one", 1)):
        assert MulticolorGSPreconditioner(matrix(name)).ncolors == want, name


@pytest.mark.parametrize("name", APPLY_CASES)
@pytest.mark.parametrize("sweeps,symmetric", [(1, True), (2, True), (1, False), (2, False)])
def test_apply_is_bitwise_the_oracle(name, sweeps, symmetric):
    import torch
    A, v = matrix(name), _vector(name)
    y_ref = _oracle(name, sweeps, symmetric)(v)
    M = MulticolorGSPreconditioner(A, sweeps=sweeps, symmetric=symmetric)
    y = M.apply(v)
    assert np.array_equal(_bits(y), _bits(y_ref))
    yd = M.apply(DeviceVector.from_numpy(v))
    assert isinstance(yd, DeviceVector) and np.array_equal(_bits(yd.numpy()), _bits(y_ref))
    yt = M.apply(torch.from_numpy(np.array(v)).to("cuda"))
    assert yt.is_cuda and np.array_equal(_bits(yt.cpu().numpy()), _bits(y_ref))
    assert np.array_equal(_bits(M.applyLeft(v)), _bits(y_ref)) and np.array_equal(_bits(M.applyRight(v)), _bits(y_ref))
    assert np.array_equal(_bits(M.apply(v)), _bits(y))                   # two applies in a row


def test_long_row_spans_more_than_one_chunk():
    """The case that takes the kernel's chunk loop: one row longer than the 1280 products a workgroup stages at once."""
    A = matrix("longrow")
    assert np.diff(A.indptr).max() > 1280 and _oracle("longrow", 1, True).ncolors >= 3


@pytest.mark.parametrize("name,sweeps,symmetric", [("dh10", 2, True), ("nonsym", 1, False), ("negfd33", 1, True)])
def test_deterministic_and_stateless(name, sweeps, symmetric):
    """Two handles give the same bits; one handle applied to v, to another vector, and to v again gives v's bits
    again: nothing of an apply is left in the handle."""
    A, v = matrix(name), _vector(name)
    ref = _oracle(name, sweeps, symmetric)
    dA = DeviceCSR.from_scipy(A)
    M1 = MulticolorGSPreconditioner(dA, sweeps=sweeps, symmetric=symmetric)
    M2 = MulticolorGS(sweeps=sweeps, symmetric=symmetric).form(dA)
    assert isinstance(M2, MulticolorGSPreconditioner)
    y1 = M1.apply(v)
    assert np.array_equal(_bits(y1), _bits(M2.apply(v))) and np.array_equal(_bits(y1), _bits(ref(v)))
    w = np.random.default_rng(99).standard_normal(A.shape[0]) * 1e3
    assert np.array_equal(_bits(M1.apply(w)), _bits(ref(w)))
    assert np.array_equal(_bits(M1.apply(v)), _bits(y1))
    del dA                                            # the matrix is not borrowed
    assert np.array_equal(_bits(M1.apply(v)), _bits(y1))


def _create_rc(dA, sweeps=1, flags=N.PSK_MCGS_SYMMETRIC):
    h = ctypes.c_void_p()
    rc = N.lib.psk_prec_create_mcgs(dA.handle, sweeps, flags, ctypes.byref(h))
    if rc == N.PSK_OK:
        N.lib.psk_prec_destroy(h)
    else:
        assert not h.value                            # written only on success
    return rc, N.lib.psk_last_error().decode()


def test_refusals():
    import scipy.sparse as sp
    dA = DeviceCSR.from_scipy(matrix("negfd16"))
    assert _create_rc(dA)[0] == N.PSK_OK
    # a zero diagonal (stored), a missing one and one that is not finite: the smallest such row is named
    def with_diagonal(rows, value):
        B = matrix("negfd16").copy()
        for i in rows:
            e = B.indptr[i] + int(np.flatnonzero(B.indices[B.indptr[i]:B.indptr[i + 1]] == i)[0])
            B.data[e] = value
        return B

    stored = with_diagonal([200, 9], 0.0)
    assert stored.nnz == matrix("negfd16").nnz
    rc, msg = _create_rc(DeviceCSR.from_scipy(stored))
    assert rc == N.PSK_ERR_ARG and "row 9 " in msg
    missing = stored.copy()
    missing.eliminate_zeros()
    assert missing.nnz == stored.nnz - 2
    rc, msg = _create_rc(DeviceCSR.from_scipy(missing))
    assert rc == N.PSK_ERR_ARG and "row 9 " in msg
    rc, msg = _create_rc(DeviceCSR.from_scipy(with_diagonal([4], np.inf)))
    assert rc == N.PSK_ERR_ARG and "row 4 " in msg
    with pytest.raises(N.PskError) as e:
        MulticolorGSPreconditioner(stored)
    assert e.value.code == N.PSK_ERR_ARG
    # sweeps, flags, shape
    assert _create_rc(dA, sweeps=0)[0] == N.PSK_ERR_ARG
    assert _create_rc(dA, sweeps=-1)[0] == N.PSK_ERR_ARG
    assert _create_rc(dA, flags=2)[0] == N.PSK_ERR_ARG
    rect = DeviceCSR.from_scipy(sp.csr_matrix(np.array([[1.0, 2.0, 0.0], [0.0, 3.0, 4.0]])), rectangular=True)
    assert _create_rc(rect)[0] == N.PSK_ERR_ARG
    # more than 64 colours: a dense 70 x 70; the message names the count
    rc, msg = _create_rc(DeviceCSR.from_scipy(matrix("dense70")))
    assert rc == N.PSK_ERR_UNSUPPORTED and "70 colours" in msg
    with pytest.raises(N.PskError) as e:
        MulticolorGSPreconditioner(matrix("dense70"))
    assert e.value.code == N.PSK_ERR_UNSUPPORTED
    # the info call is for this kind only
    J = __import__("pysolvers_amd").JacobiPreconditioner(dA)
    assert N.lib.psk_prec_mcgs_info(J.device_handle, None, None, None, None) == N.PSK_ERR_ARG


def test_sharded_matrix_is_unsupported():
    comm = Communicator(1, 0, dry=True)
    try:
        A = fd_laplacian_2d_sharded(-1.0, 1.0, 8, comm)
        assert _create_rc(A)[0] == N.PSK_ERR_UNSUPPORTED
        with pytest.raises(N.PskError) as e:
            MulticolorGSPreconditioner(A)
        assert e.value.code == N.PSK_ERR_UNSUPPORTED
        del A
    finally:
        comm.destroy()


@functools.lru_cache(maxsize=None)
def _system(name):
    A = matrix(name)
    b = A @ np.random.default_rng(12345).random(A.shape[0])
    b.setflags(write=False)
    return A, b, krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=krylov.jacobi_form(A))["iters"]


@pytest.mark.parametrize("name,sweeps,expect", [("negfd64", 1, (89, 177)), ("negfd64", 2, (63, 177)),
                                                ("dh10", 1, (52, 103))])
def test_pcg_with_mcgs_matches_the_oracle(name, sweeps, expect):
    import pysolvers_amd as psk
    A, b, jac = _system(name)
    st = psk.PCG(control=_ctl(maxiter=1000, tau=1e-8), precond=psk.MulticolorGS(sweeps)).makeSolver().solve(A, b)
    ref = krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=_oracle(name, sweeps, True))
    nb = np.linalg.norm(b)
    n = min(len(st.info["hist"]), len(ref["hist"]))
    dev = np.max(np.abs(st.info["hist"][:n] - ref["hist"][:n])) / nb
    print("PCG+MulticolorGS(%d) %s: iters %d (oracle %d, Jacobi %d) hist dev %.3e" % (sweeps, name, st.iters(),
                                                                                     ref["iters"], jac, dev))
    assert st.success() and ref["success"] and st.iters() == ref["iters"] < jac
    assert (ref["iters"], jac) == expect
    assert len(st.info["hist"]) == len(ref["hist"]) and dev <= RTOL_RESID
    assert np.linalg.norm(st.soln() - ref["soln"]) <= 1e-9 * np.linalg.norm(ref["soln"])


@pytest.mark.parametrize("symmetric", [True, False])
def test_gmres_with_mcgs_matches_the_oracle(symmetric):
    import pysolvers_amd as psk
    A, b, _ = _system("negfd32")
    st = psk.GMRES(control=_ctl(maxiter=200, tau=1e-8), precond=psk.MulticolorGS(1, symmetric)).makeSolver().solve(A, b)
    ref = krylov.gmres(A, b, maxiter=200, tau=1e-8, precond=_oracle("negfd32", 1, symmetric))
    nb = np.linalg.norm(b)
    n = min(len(st.info["hist"]), len(ref["hist"]))
    dev = np.max(np.abs(st.info["hist"][:n] - ref["hist"][:n])) / nb
    print("GMRES+MulticolorGS(1, symmetric=%s) -FD 32^2: iters %d (oracle %d) hist dev %.3e"
          % (symmetric, st.iters(), ref["iters"], dev))
    assert st.success() and ref["success"] and st.iters() == ref["iters"]
    assert len(st.info["hist"]) == len(ref["hist"]) and dev <= RTOL_RESID
    assert np.linalg.norm(st.soln() - ref["soln"]) <= 1e-9 * np.linalg.norm(ref["soln"])


def test_minres_with_mcgs_converges():
    import pysolvers_amd as psk
    A, b, _ = _system("negfd32")
    st = psk.MINRES(_ctl(maxiter=1000, tau=1e-8), psk.MulticolorGS()).makeSolver().solve(A, b)
    sj = psk.MINRES(_ctl(maxiter=1000, tau=1e-8), psk.Jacobi()).makeSolver().solve(A, b)
    print("MINRES -FD 32^2: iters MulticolorGS(1) %d, Jacobi %d; status %r" % (st.iters(), sj.iters(),
                                                                             st.info.get("status")))
    assert st.success() and st.info["status"] == "converged" and sj.success()
    # the test was made in the M^-1 norm; sqrt(cond(M)) is the exact bound between it and the 2-norm (psk.h)
    op = _oracle("negfd32", 1, True)
    Minv = np.column_stack([op(e) for e in np.eye(A.shape[0])])
    ev = np.linalg.eigvalsh(0.5 * (Minv + Minv.T))
    assert ev[0] > 0.0
    assert np.linalg.norm(b - A @ st.soln()) <= np.sqrt(ev[-1] / ev[0]) * 1e-8 * np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def _negfd32():
    """(-FD 32^2, the oracle's 3-level hierarchy): built once."""
    A = matrix("negfd32").copy()                      # writable: the setup may sort rows in place
    return A, amg.hierarchy(A, 3)


@pytest.mark.parametrize("smoother,sweeps,symmetric", [(MulticolorGaussSeidelSmoother, 1, True),
                                                       (MulticolorGaussSeidelSmoother.of(sweeps=1, symmetric=False), 1, False)])
def test_amg_apply_with_multicolor_smoother(smoother, sweeps, symmetric):
    A, levels = _negfd32()
    v = np.random.default_rng(64).standard_normal(A.shape[0])
    M = AMGPreconditioner(A, numIters=2, numLevels=3, smoother=smoother)
    assert all(isinstance(s, MulticolorGaussSeidelSmoother) and isinstance(s.operator, MulticolorGSPreconditioner)
               and s.operator.sweeps == sweeps and s.operator.symmetric == symmetric for s in M._S[1:])
    S = [None] + [mo.MCGS(L, sweeps, symmetric) for L in levels[0][1:]]
    assert all(s.operator.ncolors == o.ncolors for s, o in zip(M._S[1:], S[1:]))
    y = M.apply(v)
    y_ref = cheby_oracle.amg_apply(A, levels, S, v, num_iters=2)
    rel = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
    print("AMG apply, multicolour GS smoother (symmetric=%s), -FD 32^2 L=3: rel %.3e" % (symmetric, rel))
    assert rel <= 1e-10
    assert np.array_equal(_bits(M.apply(v)), _bits(y))
    # the smoother's host-callable contract (x <- x + S^-1 (f - A x), nu sweeps) against the oracle's sweeps
    f, x0 = v[:levels[0][1].shape[0]], np.zeros(levels[0][1].shape[0])
    xs = M._S[1].apply(f, x0, 2)
    assert np.linalg.norm(xs - cheby_oracle.smooth(levels[0][1], S[1], f, x0, 2)) <= 1e-12 * np.linalg.norm(xs)


def test_pcg_with_amg_and_the_multicolor_smoother_converges():
    import pysolvers_amd as psk
    A, b, _ = _system("negfd32")
    A = A.copy()                                      # writable: the setup may sort rows in place
    its = {}
    for label, sm in (("multicolour", psk.MulticolorGaussSeidelSmoother), ("Gauss-Seidel", GaussSeidelSmoother)):
        st = psk.PCG(control=_ctl(maxiter=100, tau=1e-8),
                     precond=psk.AMG(numIters=5, numLevels=3, smoother=sm)).makeSolver().solve(A, b)
        assert st.success(), label
        assert np.linalg.norm(b - A @ st.soln()) <= 1e-7 * np.linalg.norm(b)
        its[label] = st.iters()
    print("PCG + AMG(numIters 5, 3 levels) -FD 32^2: iterations %r" % its)


def test_pcg_multi_refuses_it_and_solve_many_falls_back():
    import pysolvers_amd as psk
    A = matrix("negfd16")
    dA = DeviceCSR.from_scipy(A)
    M = MulticolorGSPreconditioner(dA)
    B = np.ascontiguousarray(np.random.default_rng(8).standard_normal((A.shape[0], 3)))
    X = np.empty_like(B)
    ctl = N.PskCtl(maxiter=50, tau=1e-8, fail_on_maxiter=1, restart=0, check_every=0, time_kernels=0, norm_b=0.0)
    res = (N.PskResult * 3)()
    rc = N.lib.psk_pcg_multi(dA.handle, M.device_handle, 3, N.ptr(B), N.ptr(X), ctypes.byref(ctl), res, None, N.PSK_HOST)
    assert rc == N.PSK_ERR_UNSUPPORTED and b"preconditioner" in N.lib.psk_last_error()
    c = _ctl(maxiter=300, tau=1e-10)
    sts = psk.PCG(control=c, precond=psk.MulticolorGS()).makeSolver().solveMany(A, B)
    assert len(sts) == 3
    for j, st in enumerate(sts):
        bj = np.ascontiguousarray(B[:, j])
        one = psk.PCG(control=c, precond=psk.MulticolorGS()).makeSolver().solve(A, bj)
        assert st.success() and st.iters() == one.iters()
        assert np.array_equal(_bits(st.soln()), _bits(one.soln()))       # the same code path, column by column
        assert np.linalg.norm(bj - A @ st.soln()) <= 1e-9 * np.linalg.norm(bj)
