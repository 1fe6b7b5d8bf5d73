"""GPU tests of the factorized sparse approximate inverse (psk_csr_fsai, psk_prec_create_fsai, fsai.hip).

Bars (written here, not inferred):
* G against tests/fsai_oracle.py: BITWISE (indptr, indices, the bits of the values) and the same sign: both sides
  round every operation once, in the same order; the f64 device sqrt and division are IEEE (correctly rounded).
* The one-lane-per-row kernel against the wave-per-row kernel (PSK_FSAI_WAVE_ONLY): bitwise.
* apply against the oracle's (sign G^T)(G v): bitwise (two SpMVs under the SpMV's contract), for host arrays,
  DeviceVector and CUDA tensors, handle to handle and apply after apply.
* PCG / GMRES with it against oracle.krylov with the oracle operator: equal iteration counts, residual histories
  within RTOL_RESID = 1e-10 of ||b|| (the project's solver-parity bar; the dot products round differently), the
  solution within 1e-9 relative; PCG counts below the oracle's Jacobi count, and on -FD 64^2 the counts the numpy
  prototype of this arithmetic gave: 94 (power 1) and 67 (power 2) against Jacobi's 177.
* MINRES with it on an SPD matrix: converged, in fewer iterations than MINRES with Jacobi.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import fsai_oracle as fo
from conftest import GOLDEN
from oracle import fdlap, krylov

from pysolvers_amd import _native as N
from pysolvers_amd.Linear import (Communicator, DeviceCSR, DeviceVector, FSAI, FSAIPreconditioner,
                                  fd_laplacian_2d_sharded, matmat)

pytestmark = pytest.mark.gpu

RTOL_RESID = 1e-10
BAND_N = 300


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _ctl(**kw):
    from pysolvers_amd import CommonSolverArgs
    kw.setdefault("showIters", False)
    kw.setdefault("showFinal", False)
    return CommonSolverArgs(**kw)


def _banded(sub, n=BAND_N, seed=63):
    """Symmetric, strictly diagonally dominant with a positive diagonal (so SPD), exactly `sub` sub-diagonals, every
    entry inside the band stored: row i's lower part has min(i, sub) + 1 entries. Columns shuffled inside every row."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n))
    for k in range(1, sub + 1):
        v = rng.uniform(0.1, 1.0, size=n - k) * rng.choice([-1.0, 1.0], size=n - k)
        D += np.diag(v, -k) + np.diag(v, k)
    D += np.diag(np.abs(D).sum(axis=1) + 1.0 + rng.random(n))
    A = sp.csr_matrix(D)
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
    if name.startswith("negfd"):
        return (-fdlap.fd_laplacian_2d(-1.0, 1.0, int(name[5:]))).tocsr()
    if name.startswith("fd"):
        return fdlap.fd_laplacian_2d(-1.0, 1.0, int(name[2:])).tocsr()
    if name in ("dh8", "dh10"):
        return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-%s.mtx" % name[2:])).tocsr()
    if name == "one":
        return sp.csr_matrix(np.array([[2.5]]))
    if name == "negone":
        return sp.csr_matrix(np.array([[-2.5]]))
    if name == "band63":
        return _banded(63)
    if name == "band64":
        return _banded(64)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle(name, power):
    """The oracle operator (G, sign, apply): computed once, shared, never written to."""
    op = fo.FSAI(_matrix(name), power=power)
    op.G.data.setflags(write=False)
    return op


@functools.lru_cache(maxsize=None)
def _vector(name):
    return np.random.default_rng(len(name) + 17).standard_normal(_matrix(name).shape[0])


def _same_matrix(G, ref):
    S = G.to_scipy()
    return (np.array_equal(S.indptr, ref.indptr) and np.array_equal(S.indices, ref.indices)
            and np.array_equal(_bits(S.data), _bits(ref.data)))


# (matrix, power): the longest row m of G and the numeric kernel it takes
CASES = [("negfd8", 1), ("negfd8", 2), ("fd17", 1), ("fd17", 2), ("dh8", 1), ("dh8", 2), ("dh10", 2), ("one", 1),
         ("negone", 1), ("band63", 1)]
MAX_ROW = {("negfd8", 1): 3, ("negfd8", 2): 7, ("fd17", 1): 3, ("fd17", 2): 7, ("dh8", 1): 5, ("dh8", 2): 21,
           ("dh10", 2): 21, ("one", 1): 1, ("negone", 1): 1, ("band63", 1): 64}


def test_the_matrices_have_the_shapes_the_kernel_paths_need():
    for key, m in MAX_ROW.items():
        assert _oracle(*key).max_row == m, key
    A = _matrix("band63")
    low = np.diff(sp.tril(A).tocsr().indptr)
    assert np.array_equal(low, np.minimum(np.arange(BAND_N), 63) + 1)              # m = 1..64 all occur
    assert set(low) == set(range(1, 65)) and N.PSK_FSAI_ROW_CAP == 64
    ip = A.indptr
    assert all(np.any(np.diff(A.indices[ip[i]:ip[i + 1]]) < 0) for i in range(70, 80))   # unsorted rows
    assert abs(A - A.T).max() == 0.0
    assert np.max(np.diff(sp.tril(_matrix("band64")).tocsr().indptr)) == 65
    assert _oracle("fd17", 1).sign == -1 and _oracle("negone", 1).sign == -1 and _oracle("negfd8", 1).sign == 1


@pytest.mark.parametrize("name,power", CASES)
def test_g_is_bitwise_the_oracle(name, power):
    A = _matrix(name)
    ref = _oracle(name, power)
    dA = DeviceCSR.from_scipy(A)
    G, sign = dA.fsai(pattern=matmat(dA, dA) if power == 2 else None)
    assert sign == ref.sign
    S = G.to_scipy()
    assert np.array_equal(S.indptr, ref.G.indptr) and np.array_equal(S.indices, ref.G.indices)
    same = _bits(S.data) == _bits(ref.G.data)
    if not same.all():
        bad = np.flatnonzero(~same)
        print("%s power %d: %d of %d values differ, first at entry %d: %r vs %r" % (
            name, power, bad.size, same.size, bad[0], S.data[bad[0]], ref.G.data[bad[0]]))
    assert same.all()
    # the general kernel gives the same bits whatever kernel the library chose
    Gw, sw = dA.fsai(pattern=matmat(dA, dA) if power == 2 else None, flags=N.PSK_FSAI_WAVE_ONLY)
    assert sw == sign and _same_matrix(Gw, ref.G)


@pytest.mark.parametrize("name", ["negfd8", "fd17"])
def test_small_row_kernel_equals_general_kernel(name):
    dA = DeviceCSR.from_scipy(_matrix(name))
    assert _oracle(name, 1).max_row <= 4          # flags 0 takes the one-lane-per-row kernel
    G0, s0 = dA.fsai()
    G1, s1 = dA.fsai(flags=N.PSK_FSAI_WAVE_ONLY)
    assert s0 == s1 and _same_matrix(G0, G1.to_scipy())
    # and a device-generated stencil (diagonal SpMV layout, rows as the generator stores them) gives them too
    if name == "fd17":
        Gd, sd = DeviceCSR.fd_laplacian_2d(-1.0, 1.0, 17).fsai()
        assert sd == s0 == -1 and _same_matrix(Gd, G0.to_scipy())


@pytest.mark.parametrize("name,power", [("negfd8", 1), ("fd17", 1), ("fd17", 2), ("dh8", 1), ("dh10", 2), ("one", 1),
                                        ("negone", 1), ("band63", 1)])
def test_apply_is_bitwise_the_oracle(name, power):
    import torch
    A, v = _matrix(name), _vector(name)
    ref = _oracle(name, power)
    y_ref = ref(v)
    M = FSAIPreconditioner(A, power=power)
    info = M.device_info()
    assert info["kind"] == N.PSK_PREC_FSAI and info["n"] == A.shape[0]
    assert info["nnz_l"] == info["nnz_u"] == ref.nnz and info["levels_l"] == info["levels_u"] == 0
    assert (M.sign, M.nnz, M.max_row) == (ref.sign, ref.nnz, ref.max_row)
    y = M.apply(v)
    assert np.array_equal(_bits(y), _bits(y_ref))
    yd = M.apply(DeviceVector.from_numpy(v))
    assert isinstance(yd, DeviceVector) and np.array_equal(_bits(yd.numpy()), _bits(y_ref))
    yt = M.apply(torch.from_numpy(v).to("cuda"))
    assert yt.is_cuda and np.array_equal(_bits(yt.cpu().numpy()), _bits(y_ref))
    assert np.array_equal(_bits(M.applyLeft(v)), _bits(y_ref)) and np.array_equal(_bits(M.applyRight(v)), _bits(y_ref))
    # the same bits as two psk_spmv calls on the factor and its signed transpose
    dG = DeviceCSR.from_scipy(ref.G)
    dGt = DeviceCSR.from_scipy(ref.Gt)
    from pysolvers_amd.Linear import spmv
    assert np.array_equal(_bits(spmv(dGt, spmv(dG, v))), _bits(y))


@pytest.mark.parametrize("name,power", [("dh8", 2), ("fd17", 1), ("band63", 1)])
def test_deterministic_and_stateless(name, power):
    """Two handles give the same bits; one handle applied to v, to another vector, and to v again gives v's bits
    again: nothing of an apply is left in the work vector."""
    A, v = _matrix(name), _vector(name)
    ref = _oracle(name, power)
    dA = DeviceCSR.from_scipy(A)
    M1, M2 = FSAIPreconditioner(dA, power=power), FSAI(power=power).form(dA)
    assert isinstance(M2, FSAIPreconditioner)
    y1 = M1.apply(v)
    assert np.array_equal(_bits(y1), _bits(M2.apply(v))) and np.array_equal(_bits(y1), _bits(ref(v)))
    w = np.random.default_rng(99).standard_normal(A.shape[0]) * 1e3
    assert np.array_equal(_bits(M1.apply(w)), _bits(ref(w)))
    assert np.array_equal(_bits(M1.apply(v)), _bits(y1))


def test_explicit_patterns():
    """A pattern with entries outside A's pattern (those B entries are 0.0) and one holding upper entries (ignored):
    both bitwise the oracle, for both signs."""
    for name in ("negfd8", "fd17"):
        A = _matrix(name)
        n = A.shape[0]
        rng = np.random.default_rng(n)
        extra = sp.random(n, n, density=6.0 / n, random_state=rng, format="csr")
        wide = (abs(A) + abs(extra) + abs(extra.T) + sp.identity(n)).tocsr()      # upper entries too
        assert (wide - wide.multiply(abs(A) > 0)).nnz > 0                          # entries outside A's pattern
        assert sp.triu(wide, k=1).nnz > 0
        ref, sref = fo.fsai(A, wide)
        assert 4 < np.max(np.diff(ref.indptr)) <= 64
        dA = DeviceCSR.from_scipy(A)
        G, sign = dA.fsai(pattern=DeviceCSR.from_scipy(wide))
        assert sign == sref and _same_matrix(G, ref)
        # the lower triangle alone is the same pattern
        G2, _ = dA.fsai(pattern=sp.tril(wide).tocsr())
        assert _same_matrix(G2, ref)
        # upper entries added to A's own pattern change nothing
        G3, _ = dA.fsai(pattern=DeviceCSR.from_scipy((sp.tril(A) + sp.triu(wide, k=1)).tocsr()))
        assert _same_matrix(G3, _oracle(name, 1).G)


def _fsai_rc(dA, pattern=None, flags=0):
    h, s = ctypes.c_void_p(), N.I32(77)
    rc = N.lib.psk_csr_fsai(dA.handle, None if pattern is None else pattern.handle, flags, ctypes.byref(h),
                            ctypes.byref(s))
    if rc == N.PSK_OK:
        N.lib.psk_csr_destroy(h)
    else:
        assert not h.value and s.value == 77          # written only on success
    return rc, N.lib.psk_last_error().decode()


def test_refusals():
    A = _matrix("negfd8")
    n = A.shape[0]
    dA = DeviceCSR.from_scipy(A)
    assert _fsai_rc(dA)[0] == N.PSK_OK
    # a pattern row without its diagonal
    P = A.tolil()
    P[5, 5] = 0.0
    P = P.tocsr()
    P.eliminate_zeros()
    rc, msg = _fsai_rc(dA, DeviceCSR.from_scipy(P))
    assert rc == N.PSK_ERR_ARG and "row 5" in msg
    # over the cap: the smallest such row is named
    rc, msg = _fsai_rc(DeviceCSR.from_scipy(_matrix("band64")))
    assert rc == N.PSK_ERR_UNSUPPORTED and "row 64" in msg
    with pytest.raises(N.PskError) as e:
        FSAIPreconditioner(_matrix("band64"))
    assert e.value.code == N.PSK_ERR_UNSUPPORTED
    # a duplicate column, in A and in the pattern
    dup = sp.csr_matrix((np.array([2.0, 1.0, 1.0, 3.0]), np.array([0, 0, 0, 1]), np.array([0, 2, 4])), shape=(2, 2))
    dup.has_canonical_format = False
    ddup = DeviceCSR.from_scipy(dup)
    assert ddup.nnz == 4
    assert _fsai_rc(ddup)[0] == N.PSK_ERR_UNSUPPORTED
    two = DeviceCSR.from_scipy(sp.csr_matrix(np.array([[2.0, 1.0], [1.0, 3.0]])))
    assert _fsai_rc(two, ddup)[0] == N.PSK_ERR_UNSUPPORTED
    # rectangular, a pattern of another size, an unknown flag
    rect = DeviceCSR.from_scipy(sp.csr_matrix(np.array([[1.0, 2.0, 0.0], [0.0, 3.0, 4.0]])), rectangular=True)
    assert _fsai_rc(rect)[0] == N.PSK_ERR_ARG
    assert _fsai_rc(dA, two)[0] == N.PSK_ERR_ARG
    assert _fsai_rc(dA, None, 2)[0] == N.PSK_ERR_ARG
    # indefinite: -FD 8^2 shifted so that a pivot fails; the oracle names the same row
    # (3 in units of the stencil's off-diagonal entry: the diagonal stays positive, the 2 x 2 block of row 1 is singular)
    shift = (A - 3.0 * abs(A[0, 1]) * sp.identity(n)).tocsr()
    assert np.linalg.eigvalsh(shift.toarray()).min() < 0.0 < shift.diagonal().min()
    with pytest.raises(fo.PivotError) as pe:
        fo.fsai(shift)
    rc, msg = _fsai_rc(DeviceCSR.from_scipy(shift))
    assert rc == N.PSK_ERR_ARG and "not positive definite" in msg and ("row %d " % pe.value.row) in msg
    rc, msg = _fsai_rc(DeviceCSR.from_scipy(shift), None, N.PSK_FSAI_WAVE_ONLY)
    assert rc == N.PSK_ERR_ARG and ("row %d " % pe.value.row) in msg
    # diag(1, -1): the sign comes from row 0
    assert _fsai_rc(DeviceCSR.from_scipy(sp.csr_matrix(np.diag([1.0, -1.0]))))[0] == N.PSK_ERR_ARG
    # row 0 without a diagonal entry: no sign
    nod = sp.csr_matrix((np.array([1.0, 1.0, 2.0]), np.array([1, 0, 1]), np.array([0, 1, 3])), shape=(2, 2))
    assert _fsai_rc(DeviceCSR.from_scipy(nod))[0] == N.PSK_ERR_ARG
    # the info call is for this kind only
    J = __import__("pysolvers_amd").JacobiPreconditioner(dA)
    assert N.lib.psk_prec_fsai_info(J.device_handle, None, None, None) == N.PSK_ERR_ARG
    with pytest.raises(ValueError):
        FSAIPreconditioner(dA, power=3)


def test_sharded_matrix_is_unsupported():
    comm = Communicator(1, 0, dry=True)
    try:
        A = fd_laplacian_2d_sharded(-1.0, 1.0, 8, comm)
        assert _fsai_rc(A)[0] == N.PSK_ERR_UNSUPPORTED
        h = ctypes.c_void_p()
        assert N.lib.psk_prec_create_fsai(A.handle, None, 0, ctypes.byref(h)) == N.PSK_ERR_UNSUPPORTED
        with pytest.raises(N.PskError) as e:
            FSAIPreconditioner(A)
        assert e.value.code == N.PSK_ERR_UNSUPPORTED
        del A
    finally:
        comm.destroy()


@functools.lru_cache(maxsize=None)
def _system(name):
    A = _matrix(name)
    b = A @ np.random.default_rng(12345).random(A.shape[0])
    b.setflags(write=False)
    return A, b, krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=krylov.jacobi_form(A))["iters"]


@pytest.mark.parametrize("name,power,expect", [("negfd64", 1, (94, 177)), ("negfd64", 2, (67, 177)), ("dh10", 1, None)])
def test_pcg_with_fsai_matches_the_oracle(name, power, expect):
    import pysolvers_amd as psk
    A, b, jac = _system(name)
    st = psk.PCG(control=_ctl(maxiter=1000, tau=1e-8), precond=psk.FSAI(power)).makeSolver().solve(A, b)
    ref = krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=_oracle(name, power))
    nb = np.linalg.norm(b)
    n = min(len(st.info["hist"]), len(ref["hist"]))
    dev = np.max(np.abs(st.info["hist"][:n] - ref["hist"][:n])) / nb
    print("PCG+FSAI(%d) %s: iters %d (oracle %d, Jacobi %d) hist dev %.3e" % (power, name, st.iters(), ref["iters"],
                                                                            jac, dev))
    assert st.success() and ref["success"] and st.iters() == ref["iters"] < jac
    if expect is not None:
        assert (ref["iters"], jac) == expect
    assert len(st.info["hist"]) == len(ref["hist"]) and dev <= RTOL_RESID
    assert np.linalg.norm(st.soln() - ref["soln"]) <= 1e-9 * np.linalg.norm(ref["soln"])


def test_gmres_with_fsai_matches_the_oracle():
    import pysolvers_amd as psk
    A, b, _ = _system("negfd32")
    st = psk.GMRES(control=_ctl(maxiter=200, tau=1e-8), precond=psk.FSAI()).makeSolver().solve(A, b)
    ref = krylov.gmres(A, b, maxiter=200, tau=1e-8, precond=_oracle("negfd32", 1))
    nb = np.linalg.norm(b)
    n = min(len(st.info["hist"]), len(ref["hist"]))
    dev = np.max(np.abs(st.info["hist"][:n] - ref["hist"][:n])) / nb
    print("GMRES+FSAI(1) -FD 32^2: iters %d (oracle %d) hist dev %.3e" % (st.iters(), ref["iters"], dev))
    assert st.success() and ref["success"] and st.iters() == ref["iters"]
    assert len(st.info["hist"]) == len(ref["hist"]) and dev <= RTOL_RESID


def test_minres_with_fsai_converges_faster_than_with_jacobi():
    import pysolvers_amd as psk
    A, b, _ = _system("negfd32")
    st = psk.MINRES(_ctl(maxiter=1000, tau=1e-8), psk.FSAI()).makeSolver().solve(A, b)
    sj = psk.MINRES(_ctl(maxiter=1000, tau=1e-8), psk.Jacobi()).makeSolver().solve(A, b)
    print("MINRES -FD 32^2: iters FSAI(1) %d, Jacobi %d; status %r" % (st.iters(), sj.iters(), st.info.get("status")))
    assert st.success() and sj.success() and st.iters() < sj.iters()
    assert st.info["status"] == "converged" and sj.info["status"] == "converged"
    # the test was made in the M^-1 norm; sqrt(cond(M)) is the exact bound between it and the 2-norm (psk.h)
    Gd = _oracle("negfd32", 1).G.toarray()
    ev = np.linalg.eigvalsh(Gd.T @ Gd)
    assert np.linalg.norm(b - A @ st.soln()) <= np.sqrt(ev[-1] / ev[0]) * 1e-8 * np.linalg.norm(b)
