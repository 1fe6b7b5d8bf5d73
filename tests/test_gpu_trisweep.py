"""GPU tests of the Jacobi-sweep triangular applies (psk_prec_trisolve_sweeps, trisolve_sweep.hip;
TriangularSolveChain.sweeps and the ``sweeps=`` keyword of the ILU / IC preconditioner types).

Bars (written here, not inferred):
* Apply: max |device - oracle| <= 1e-12 max |oracle| (RTOL_APPLY of test_gpu_ilu0.py) against tests/trisweep_oracle.py
  for s in {1, 2, 3, 7} with L only, U only and both factors swept. "L only" and "U only" are the mixed-mode cases:
  the other factor runs its exact schedule, which is what the sentinel-fill branches of the apply serve. The device
  and the oracle differ only in the summation order of a row's products.
* Nilpotency: with levels - 1 sweeps (levels from psk_prec_info) the swept apply is within the same bar of the same
  chain's exact apply.
* Determinism: swept applies are bitwise equal run to run; after set = 0 the apply is bitwise that of a fresh
  preconditioner; psk_prec_trisolve_schedule reports the same schedule before, during and after.
* Every lane width (PSK_TRISWEEP_WIDTH = 1, 4, 16, 64) stays within the apply bar.
* GMRES with RightILU0(sweeps=4): history within 1e-10 ||b|| (RTOL_RESID) of oracle.krylov.gmres driven by the oracle's
  swept apply; iteration counts equal where no oracle history entry lies within a relative 1e-6 of tau ||b||
  (test_gpu_ilu0.py's rule). PCG on fd17 and BiCGStab on cd33 converge to tau and take fewer iterations than Jacobi.
* AMG: a Gauss-Seidel smoother chain switched to 5 sweeps is honoured (the paired-sweep kernel steps aside): one
  apply within 1e-12 max of the oracle's cycle with the swept smoother.
* Errors return PSK_ERR_ARG and change neither the sweep counts nor the apply's bits.

Cases — the smallest shapes at which the kernel can go wrong (ILU(0) factors unless stated):
  fd17      289 rows stored unsorted, 33 levels, 1 lane per row
  cd33      nonsymmetric values
  dh8       irregular
  rand511   n no multiple of 64 or 256, uneven rows (a 506-entry row of A)
  dense300  a dense strict-lower random factor with its diagonal (non-unit L) and its transpose as a UNIT upper factor:
            rows of up to 299 entries, so 64 lanes per row and the chunk loop run, and mean and longest row disagree
  diag5     no off-diagonal entry at all
  n1        a single row
  ilut32    SuperLU ILUT chain of FD 32^2: gather_in and gather_out, unit L and non-unit U
  ic32      IC chain of -FD 32^2: L then L^T, both non-unit
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import bicgstab_oracle as bo
import cheby_oracle as co
import ilu0_oracle as io0
import trisweep_oracle as tso
from conftest import GOLDEN
from oracle import amg as oamg
from oracle import fdlap, krylov

pytestmark = pytest.mark.gpu

TAU = 1e-10
MAXITER = 400
RTOL_APPLY = 1e-12
RTOL_RESID = 1e-10
ILU0_CASES = ("fd17", "cd33", "dh8", "rand511", "diag5", "n1")
CASES = ILU0_CASES + ("dense300", "ilut32", "ic32")
SWEEPS = (1, 2, 3, 7)


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU visible to libpsk"
    return pysolvers_amd


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name.startswith("fd"):
        return fdlap.fd_laplacian_2d(-1.0, 1.0, int(name[2:])).tocsr()
    if name == "negfd32":
        return (-fdlap.fd_laplacian_2d(-1.0, 1.0, 32)).tocsr()
    if name == "cd33":
        return bo.cd_matrix(33, 0.5)
    if name == "dh8":
        return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr()
    if name == "rand511":
        return bo.random_nonsym(511, seed=511)
    if name == "diag5":
        return sp.diags([2.0, -3.0, 0.5, 7.0, 1.25]).tocsr()
    if name == "n1":
        return sp.csr_matrix(np.array([[4.0]]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ilu0_factor(name):
    F = io0.ilu0(_matrix(name))
    F.data.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def _dense300():
    """(L, U): L = strict-lower dense random + a diagonal in [1, 2), every off-diagonal row and column sum below 1;
    U = L^T, used as a unit factor."""
    n = 300
    rng = np.random.default_rng(300)
    S = np.tril(rng.uniform(-1.0, 1.0, size=(n, n)), k=-1) / n
    L = sp.csr_matrix(S + np.diag(1.0 + rng.random(n)))
    return L, sp.csr_matrix(L.T)


def _make(psk, name):
    """(device operator, oracle chain factory (s_l, s_u) -> callable) of a case. A fresh device operator per call."""
    from pysolvers_amd.Linear.TriangularSolve import TriangularSolveChain
    if name in ILU0_CASES:
        F = _ilu0_factor(name)
        return psk.RightILU0().form(_matrix(name)), lambda sl, su: tso.ilu0_chain(F, sl, su)
    if name == "dense300":
        L, U = _dense300()
        M = TriangularSolveChain(300, L=L, l_unit=False, U=U, u_unit=True)
        return M, lambda sl, su: tso.Chain(L=L, l_unit=False, U=U, u_unit=True, s_l=sl, s_u=su)
    if name == "ilut32":
        M = psk.RightILUT().form(_matrix("fd32"))
        return M, lambda sl, su: tso.superlu_chain(M.ILU(), sl, su)
    if name == "ic32":
        M = psk.RightIC().form(_matrix("negfd32"))
        return M, lambda sl, su: tso.Chain(L=M._L, U=M._Lt, s_l=sl, s_u=su)
    raise KeyError(name)


def _rhs(n):
    return np.random.default_rng(3).standard_normal(n)


def _apply(M, v):
    return M._device_apply(np.array(v))


def _set(M, sl, su):
    M.sweeps("L", sl)
    M.sweeps("U", su)
    assert (M.sweeps("L"), M.sweeps("U")) == (sl, su)


def _dev(y, ref):
    assert np.all(np.isfinite(y))
    return float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))


# ---- 1. the apply against the oracle: every s, L only / U only (mixed mode) / both --------------------------------

@pytest.mark.parametrize("name", CASES)
def test_apply_vs_oracle(psk, name):
    M, oracle = _make(psk, name)
    v = _rhs(M.n)
    assert (M.sweeps("L"), M.sweeps("U")) == (0, 0)          # nothing sweeps unless asked
    worst = 0.0
    for s in SWEEPS:
        for sl, su in ((s, 0), (0, s), (s, s)):
            _set(M, sl, su)
            d = _dev(_apply(M, v), oracle(sl, su)(v))
            print("%s: sweeps L=%d U=%d deviation %.3e max|oracle|" % (name, sl, su, d))
            worst = max(worst, d)
            assert d <= RTOL_APPLY, (name, sl, su, d)
    _set(M, 0, 0)
    d = _dev(_apply(M, v), oracle(0, 0)(v))                    # and the exact apply is still the exact apply
    assert d <= RTOL_APPLY, (name, d)
    print("%s: worst swept deviation %.3e" % (name, worst))


def test_cases_have_the_shapes_they_are_chosen_for(psk):
    A = _matrix("fd17")
    ip = A.indptr
    assert any(np.any(np.diff(A.indices[ip[i]:ip[i + 1]]) < 0) for i in range(A.shape[0]))   # stored unsorted
    assert _matrix("rand511").shape[0] % 64 != 0 and max(np.diff(_matrix("rand511").indptr)) == 506
    L, _ = _dense300()
    assert max(np.diff(L.indptr)) == 300 and L.nnz == 300 * 301 // 2
    M, _ = _make(psk, "fd17")
    assert M.device_info()["levels_l"] == 33 and M.device_info()["levels_u"] == 33
    M, _ = _make(psk, "diag5")
    assert M.device_info()["nnz_l"] == 0 and M.device_info()["nnz_u"] == 0


# ---- 2. nilpotency: levels - 1 sweeps are the exact solve ---------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_levels_minus_one_sweeps_equal_the_exact_apply(psk, name):
    M, _ = _make(psk, name)
    v = _rhs(M.n)
    exact = _apply(M, v)
    info = M.device_info()
    sl, su = max(int(info["levels_l"]) - 1, 1), max(int(info["levels_u"]) - 1, 1)
    _set(M, sl, su)
    d = _dev(_apply(M, v), exact)
    print("%s: %d / %d sweeps (levels %d / %d) vs the exact apply %.3e max" % (name, sl, su, info["levels_l"],
                                                                             info["levels_u"], d))
    assert d <= RTOL_APPLY, (name, d)


# ---- 3. determinism and no residue --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fd17", "rand511", "ilut32"])
def test_deterministic_and_set_zero_leaves_no_residue(psk, name):
    M, _ = _make(psk, name)
    fresh, _ = _make(psk, name)
    v = _rhs(M.n)
    before = (M.schedule("L"), M.schedule("U"))
    y_exact = _apply(M, v)
    _set(M, 3, 2)
    during = (M.schedule("L"), M.schedule("U"))
    y1, y2 = _apply(M, v), _apply(M, v)
    assert np.array_equal(_bits(y1), _bits(y2))                 # run to run
    assert not np.array_equal(_bits(y1), _bits(y_exact))        # and it is another operator
    _set(M, 0, 0)
    after = (M.schedule("L"), M.schedule("U"))
    assert before == during == after
    y_back = _apply(M, v)
    assert np.array_equal(_bits(y_back), _bits(_apply(fresh, v)))
    assert np.array_equal(_bits(y_back), _bits(y_exact))
    yd = M._device_apply(psk.DeviceVector.from_numpy(np.array(v))).numpy()
    assert np.array_equal(_bits(yd), _bits(y_exact))


# ---- 4. every lane width ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rand511", "dense300"])
@pytest.mark.parametrize("width", [1, 4, 16, 64])
def test_every_lane_width(psk, name, width, monkeypatch):
    """PSK_TRISWEEP_WIDTH is read when the sweep count is set."""
    M, oracle = _make(psk, name)
    v = _rhs(M.n)
    monkeypatch.setenv("PSK_TRISWEEP_WIDTH", str(width))
    _set(M, 3, 3)
    monkeypatch.delenv("PSK_TRISWEEP_WIDTH")
    d = _dev(_apply(M, v), oracle(3, 3)(v))
    print("%s: %d lanes per row, deviation %.3e max|oracle|" % (name, width, d))
    assert d <= RTOL_APPLY, (name, width, d)


# ---- 5. the solvers -----------------------------------------------------------------------------------------------

def _ctl(psk, **kw):
    kw.setdefault("showIters", False)
    kw.setdefault("showFinal", False)
    kw.setdefault("maxiter", MAXITER)
    kw.setdefault("tau", TAU)
    return psk.CommonSolverArgs(**kw)


@pytest.mark.parametrize("name", ["fd17", "cd33", "dh8", "rand511"])
def test_gmres_with_swept_ilu0_matches_oracle(psk, name):
    A, b = _matrix(name), _rhs(_matrix(name).shape[0])
    nb = np.linalg.norm(b)
    ref = krylov.gmres(A, b, maxiter=MAXITER, tau=TAU, precond=tso.ilu0_chain(_ilu0_factor(name), 4, 4))
    st = psk.GMRES(control=_ctl(psk), precond=psk.RightILU0(sweeps=4)).makeSolver().solve(A, b)
    assert st.success() and ref["success"], st.msg()
    h, ho = st.info["hist"], ref["hist"]
    m = min(len(h), len(ho))
    dev = np.max(np.abs(h[:m] - ho[:m])) / nb
    print("%s: GMRES + ILU(0) with 4 sweeps: iters %d (oracle %d), history deviation %.3e ||b||"
          % (name, st.iters(), ref["iters"], dev))
    assert dev <= RTOL_RESID, (name, dev)
    th = TAU * nb
    if not np.any(np.abs(ho - th) <= 1e-6 * th):
        assert st.iters() == ref["iters"] and len(h) == len(ho)
    assert np.linalg.norm(b - A @ st.soln()) <= TAU * nb


def test_pcg_fd17_with_swept_ilu0(psk):
    """Equal sweep counts keep the chain symmetric for a symmetric A (test_trisweep_cpu.py), so PCG may use it."""
    A, b = _matrix("fd17"), _rhs(289)
    nb = np.linalg.norm(b)
    st = psk.PCG(control=_ctl(psk), precond=psk.RightILU0(sweeps=4)).makeSolver().solve(A, b)
    sj = psk.PCG(control=_ctl(psk), precond=psk.Jacobi()).makeSolver().solve(A, b)
    print("PCG fd17: ILU(0) with 4 sweeps %d iterations, Jacobi %d" % (st.iters(), sj.iters()))
    assert st.success() and sj.success()
    assert np.linalg.norm(b - A @ st.soln()) <= TAU * nb
    assert st.iters() < sj.iters()


def test_bicgstab_cd33_with_swept_ilu0(psk):
    A, b = _matrix("cd33"), _rhs(1089)
    nb = np.linalg.norm(b)
    st = psk.BiCGStab(control=_ctl(psk), precond=psk.RightILU0(sweeps=4)).makeSolver().solve(A, b)
    sj = psk.BiCGStab(control=_ctl(psk), precond=psk.Jacobi()).makeSolver().solve(A, b)
    print("BiCGStab cd33: ILU(0) with 4 sweeps %d iterations, Jacobi %d" % (st.iters(), sj.iters()))
    assert st.success() and sj.success()
    assert np.linalg.norm(b - A @ st.soln()) <= TAU * nb
    assert st.iters() < sj.iters()


def test_keyword_forms(psk):
    A, v = _matrix("cd33"), _rhs(1089)
    F = _ilu0_factor("cd33")
    mixed = psk.RightILU0(sweeps=(0, 3)).form(A)
    assert (mixed.sweeps("L"), mixed.sweeps("U")) == (0, 3)
    y = mixed.applyRight(np.array(v))
    assert _dev(y, tso.ilu0_chain(F, 0, 3)(v)) <= RTOL_APPLY
    both = psk.RightILU0(sweeps=3).form(A)
    assert (both.sweeps("L"), both.sweeps("U")) == (3, 3)
    exact = psk.RightILU0().form(A)
    assert (exact.sweeps("L"), exact.sweeps("U")) == (0, 0)
    assert not np.array_equal(_bits(y), _bits(both.applyRight(np.array(v))))
    assert not np.array_equal(_bits(y), _bits(exact.applyRight(np.array(v))))
    left = psk.LeftILU0(sweeps=3).form(A)
    assert np.array_equal(_bits(left.applyLeft(np.array(v))), _bits(both.applyRight(np.array(v))))
    ic = psk.RightIC(sweeps=(2, 0)).form(_matrix("negfd32"))
    assert (ic.sweeps("L"), ic.sweeps("U")) == (2, 0)
    ilut = psk.RightILUT(sweeps=5).form(_matrix("fd32"))
    assert (ilut.sweeps("L"), ilut.sweeps("U")) == (5, 5)
    st = psk.GMRES(control=_ctl(psk), precond=psk.RightILU0(sweeps=(0, 3))).makeSolver().solve(A, np.array(v))
    assert st.success(), st.msg()


# ---- 6. the AMG smoother's x += S^-1 r path ------------------------------------------------------------------------

def test_amg_gauss_seidel_smoother_in_sweep_mode(psk):
    from pysolvers_amd import _native as N
    A = _matrix("negfd32")
    v = _rhs(A.shape[0])
    M = psk.AMG(numIters=2, numLevels=2).form(A)
    on, el = ctypes.c_int32(), ctypes.c_int32()
    N.check(N.load_lab().psk_lab_amg_gs_pair(M.device_handle, -1, ctypes.byref(on), ctypes.byref(el)), "gs_pair")
    assert (on.value, el.value) == (1, 1)                     # the level would run the paired kernel
    y_gs = M.applyRight(np.array(v))
    S = M._S[1].operator
    assert S.sweeps("U", 5) == 5
    y = M.applyRight(np.array(v))
    levels = oamg.hierarchy(A, 2)
    U = sp.triu(levels[0][1]).tocsr()
    ref = co.amg_apply(A, levels, [None, lambda r: tso.sweep_solve(U, r, 5)], v, num_iters=2)
    d = _dev(y, ref)
    print("AMG negfd32, smoother with 5 sweeps: deviation %.3e max|oracle|; against Gauss-Seidel %.3e"
          % (d, _dev(y_gs, ref)))
    assert d <= RTOL_APPLY, d
    assert not np.array_equal(_bits(y), _bits(y_gs))
    assert S.sweeps("U", 0) == 0
    assert np.array_equal(_bits(M.applyRight(np.array(v))), _bits(y_gs))   # and the pair is back


# ---- 7. errors ----------------------------------------------------------------------------------------------------

def test_errors_change_nothing(psk):
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear.TriangularSolve import TriangularSolveChain
    assert N.PSK_ERR_ARG == -1
    M, _ = _make(psk, "fd17")
    v = _rhs(M.n)
    _set(M, 2, 3)
    y = _apply(M, v)
    out = N.I32(77)
    fn = N.lib.psk_prec_trisolve_sweeps
    gs = TriangularSolveChain(289, U=sp.triu(_matrix("fd17")).tocsr(), u_unit=False)      # no L factor
    jac = psk.Jacobi().form(_matrix("fd17"))
    bad = {
        "which": (M.device_handle, 2, 4),
        "which_negative": (M.device_handle, -1, 4),
        "absent_factor": (gs.device_handle, 0, 4),
        "jacobi_handle": (jac.device_handle, 0, 4),
        "null_handle": (None, 0, 4),
        "set_minus_2": (M.device_handle, 0, -2),
        "set_65537": (M.device_handle, 1, 65537),
    }
    for what, (h, which, set_) in bad.items():
        assert fn(h, which, set_, ctypes.byref(out)) == N.PSK_ERR_ARG, what
        assert out.value == 77, what                             # not written on error
        assert (M.sweeps("L"), M.sweeps("U")) == (2, 3), what
        assert gs.sweeps("U") == 0
    assert np.array_equal(_bits(_apply(M, v)), _bits(y))
    with pytest.raises(N.PskError) as e:
        M.sweeps("L", 65537)
    assert e.value.code == N.PSK_ERR_ARG
    assert fn(M.device_handle, 0, 65536, None) == N.PSK_OK       # the largest count is accepted (not applied here)
    assert M.sweeps("L", 2) == 2
    assert np.array_equal(_bits(_apply(M, v)), _bits(y))
