"""GPU tests of the ILU(0) preconditioner factored on the device (psk_csr_ilu0 / psk_prec_create_ilu0, ilu0.hip;
pysolvers_amd.Linear.RightILU0 / LeftILU0, DeviceCSR.ilu0).

Bars (written here, not inferred):
* Factor: indptr, indices and the uint64 view of the values EQUAL those of tests/ilu0_oracle.py, the statement-by-
  statement restatement of the arithmetic include/psk.h defines; run to run, scipy vs DeviceCSR input, and every
  lanes-per-row geometry (PSK_ILU0_WIDTH) bitwise equal.
* Apply: max |psk_prec_apply(v) - apply(F)(v)| <= 1e-12 max |apply(F)(v)| under the planner's schedule and under
  every schedule that can be forced. The two differ only in the summation order of a row's products (at most 9 per
  row on five cases; rand511's 506-entry row is covered by the same bound relative to the result).
* GMRES: history within 1e-10 ||b|| of oracle.krylov.gmres with the oracle's ILU(0) apply (the project's solver-
  parity bar), equal iteration counts where no oracle history entry lies within a relative 1e-6 of tau ||b|| (all
  five cases qualify; asserted), true residual <= tau ||b|| computed on the host.
* Errors are error returns and leave no sticky state.

Cases: the smallest shapes that reach each way the kernels can go wrong —
  fd17     unsorted stored rows, 33 levels
  cd33     nonsymmetric values
  dh8/10   3 levels, 64 and 256 rows wide
  rand511  unsorted rows, a 506-entry row, 20 levels (16 lanes per row by the mean row length)
  fd300    599 levels up to 300 rows wide (a level spans workgroups), n = 90000 above the one-workgroup LDS
           triangular schedule's 18432 rows
"""
import functools
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import bicgstab_oracle as bo
import ilu0_oracle as io0
from conftest import GOLDEN
from oracle import fdlap, krylov

pytestmark = pytest.mark.gpu

TAU = 1e-10
MAXITER = 400
RTOL_APPLY = 1e-12
RTOL_RESID = 1e-10
CASES = ("fd17", "cd33", "dh8", "dh10", "rand511", "fd300")
SOLVER_CASES = ("fd17", "cd33", "dh8", "dh10", "rand511")
SCHEDULES = ("syncfree", "band", "lds", "grid", "part", "levels")


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
    if name == "cd33":
        return bo.cd_matrix(33, 0.5)
    if name.startswith("dh"):
        return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-%s.mtx" % name[2:])).tocsr()
    if name == "rand511":
        return bo.random_nonsym(511, seed=511)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle_factor(name):
    """The oracle's F: computed once, shared, never written to."""
    F = io0.ilu0(_matrix(name))
    F.data.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def _rhs(name):
    b = np.random.default_rng(3).standard_normal(_matrix(name).shape[0])
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _oracle_apply(name):
    y = io0.apply(_oracle_factor(name))(_rhs(name))
    y.setflags(write=False)
    return y


def _same_factor(F, ref):
    assert np.array_equal(F.indptr, ref.indptr)
    assert np.array_equal(F.indices, ref.indices)
    assert np.array_equal(_bits(F.data), _bits(ref.data))


def _ctl(psk, **kw):
    kw.setdefault("showIters", False)
    kw.setdefault("showFinal", False)
    kw.setdefault("maxiter", MAXITER)
    kw.setdefault("tau", TAU)
    return psk.CommonSolverArgs(**kw)


# ---- 1. the factor, bitwise --------------------------------------------------------------------------------------

def test_unsorted_cases_are_stored_unsorted():
    for name in ("fd17", "rand511", "fd300"):
        A = _matrix(name)
        ip = A.indptr
        assert any(np.any(np.diff(A.indices[ip[i]:ip[i + 1]]) < 0) for i in range(min(A.shape[0], 600))), name
    assert max(np.diff(_matrix("rand511").indptr)) == 506


@pytest.mark.parametrize("name", CASES)
def test_factor_bitwise_vs_oracle(psk, name):
    A, ref = _matrix(name), _oracle_factor(name)
    dA = psk.DeviceCSR.from_scipy(A)
    M = psk.RightILU0().form(A)
    _same_factor(M.factors(), ref)                       # the preconditioner object's F, scipy input
    F1 = dA.ilu0()
    assert isinstance(F1, psk.DeviceCSR) and F1.shape == A.shape and F1.nnz == A.nnz
    _same_factor(F1.to_scipy(), ref)                     # DeviceCSR.ilu0()
    _same_factor(dA.ilu0().to_scipy(), ref)              # a second run
    _same_factor(psk.RightILU0().form(dA).factors(), ref)   # DeviceCSR input
    info = M.device_info()
    assert info["kind"] == psk._native.PSK_PREC_ILU and info["n"] == A.shape[0]
    assert info["nnz_l"] + info["nnz_u"] + A.shape[0] == A.nnz   # strict lower + strict upper + the diagonal


@pytest.mark.parametrize("name", ["fd17", "rand511", "dh10"])
@pytest.mark.parametrize("width", [1, 4, 16, 64])
def test_factor_does_not_depend_on_the_launch_geometry(psk, name, width, monkeypatch):
    """1, 4, 16 or 64 lanes per row (the library picks by the mean row length): the same bits."""
    monkeypatch.setenv("PSK_ILU0_WIDTH", str(width))
    _same_factor(psk.DeviceCSR.from_scipy(_matrix(name)).ilu0().to_scipy(), _oracle_factor(name))


# ---- 2. the apply -------------------------------------------------------------------------------------------------

def _check_apply(name, y):
    ref = _oracle_apply(name)
    dev = np.max(np.abs(y - ref)) / np.max(np.abs(ref))
    print("%s: apply deviation %.3e max|oracle apply|" % (name, dev))
    assert np.all(np.isfinite(y))
    assert dev <= RTOL_APPLY, (name, dev)


@pytest.mark.parametrize("name", CASES)
def test_apply_vs_oracle(psk, name):
    M = psk.RightILU0().form(_matrix(name))
    print("%s: schedules L=%s U=%s" % (name, M.schedule("L")["schedule"], M.schedule("U")["schedule"]))
    y = M.applyRight(np.array(_rhs(name)))
    _check_apply(name, y)
    assert np.array_equal(_bits(M.applyRight(np.array(_rhs(name)))), _bits(y))                   # run to run
    yd = M.applyRight(psk.DeviceVector.from_numpy(np.array(_rhs(name)))).numpy()                 # device vector
    assert np.array_equal(_bits(yd), _bits(y))
    left = psk.LeftILU0().form(_matrix(name))
    v = np.array(_rhs(name))
    assert left.applyRight(v) is v                                                               # identity
    assert np.array_equal(_bits(left.applyLeft(v)), _bits(y))


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("name", CASES)
def test_apply_under_each_forced_schedule(psk, name, sched, monkeypatch):
    """The partitioned and levels layouts exist only when built at creation, so those two cases ask for them in the
    environment before form()."""
    if sched in ("part", "levels"):
        monkeypatch.setenv({"part": "PSK_TRISOLVE_PART", "levels": "PSK_TRISOLVE_LEVELS"}[sched], "1")
    M = psk.RightILU0().form(_matrix(name))
    forced = []
    for which in ("L", "U"):
        try:
            M.schedule(which, set=sched)
            forced.append(which)
        except Exception as e:   # grid: no grid plan; lds: too large for one workgroup; band: rows too long; ...
            why = str(e)
    if not forced:
        pytest.skip("schedule %s not available for %s: %s" % (sched, name, why))
    for which in forced:
        assert M.schedule(which)["schedule"] == sched
    _check_apply(name, M.applyRight(np.array(_rhs(name))))


# ---- 3. the solvers -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gmres_reference(name):
    r = krylov.gmres(_matrix(name), _rhs(name), maxiter=MAXITER, tau=TAU, precond=io0.apply(_oracle_factor(name)))
    r["hist"].setflags(write=False)
    return r


def _counts_comparable(ref, nb):
    th = TAU * nb
    return not np.any(np.abs(ref["hist"] - th) <= 1e-6 * th)


@pytest.mark.parametrize("name", SOLVER_CASES)
def test_gmres_matches_oracle(psk, name):
    A, b = _matrix(name), np.array(_rhs(name))
    ref = _gmres_reference(name)
    nb = np.linalg.norm(b)
    st = psk.GMRES(control=_ctl(psk), precond=psk.RightILU0()).makeSolver().solve(A, b)
    assert st.success() and ref["success"], st.msg()
    h, ho = st.info["hist"], ref["hist"]
    m = min(len(h), len(ho))
    dev = np.max(np.abs(h[:m] - ho[:m])) / nb
    print("%s: GMRES+ILU(0) iters %d (oracle %d), history deviation %.3e ||b||" % (name, st.iters(), ref["iters"], dev))
    assert dev <= RTOL_RESID, (name, dev)
    assert _counts_comparable(ref, nb), name            # every case takes part in the count comparison
    assert st.iters() == ref["iters"] and len(h) == len(ho)
    assert np.linalg.norm(b - A @ st.soln()) <= TAU * nb


def test_gmres_oracle_counts():
    """The CPU runs' iteration counts the device is compared with (recorded when the feature was written)."""
    assert [_gmres_reference(n)["iters"] for n in SOLVER_CASES] == [24, 27, 32, 66, 10]


def test_pcg_fd17(psk):
    """For a symmetric A the ILU(0) product L U is symmetric, so PCG may use it."""
    A, b = _matrix("fd17"), np.array(_rhs("fd17"))
    nb = np.linalg.norm(b)
    st = psk.PCG(control=_ctl(psk), precond=psk.RightILU0()).makeSolver().solve(A, b)
    sj = psk.PCG(control=_ctl(psk), precond=psk.Jacobi()).makeSolver().solve(A, b)
    print("PCG fd17: ILU(0) %d iterations, Jacobi %d" % (st.iters(), sj.iters()))
    assert st.success() and sj.success()
    assert np.linalg.norm(b - A @ st.soln()) <= TAU * nb
    assert st.iters() < sj.iters()


def test_bicgstab_cd33(psk):
    A, b = _matrix("cd33"), np.array(_rhs("cd33"))
    nb = np.linalg.norm(b)
    st = psk.BiCGStab(control=_ctl(psk), precond=psk.RightILU0()).makeSolver().solve(A, b)
    sj = psk.BiCGStab(control=_ctl(psk), precond=psk.Jacobi()).makeSolver().solve(A, b)
    print("BiCGStab cd33: ILU(0) %d iterations, Jacobi %d" % (st.iters(), sj.iters()))
    assert st.success() and sj.success()
    assert np.linalg.norm(b - A @ st.soln()) <= TAU * nb
    assert st.iters() < sj.iters()


# ---- 4. errors ----------------------------------------------------------------------------------------------------

def _csr(data, indices, indptr, shape):
    A = sp.csr_matrix((np.array(data, dtype=np.float64), np.array(indices, dtype=np.int32),
                       np.array(indptr, dtype=np.int32)), shape=shape)
    A.has_sorted_indices = False
    return A


BAD = {
    # name: (matrix, code, text in the message)
    "zero_pivot": (lambda: _csr([0.0, 1.0, 1.0, 0.0], [0, 1, 0, 1], [0, 2, 4], (2, 2)), -1, "row 0"),
    "pivot_cancels": (lambda: _csr([1.0, 1.0, 1.0, 1.0], [0, 1, 0, 1], [0, 2, 4], (2, 2)), -1, "row 1"),
    "no_diagonal": (lambda: _csr([2.0, 1.0, 1.0], [0, 1, 0], [0, 2, 3], (2, 2)), -1, "diagonal"),
    "duplicate": (lambda: _csr([2.0, 1.0, 1.0, 3.0], [0, 0, 0, 1], [0, 2, 4], (2, 2)), -5, "duplicate"),
    "rectangular": (lambda: _csr([2.0, 1.0, 1.0, 3.0], [0, 2, 0, 1], [0, 2, 4], (2, 3)), -1, "square"),
}


@pytest.mark.parametrize("kind", list(BAD))
def test_errors_are_returned_and_leave_no_state(psk, kind):
    from pysolvers_amd import _native as N
    assert (N.PSK_ERR_ARG, N.PSK_ERR_UNSUPPORTED) == (-1, -5)
    make, code, text = BAD[kind]
    dA = psk.DeviceCSR.from_scipy(make(), rectangular=True)
    with pytest.raises(N.PskError) as e:
        dA.ilu0()
    assert e.value.code == code and text in str(e.value), str(e.value)
    with pytest.raises(N.PskError) as e:
        psk.RightILU0().form(dA)
    assert e.value.code == code and text in str(e.value), str(e.value)
    # a valid form right after the error: nothing sticky is left behind
    _same_factor(psk.RightILU0().form(_matrix("fd17")).factors(), _oracle_factor("fd17"))


# ---- 5. Newton ----------------------------------------------------------------------------------------------------

def test_newton_bratu_with_gmres_ilu0_steps(psk):
    """FD-Bratu 32^2 (examples/FDBratu2D.py, the case of test_gpu_newton.py) with GMRES + RightILU0 steps and the
    preconditioner frozen: Newton succeeds and the final ||F|| meets its own stopping rule
    ||F|| <= tau ||F_0|| + tau (Newton.py:54), the converged-norm bar of the suite's other Newton runs."""
    from pysolvers_amd.Nonlinear import NewtonSolver
    from oracle import newton
    func = newton.Bratu2D(m=32)
    tau = 1.0e-12
    lin = psk.GMRES(control=psk.CommonSolverArgs(showIters=False, showFinal=False), precond=psk.RightILU0())
    ns = NewtonSolver(control=psk.CommonSolverArgs(tau=tau, maxiter=10, showIters=False, showFinal=False),
                      solver=lin, fixLinTol=False, minLinTol=1.0e-6, freezePrec=True)
    st = ns.solve(func, func.initialU())
    assert st.success(), st.msg()
    normF0 = np.linalg.norm(func.evalF(func.initialU()))
    assert np.linalg.norm(func.evalF(st.soln())) <= tau * normF0 + tau
    assert len(ns.linear_iters) == st.iters() - 1 and all(k >= 1 for k in ns.linear_iters)
