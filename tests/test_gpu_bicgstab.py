"""GPU tests of the device-resident BiCGStab solver (psk_bicgstab, bicgstab.hip; pysolvers_amd.Linear.BiCGStab).

Bars (written here, not inferred):
* Residual history against tests/bicgstab_oracle.py: |h_dev[k] - h_oracle[k]| <= RTOL_RESID ||b|| = 1e-10 ||b|| (the
  project's solver-parity bar) for k in the PREFIX on which the oracle's own three dot-product orders (np.dot,
  math.fsum, 512-element chunks) agree within 2e-11 ||b||. The device performs the oracle's operations in the
  oracle's order, only its dot products sum in another order (gridsum), and BiCGStab amplifies that rounding: past
  the prefix even two CPU summation orders part by up to 1e-2 ||b||, so nothing can be asserted there. 1e-10 is
  5x the 2e-11 cap. A case takes part only with a prefix of >= 10 iterations, or with a prefix that is the three
  CPU runs' whole history (the strongly preconditioned cases converge, all orders alike, in fewer than 10); the
  test asserts it, so a case cannot drop out silently.
* Equal iteration counts only where the three CPU runs agree on them and no oracle history entry lies within a
  relative 1e-6 of tau ||b|| (bicgstab_oracle.counts_comparable).
* True residual ||b - A x|| <= tau ||b||, computed on the host with scipy: the solver's own stopping rule.
* Run to run, and host / DeviceVector / CUDA-tensor right-hand sides: bitwise.
"""
import functools
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import bicgstab_oracle as bo
import cheby_oracle
from conftest import GOLDEN
from oracle import fdlap, krylov

pytestmark = pytest.mark.gpu

RTOL_RESID = 1e-10
TAU = 1e-10
MAXITER = 1000


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU visible to libpsk"
    return pysolvers_amd


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _ctl(psk, **kw):
    kw.setdefault("showIters", False)
    kw.setdefault("showFinal", False)
    kw.setdefault("maxiter", MAXITER)
    kw.setdefault("tau", TAU)
    return psk.CommonSolverArgs(**kw)


# name -> (matrix, preconditioner); the right-hand side is seeded by the name
@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name.startswith("cd"):
        m = int(name[2:4])
        return bo.cd_matrix(m, {17: 0.3, 33: 0.5, 64: 0.2}[m])
    if name == "dh8":
        return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr()
    if name.startswith("fd17"):
        return fdlap.fd_laplacian_2d(-1.0, 1.0, 17).tocsr()
    if name.startswith("rand"):
        n = int(name[4:])
        return bo.random_nonsym(n, seed=7 if n == 1100 else n)
    raise KeyError(name)


CASES = {"cd17": "jacobi", "cd33": "jacobi", "cd64": "jacobi", "dh8": "jacobi", "cd17_id": "identity",
         "rand1100": "jacobi", "rand511": "jacobi", "rand512": "jacobi", "rand513": "jacobi", "rand1025": "jacobi",
         "cd33_ilut": "ilut", "fd17_cheb": "cheb"}


@functools.lru_cache(maxsize=None)
def _rhs(name):
    b = np.random.default_rng(len(name) + 17).standard_normal(_matrix(name).shape[0])
    b.setflags(write=False)
    return b


def _oracle_prec(name):
    A = _matrix(name)
    return {"jacobi": lambda: krylov.jacobi_form(A), "identity": lambda: bo.identity,
            "ilut": lambda: krylov.ilut_form(A), "cheb": lambda: cheby_oracle.Chebyshev(A, degree=3)}[CASES[name]]()


def _device_prec(psk, name):
    return {"jacobi": psk.JacobiPreconditionerType, "identity": psk.IdentityPreconditionerType,
            "ilut": psk.RightILUT, "cheb": lambda: psk.Chebyshev(degree=3)}[CASES[name]]()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(the oracle under its three dot orders, the agreeing prefix): computed once, shared, never written to."""
    res, prefix = bo.spread(_matrix(name), _rhs(name), M=_oracle_prec(name), tau=TAU, maxiter=MAXITER)
    for r in res:
        r["hist"].setflags(write=False)
    return res, prefix


def _solve(psk, name, A=None, b=None, **ctl):
    solver = psk.BiCGStab(control=_ctl(psk, **ctl), precond=_device_prec(psk, name)).makeSolver()
    return solver.solve(_matrix(name) if A is None else A, _rhs(name) if b is None else b)


def _check_prefix_parity(name, st):
    res, prefix = _reference(name)
    whole = all(len(r["hist"]) == prefix for r in res)
    assert prefix >= 10 or whole, (name, prefix, [len(r["hist"]) for r in res])
    if CASES[name] in ("jacobi", "identity") and not name.startswith("rand"):
        assert prefix >= 10, (name, prefix)                     # the table cases of the bar above
    nb = np.linalg.norm(_rhs(name))
    h, ho = st.info["hist"], res[0]["hist"]
    assert len(h) >= prefix, (name, len(h), prefix)
    dev = np.max(np.abs(h[:prefix] - ho[:prefix])) / nb
    print("%s: prefix %d of %d, history deviation %.3e ||b||, iters %d (oracle %s)"
          % (name, prefix, len(ho), dev, st.iters(), [r["iters"] for r in res]))
    assert dev <= RTOL_RESID, (name, dev)
    assert st.success(), (name, st.msg())
    if bo.counts_comparable(res, TAU):
        assert st.iters() == res[0]["iters"], (name, st.iters(), res[0]["iters"])


def _check_true_residual(name, st):
    A, b = _matrix(name), _rhs(name)
    assert np.linalg.norm(b - A @ st.soln()) <= TAU * np.linalg.norm(b)


def test_random_matrix_has_the_shape_the_kernel_paths_need():
    A = _matrix("rand1100").copy()       # scipy's arithmetic sorts its operand's rows in place
    per = np.diff(A.indptr)
    assert per.min() == 1 and per[bo.LONG_ROW] == A.shape[0] - 5 > 1024
    assert any(np.any(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) < 0) for i in range(10, 40))   # unsorted
    assert abs(A - A.T).max() > 0.0                                                     # nonsymmetric
    off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(A.diagonal())
    assert np.all(A.diagonal() > off)                                                   # strictly diagonally dominant
    r, avg = 256, A.nnz / A.shape[0]                     # rows per SpMV tile (psk::tile_rows_for)
    while r > 32 and avg * r > 1280:
        r >>= 1
    t0 = bo.LONG_ROW // r * r
    assert A.indptr[min(t0 + r, A.shape[0])] - A.indptr[t0] > 1280                      # a multi-chunk tile


@pytest.mark.parametrize("name", ["cd17", "cd33", "cd64", "dh8", "cd17_id", "rand1100"])
def test_prefix_parity_with_the_oracle(psk, name):
    st = _solve(psk, name)
    _check_prefix_parity(name, st)
    assert st.info["status"] == "converged" and len(st.info["hist"]) == st.iters()
    assert st.resid() <= TAU * st.info["norm_b"]                     # the true residual the device measured
    assert st.info["spmv_launches"] in (2 * st.iters(), 2 * st.iters() + 1)   # 2 per iteration (1 in a half step) + 1


@pytest.mark.parametrize("name", ["cd17", "cd33", "cd64"])
def test_every_spmv_layout_gives_the_same_solve(psk, name):
    """The cd operators admit every layout (constant diagonals, 5 distinct values); forced as
    tests/test_gpu_layout.py forces them. Each meets the oracle on the prefix."""
    dA = psk.DeviceCSR.from_scipy(_matrix(name))
    for lay in ("diag", "csr", "sliced", "sliced_wide", "sliced_dict"):
        dA.set_layout(lay)
        assert dA.layout == lay
        _check_prefix_parity(name, _solve(psk, name, A=dA))


@pytest.mark.parametrize("name", ["rand511", "rand512", "rand513", "rand1025"])
def test_vector_tile_edges(psk, name):
    """One 512-element tile minus one, exactly one, one plus one (a tile of a single element), two plus one."""
    st = _solve(psk, name)
    _check_prefix_parity(name, st)
    _check_true_residual(name, st)


@pytest.mark.parametrize("name", ["cd33_ilut", "fd17_cheb"])
def test_general_preconditioners(psk, name):
    """RightILUT (the oracle applies the same SuperLU factors' solve) and Chebyshev(3) (tests/cheby_oracle.py)."""
    st = _solve(psk, name)
    _check_prefix_parity(name, st)
    _check_true_residual(name, st)


# ---- statuses: each an ordinary return ---------------------------------------------------------------------------

def test_breakdown_at_iteration_zero(psk):
    A = sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))
    st = psk.BiCGStab(control=_ctl(psk)).makeSolver().solve(A, np.array([1.0, 0.0]))
    assert not st.success() and st.iters() == 0 and st.msg() == "breakdown dot(rhat,v)==0"
    assert st.info["status"] == "breakdown" and len(st.info["hist"]) == 0


def test_diagonal_matrix_takes_the_half_step_exit(psk):
    """diag(d) with Jacobi: s is exactly 0 when d holds powers of two (every product exact; see the CPU test), so
    the half step ends the solve at iteration 0."""
    rng = np.random.default_rng(3)
    n = 700
    d = 2.0 ** rng.integers(-3, 4, size=n)
    b = rng.standard_normal(n)
    st = psk.BiCGStab(control=_ctl(psk), precond=psk.JacobiPreconditionerType()).makeSolver().solve(
        sp.diags(d).tocsr(), b)
    assert st.success() and st.iters() == 1
    assert np.array_equal(st.info["hist"], np.array([0.0]))
    assert np.array_equal(_bits(st.soln()), _bits((1.0 / d) * b))
    assert st.info["spmv_launches"] == 2                             # v = A M^-1 p and the true residual


def test_one_by_one(psk):
    A = sp.csr_matrix(np.array([[-2.5]]))
    b = np.array([2.0])
    ref = bo.bicgstab(A, b, tau=TAU)
    st = psk.BiCGStab(control=_ctl(psk)).makeSolver().solve(A, b)
    assert st.success() and st.iters() == ref["iters"] == 1
    assert np.array_equal(_bits(st.soln()), _bits(ref["soln"])) and st.soln()[0] == -0.8
    assert np.array_equal(st.info["hist"], ref["hist"])


def test_zero_rhs_forms_no_preconditioner(psk):
    A = _matrix("cd17")

    class Counting(psk.JacobiPreconditionerType):
        formed = 0

        def form(self, M):
            Counting.formed += 1
            return super().form(M)

    solver = psk.BiCGStab(control=_ctl(psk), precond=Counting()).makeSolver()
    st = solver.solve(A, np.zeros(A.shape[0]))
    assert st.success() and st.iters() == 1 and Counting.formed == 0
    assert np.array_equal(st.soln(), np.zeros(A.shape[0]))


@pytest.mark.parametrize("fail", [True, False])
def test_maxiter_rules(psk, fail):
    ref = bo.bicgstab(_matrix("cd17"), _rhs("cd17"), M=_oracle_prec("cd17"), maxiter=5, tau=TAU, fail_on_maxiter=fail)
    st = _solve(psk, "cd17", maxiter=5, failOnMaxiter=fail)
    assert bool(st.success()) == ref["success"] == (not fail)
    assert st.iters() == ref["iters"] == (4 if fail else 5)
    assert st.info["status"] == ref["status"] == ("maxiter" if fail else "converged")
    assert (st.msg() == "failure to converge") if fail else not st.msg()
    h = st.info["hist"]
    assert len(h) == 5
    assert np.max(np.abs(h - ref["hist"])) <= RTOL_RESID * np.linalg.norm(_rhs("cd17"))   # 5 <= cd17's prefix
    assert st.resid() == h[-1]


def test_tau_zero_runs_to_maxiter_with_a_finite_history(psk):
    st = _solve(psk, "cd17", maxiter=30, tau=0.0)
    assert not st.success() and st.info["status"] == "maxiter" and st.iters() == 29
    h = st.info["hist"]
    assert len(h) == 30 and np.all(np.isfinite(h))
    assert st.info["spmv_launches"] == 60


# ---- determinism ---------------------------------------------------------------------------------------------------

def test_two_solves_are_bitwise_equal(psk):
    a, b = _solve(psk, "cd64"), _solve(psk, "cd64")
    assert a.iters() == b.iters()
    assert np.array_equal(_bits(a.info["hist"]), _bits(b.info["hist"]))
    assert np.array_equal(_bits(a.soln()), _bits(b.soln()))


def test_every_kind_of_rhs_gives_the_same_bits(psk):
    import torch
    from pysolvers_amd.Linear import DeviceVector
    b = _rhs("rand1100")
    host = _solve(psk, "rand1100")
    dv = _solve(psk, "rand1100", b=DeviceVector.from_numpy(b))
    tt = _solve(psk, "rand1100", b=torch.as_tensor(np.array(b), dtype=torch.float64, device="cuda"))
    assert isinstance(dv.soln(), DeviceVector) and tt.soln().is_cuda
    for st, x in ((dv, dv.soln().numpy()), (tt, tt.soln().cpu().numpy())):
        assert st.iters() == host.iters()
        assert np.array_equal(_bits(st.info["hist"]), _bits(host.info["hist"]))
        assert np.array_equal(_bits(x), _bits(host.soln()))


# ---- Newton ----------------------------------------------------------------------------------------------------------

def test_newton_bratu_with_bicgstab_steps(psk):
    """FD-Bratu 32^2 (examples/FDBratu2D.py): Newton with BiCGStab + Jacobi steps succeeds, and the final ||F||
    meets Newton's own stopping rule ||F|| <= tau ||F_0|| + tau (Newton.py:54)."""
    from pysolvers_amd.Nonlinear import NewtonSolver
    from oracle import newton
    func = newton.Bratu2D(m=32)
    tau = 1.0e-12
    lin = psk.BiCGStab(control=psk.CommonSolverArgs(showIters=False, showFinal=False),
                       precond=psk.JacobiPreconditionerType())
    ns = NewtonSolver(control=psk.CommonSolverArgs(tau=tau, maxiter=10, showIters=False, showFinal=False),
                      solver=lin, fixLinTol=False, minLinTol=1.0e-6, freezePrec=True)
    assert isinstance(ns.solver, psk.BiCGStabSolver)
    st = ns.solve(func, func.initialU())
    assert st.success(), st.msg()
    normF0 = np.linalg.norm(func.evalF(func.initialU()))
    assert np.linalg.norm(func.evalF(st.soln())) <= tau * normF0 + tau
    # handleConvergence(i, ...) reports i + 1 after i steps, each with one linear solve
    assert len(ns.linear_iters) == st.iters() - 1 and all(k >= 1 for k in ns.linear_iters)
