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
    # 2 SpMV launches per iteration, 1 in the iteration a half-step exit ends, + 1 for the true residual. Which
    # exit the device took: with tau = 0 the same iterations run (tau only stops them) and the last one takes its
    # full step, so its history entry is ||r||; the solve's own last entry is that, or the half step's ||s||.
    # Where the oracle's three dot orders agree on the count they also say which exit it is.
    k = st.iters() - 1
    full = _raw(_system(psk, name), _rhs(name), maxiter=k + 1, tau=0.0)[1]
    assert np.array_equal(_bits(full[:k]), _bits(st.info["hist"][:k]))
    half = _bits(full)[k] != _bits(st.info["hist"])[k]
    res, _ = _reference(name)
    if bo.counts_comparable(res, TAU):
        assert {r["half"] for r in res} == {half}, (name, half)
    print("%s: %s tolerance exit at k = %d, %d SpMV launches" % (name, "half-step" if half else "full-step", k,
                                                                st.info["spmv_launches"]))
    assert st.info["spmv_launches"] == 2 * st.iters() + (0 if half else 1)


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


# ---- psk_bicgstab itself: the whole psk_result per exit kind, the stamp's generation, check_every ------------------
# (past the Python layer, which answers b = 0 before it calls the library and always passes check_every = 0)

INT_FIELDS = ("status", "success", "exit", "iters", "hist_len", "spmv_launches", "comm_samples")
_systems = {}


def _system(psk, name, prec=None):
    """(DeviceCSR, formed preconditioner or None for the identity) of a case, built once."""
    prec = CASES[name] if prec is None else prec
    if (name, prec) not in _systems:
        dA = psk.DeviceCSR.from_scipy(_matrix(name))
        _systems[name, prec] = (dA, None if prec == "identity" else _device_prec(psk, name).form(dA))
    return _systems[name, prec]


def _raw(system, b, **kw):
    """One psk_bicgstab call on host vectors: (x, hist, result)."""
    import ctypes
    from pysolvers_amd import _native as N
    dA, M = system
    kw.setdefault("maxiter", MAXITER)
    kw.setdefault("tau", TAU)
    kw.setdefault("fail_on_maxiter", 1)
    ctl = N.PskCtl(restart=0, time_kernels=0, norm_b=0.0, **kw)
    res = N.PskResult()
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.full(b.size, np.nan)
    hist = np.zeros(ctl.maxiter + 1)
    N.check(N.lib.psk_bicgstab(dA.handle, M.device_handle if M is not None else None, N.ptr(b), N.ptr(x),
                               ctypes.byref(ctl), ctypes.byref(res), N.ptr(hist), N.PSK_HOST), "psk_bicgstab")
    return x, hist[:res.hist_len].copy(), res


def _same(a, b, tag):
    (xa, ha, ra), (xb, hb, rb) = a, b
    assert xa.tobytes() == xb.tobytes(), tag
    assert ha.tobytes() == hb.tobytes(), tag
    assert [getattr(ra, f) for f in INT_FIELDS] == [getattr(rb, f) for f in INT_FIELDS], tag
    for f in ("resid", "resid_recursive", "norm_b"):
        assert np.float64(getattr(ra, f)).tobytes() == np.float64(getattr(rb, f)).tobytes(), (tag, f)
    assert ra.msg == rb.msg, tag


@pytest.mark.parametrize("kind", ["rhatv_breakdown", "maxiter_fail", "maxiter_no_fail", "zero_b_jacobi",
                                  "zero_b_general"])
def test_whole_result_per_exit_kind(psk, kind):
    """status, success, exit, iters, hist_len, spmv_launches, resid, resid_recursive of every exit that is not a
    tolerance exit (those: test_prefix_parity_with_the_oracle, test_diagonal_matrix_takes_the_half_step_exit).
    spmv_launches counts the SpMV launches that did their work: 2 per completed iteration, 1 in an iteration the
    rhat.v test ended, none behind `done`, and no true-residual launch except on a tolerance exit."""
    from pysolvers_amd import _native as N
    mi = 5
    if kind == "rhatv_breakdown":
        dA = psk.DeviceCSR.from_scipy(sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]])))
        x, h, r = _raw((dA, None), np.array([1.0, 0.0]))
        want = (N.PSK_BREAKDOWN, 0, N.PSK_EXIT_DOT_BREAKDOWN, 0, 0, 1, 0)
        assert np.isnan(r.resid) and r.resid_recursive == r.norm_b == 1.0   # no residual was reported: ||b||
        assert r.msg == b"breakdown dot(rhat,v)==0"
    elif kind.startswith("maxiter"):
        fail = kind == "maxiter_fail"
        x, h, r = _raw(_system(psk, "cd17"), _rhs("cd17"), maxiter=mi, fail_on_maxiter=int(fail))
        want = (N.PSK_MAXITER, 0, N.PSK_EXIT_MAXITER, mi - 1, mi, 2 * mi, 0) if fail else \
            (N.PSK_CONVERGED, 1, N.PSK_EXIT_MAXITER, mi, mi, 2 * mi, 0)
        assert h[-1] > TAU * r.norm_b                        # not a tolerance exit: no true residual is measured
        assert r.resid == h[-1] and r.resid_recursive == h[-1]
        assert r.msg == (b"failure to converge" if fail else b"")
        assert np.all(np.isfinite(x))
    else:
        name = "cd17" if kind == "zero_b_jacobi" else "fd17_cheb"
        x, h, r = _raw(_system(psk, name), np.zeros(_matrix(name).shape[0]))
        want = (N.PSK_CONVERGED, 1, N.PSK_EXIT_NONE, 1, 0, 0, 0)
        assert r.resid == 0.0 and r.resid_recursive == 0.0 and r.norm_b == 0.0
        assert not np.any(x) and r.msg == b""
    assert tuple(getattr(r, f) for f in INT_FIELDS) == want, (kind, [getattr(r, f) for f in INT_FIELDS])
    assert len(h) == r.hist_len
    assert (r.spmv_ms, r.gather_ms, r.halo_ms) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("name", ["cd17", "fd17_cheb"])
def test_a_zero_solve_leaves_no_stamp_behind(psk, name):
    """The done stamp of a b = 0 solve (1, tagged with that solve's generation) is not one the next solve acts
    on: the same solve directly after a b = 0 solve gives the bits it gave before. Jacobi, and a general
    preconditioner (whose solve reads the stamp in front of its loop)."""
    from pysolvers_amd import _native as N
    system, b = _system(psk, name), _rhs(name)
    first = _raw(system, b)
    assert first[2].status == N.PSK_CONVERGED and first[2].exit == N.PSK_EXIT_TOLERANCE and first[2].iters > 1
    zero = _raw(system, np.zeros(b.size))
    assert zero[2].exit == N.PSK_EXIT_NONE and zero[2].spmv_launches == 0
    _same(first, _raw(system, b), name)


@pytest.mark.parametrize("stop", ["tolerance", "maxiter10"])
@pytest.mark.parametrize("name,prec", [("cd17", "jacobi"), ("rand513", "identity")])
def test_check_every_never_shows(psk, name, prec, stop):
    """The poll chunk (ctl.check_every: 1, 3, and 16 > maxiter = 10) shows in nothing: x, the history and every
    integer field of the result, spmv_launches included (it counts launches that did their work, not enqueued
    ones). tests/test_gpu_solve_loop.py holds psk_pcg to the same."""
    from pysolvers_amd import _native as N
    system, b = _system(psk, name, prec), _rhs(name)
    kw = {} if stop == "tolerance" else dict(maxiter=10)
    runs = [_raw(system, b, check_every=C, **kw) for C in (1, 3, 16)]
    r0 = runs[0][2]
    if stop == "tolerance":
        assert (r0.status, r0.success, r0.exit) == (N.PSK_CONVERGED, 1, N.PSK_EXIT_TOLERANCE)
        assert 10 < r0.iters < MAXITER and r0.hist_len == r0.iters
    else:
        assert (r0.status, r0.success, r0.exit) == (N.PSK_MAXITER, 0, N.PSK_EXIT_MAXITER)
        assert r0.iters == 9 and r0.hist_len == 10 and r0.spmv_launches == 20
    for i, run in enumerate(runs[1:]):
        _same(runs[0], run, (name, prec, stop, i + 1))


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
