"""GPU tests of the device-resident IDR(s) solver (psk_idrs, idrs.hip; pysolvers_amd.Linear.IDRs).

Matrices, preconditioners and right-hand sides are those of tests/test_gpu_bicgstab.py (imported), plus cd33 under
RightILU0. tau = 1e-10, maxiter = 1000; one step is one SpMV, and iters, maxiter and the history count steps.

Bars (written here, not inferred):
* Residual history against tests/idrs_oracle.py: |h_dev[k] - h_oracle[k]| <= RTOL_RESID ||b|| = 1e-10 ||b|| (the
  project's solver-parity bar) for k in the PREFIX on which the oracle's own three dot-product orders (np.dot,
  math.fsum, 512-element chunks) agree within 2e-11 ||b||. The device performs the oracle's operations in the oracle's
  order, only its dot products sum in another order (gridsum), and IDR(s) amplifies that rounding as BiCGStab does.
  A case takes part only with a prefix of >= 10 steps, or with a prefix that is the three CPU runs' whole history;
  the test asserts it, so a case cannot drop out silently (cd33 with s = 8 has a prefix of 7 and is not a case).
* Equal step counts only where the three CPU runs agree on them and no oracle history entry lies within a relative
  1e-6 of tau ||b|| (bicgstab_oracle.counts_comparable).
* True residual: st.success() == (st.resid() <= tau ||b||) always (resid is the ||b - A x|| the device measured); the
  host-computed ||b - A x|| <= tau ||b|| for the cases where all three oracle runs end at <= 0.8 tau ||b|| (a run that
  ends closer to tau ||b|| may have a true residual on either side of it: cd33 with s = 4 ends at 0.95 and its true
  residual is 1.04 to 1.10 tau ||b|| in the oracle, a PSK_TRUE_RESID_FAIL by the solver's own rule).
* Run to run, across the SpMV layouts, and host / DeviceVector / CUDA-tensor right-hand sides: bitwise.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import bicgstab_oracle as bo
import idrs_oracle as io_
import ilu0_oracle
import test_gpu_bicgstab as tb
from test_gpu_bicgstab import _bits, _matrix, _rhs, psk  # noqa: F401  (psk: the module fixture)

pytestmark = pytest.mark.gpu

RTOL_RESID = 1e-10
TAU = 1e-10
MAXITER = 1000

PARITY = [("cd17", 2), ("cd17", 4), ("cd17", 8), ("cd33", 2), ("cd33", 4), ("cd64", 4), ("cd64", 8), ("dh8", 2),
          ("dh8", 4), ("dh8", 8), ("cd17_id", 4), ("rand1100", 4)]
EDGES = [("rand511", 4), ("rand512", 4), ("rand513", 4), ("rand1025", 4)]
GENERAL = [("cd33_ilut", 4), ("fd17_cheb", 4), ("cd33_ilu0", 4)]


def _kind(name):
    return "ilu0" if name == "cd33_ilu0" else tb.CASES[name]


def _oracle_prec(name):
    if _kind(name) == "ilu0":
        return ilu0_oracle.apply(ilu0_oracle.ilu0(_matrix(name)))
    return tb._oracle_prec(name)


def _device_prec(psk, name):
    return psk.RightILU0() if _kind(name) == "ilu0" else tb._device_prec(psk, name)


def _ctl(psk, **kw):
    return tb._ctl(psk, **kw)


@functools.lru_cache(maxsize=None)
def _reference(name, s):
    """(the oracle under its three dot orders, the agreeing prefix): computed once, shared, never written to."""
    res, prefix = io_.spread(_matrix(name), _rhs(name), s=s, M=_oracle_prec(name), tau=TAU, maxiter=MAXITER)
    for r in res:
        r["hist"].setflags(write=False)
    return res, prefix


def _takes_part_in_parity(name, s):
    res, prefix = _reference(name, s)
    return prefix >= 10 or all(len(r["hist"]) == prefix for r in res)


def _takes_part_in_true_residual(name, s):
    res, _ = _reference(name, s)
    nb = np.linalg.norm(_rhs(name))
    return all(r["exit"] == "tolerance" and r["hist"][-1] <= 0.8 * TAU * nb for r in res)


def _solve(psk, name, s, A=None, b=None, **ctl):
    solver = psk.IDRs(control=_ctl(psk, **ctl), precond=_device_prec(psk, name), s=s).makeSolver()
    return solver.solve(_matrix(name) if A is None else A, _rhs(name) if b is None else b)


def _check_prefix_parity(name, s, st):
    res, prefix = _reference(name, s)
    assert _takes_part_in_parity(name, s), (name, s, prefix, [len(r["hist"]) for r in res])
    nb = np.linalg.norm(_rhs(name))
    h, ho = st.info["hist"], res[0]["hist"]
    assert len(h) >= prefix, (name, s, len(h), prefix)
    dev = np.max(np.abs(h[:prefix] - ho[:prefix])) / nb
    print("%s s=%d: prefix %d of %d, history deviation %.3e ||b||, steps %d (oracle %s), last %.3f tau||b||, true "
          "residual %.3f tau||b||" % (name, s, prefix, len(ho), dev, st.iters(), [r["iters"] for r in res],
                                       h[-1] / (TAU * nb), st.resid() / (TAU * nb)))
    assert dev <= RTOL_RESID, (name, s, dev)
    if io_.counts_comparable(res, TAU):
        assert st.iters() == res[0]["iters"], (name, s, st.iters(), res[0]["iters"])


def _check_true_residual(name, s, st):
    A, b = _matrix(name), _rhs(name)
    nb = np.linalg.norm(b)
    assert st.info["status"] in ("converged", "true residual above tolerance"), (name, s, st.info["status"])
    assert bool(st.success()) == bool(st.resid() <= TAU * st.info["norm_b"]), (name, s, st.resid())
    assert st.info["norm_b"] == pytest.approx(nb, rel=1e-14)
    if _takes_part_in_true_residual(name, s):
        tr = np.linalg.norm(b - A @ np.asarray(st.soln()))
        assert tr <= TAU * nb, (name, s, tr / (TAU * nb))


def test_enough_cases_take_part():
    """At least eight parity cases and six true-residual cases (the oracle alone decides; no device run)."""
    assert sum(_takes_part_in_parity(n, s) for n, s in PARITY) >= 8
    assert all(_takes_part_in_parity(n, s) for n, s in PARITY + EDGES)
    assert sum(_takes_part_in_true_residual(n, s) for n, s in PARITY) >= 6


@pytest.mark.parametrize("name,s", PARITY)
def test_prefix_parity_with_the_oracle(psk, name, s):
    st = _solve(psk, name, s)
    _check_prefix_parity(name, s, st)
    _check_true_residual(name, s, st)
    assert len(st.info["hist"]) == st.iters() and st.info["s"] == s
    assert st.info["hist"][-1] <= TAU * st.info["norm_b"] and np.all(st.info["hist"][:-1] > TAU * st.info["norm_b"])
    assert st.info["spmv_launches"] == st.iters() + 1         # one per step + the true residual's


@pytest.mark.parametrize("name", ["cd17", "cd33", "cd64"])
def test_every_spmv_layout_gives_the_same_bits(psk, name):
    """The cd operators admit every layout; forced as tests/test_gpu_layout.py forces them. No dot product rides on
    the SpMV's layout-dependent tiles, so the whole solve is the same bits; the first meets the oracle."""
    dA = psk.DeviceCSR.from_scipy(_matrix(name))
    first = None
    for lay in ("diag", "csr", "sliced", "sliced_wide", "sliced_dict"):
        dA.set_layout(lay)
        assert dA.layout == lay
        st = _solve(psk, name, 4, A=dA)
        if first is None:
            first = st
            _check_prefix_parity(name, 4, st)
        assert st.iters() == first.iters(), lay
        assert np.array_equal(_bits(st.info["hist"]), _bits(first.info["hist"])), lay
        assert np.array_equal(_bits(st.soln()), _bits(first.soln())), lay


@pytest.mark.parametrize("name,s", EDGES)
def test_vector_tile_edges(psk, name, s):
    """One 512-element tile minus one, exactly one, one plus one (a tile of a single element), two plus one."""
    st = _solve(psk, name, s)
    _check_prefix_parity(name, s, st)
    _check_true_residual(name, s, st)
    assert st.success(), st.msg()


@pytest.mark.parametrize("name,s", GENERAL)
def test_general_preconditioners(psk, name, s):
    """RightILUT (the oracle applies the same SuperLU factors' solve), Chebyshev(3) (tests/cheby_oracle.py) and
    RightILU0 (tests/ilu0_oracle.py): v and M^-1 v materialised around prec_apply_dev."""
    st = _solve(psk, name, s)
    _check_prefix_parity(name, s, st)          # also: the oracle's step count where counts_comparable allows
    _check_true_residual(name, s, st)
    assert st.success(), st.msg()


# ---- statuses: each an ordinary return ---------------------------------------------------------------------------

def test_breakdown_on_a_zero_pivot(psk):
    A, b = io_.breakdown_system()
    ref = io_.idrs(A, b, s=4, tau=TAU)
    st = psk.IDRs(control=_ctl(psk), s=4).makeSolver().solve(A, b)
    assert not st.success() and st.iters() == ref["iters"] == 0 and st.msg() == ref["msg"] == "breakdown Mm[k][k]==0"
    assert st.info["status"] == "breakdown" and len(st.info["hist"]) == 0 and st.info["spmv_launches"] == 1


@pytest.mark.parametrize("which", ["1x1", "3x3"])
def test_systems_smaller_than_s(psk, which):
    """n < s = 4: whatever the oracle reports (status and step count; its three dot orders agree on both)."""
    if which == "1x1":
        A, b = sp.csr_matrix(np.array([[-2.5]])), np.array([2.0])
    else:
        A, b = sp.csr_matrix(np.array([[4.0, 1.0, 0.0], [-1.0, 3.0, 1.0], [0.0, -2.0, 5.0]])), np.array([1.0, 2.0, 3.0])
    refs = [io_.idrs(A, b, s=4, tau=TAU, maxiter=MAXITER, dot=d) for d in bo.DOTS]
    assert len({(r["status"], r["iters"]) for r in refs}) == 1
    st = psk.IDRs(control=_ctl(psk), s=4).makeSolver().solve(A, b)
    assert (st.info["status"], st.iters()) == (refs[0]["status"], refs[0]["iters"])
    assert len(st.info["hist"]) == len(refs[0]["hist"])
    if which == "1x1":                                   # one row: no summation order
        assert np.array_equal(_bits(st.soln()), _bits(refs[0]["soln"])) and st.soln()[0] == -0.8
        assert np.array_equal(st.info["hist"], refs[0]["hist"])


def test_zero_rhs_forms_no_preconditioner(psk):
    A = _matrix("cd17")

    class Counting(psk.JacobiPreconditionerType):
        formed = 0

        def form(self, M):
            Counting.formed += 1
            return super().form(M)

    solver = psk.IDRs(control=_ctl(psk), precond=Counting(), s=4).makeSolver()
    st = solver.solve(A, np.zeros(A.shape[0]))
    assert st.success() and st.iters() == 1 and Counting.formed == 0
    assert np.array_equal(st.soln(), np.zeros(A.shape[0]))


@pytest.mark.parametrize("fail", [True, False])
@pytest.mark.parametrize("mi", [3, 5, 7])
def test_maxiter_rules(psk, fail, mi):
    """maxiter inside a cycle (3), on the omega step (s + 1 = 5) and behind it (7)."""
    ref = io_.idrs(_matrix("cd17"), _rhs("cd17"), s=4, M=_oracle_prec("cd17"), maxiter=mi, tau=TAU,
                   fail_on_maxiter=fail)
    st = _solve(psk, "cd17", 4, maxiter=mi, failOnMaxiter=fail)
    assert bool(st.success()) == ref["success"] == (not fail)
    assert st.iters() == ref["iters"] == (mi - 1 if fail else mi)
    assert st.info["status"] == ref["status"] == ("maxiter" if fail else "converged")
    assert (st.msg() == "failure to converge") if fail else not st.msg()
    h = st.info["hist"]
    assert len(h) == mi
    assert np.max(np.abs(h - ref["hist"])) <= RTOL_RESID * np.linalg.norm(_rhs("cd17"))   # 7 <= cd17's prefix (33)
    assert st.resid() == h[-1] and st.info["spmv_launches"] == mi


def test_tau_zero_runs_to_maxiter_with_a_finite_history(psk):
    st = _solve(psk, "cd17", 4, maxiter=30, tau=0.0)
    assert not st.success() and st.info["status"] == "maxiter" and st.iters() == 29
    h = st.info["hist"]
    assert len(h) == 30 and np.all(np.isfinite(h))
    assert st.info["spmv_launches"] == 30


# ---- psk_idrs itself: refusals, the whole result for b = 0, check_every ---------------------------------------------

def _raw(system, b, s=4, **kw):
    """One psk_idrs call on host vectors: (rc, x, hist, result)."""
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
    rc = N.lib.psk_idrs(dA.handle, M.device_handle if M is not None else None, N.ptr(b), N.ptr(x), ctypes.byref(ctl), s,
                        ctypes.byref(res), N.ptr(hist), N.PSK_HOST)
    return rc, x, hist[:max(res.hist_len, 0)].copy(), res


def _same(a, b, tag):
    (_, xa, ha, ra), (_, xb, hb, rb) = a, b
    assert xa.tobytes() == xb.tobytes(), tag
    assert ha.tobytes() == hb.tobytes(), tag
    assert [getattr(ra, f) for f in tb.INT_FIELDS] == [getattr(rb, f) for f in tb.INT_FIELDS], tag
    for f in ("resid", "resid_recursive", "norm_b"):
        assert np.float64(getattr(ra, f)).tobytes() == np.float64(getattr(rb, f)).tobytes(), (tag, f)
    assert ra.msg == rb.msg, tag


def test_bad_s_is_refused(psk):
    from pysolvers_amd import _native as N
    system, b = tb._system(psk, "cd17"), _rhs("cd17")
    for s in (0, 9, -1):
        assert _raw(system, b, s=s)[0] == N.PSK_ERR_ARG, s
        assert b"psk_idrs" in N.lib.psk_last_error()
        with pytest.raises(ValueError):
            psk.IDRs(s=s)
    for s in (1, 8):
        rc, _, h, r = _raw(system, b, s=s)
        assert rc == N.PSK_OK and r.exit == N.PSK_EXIT_TOLERANCE and r.hist_len == r.iters == len(h)


@pytest.mark.parametrize("name", ["cd17", "fd17_cheb"])
def test_zero_rhs_whole_result_and_no_stamp_left_behind(psk, name):
    """b = 0 through the library (the Python layer answers it before the call): the whole result; and its done stamp
    is not one the next solve acts on (Jacobi, and a general preconditioner, whose solve reads the stamp in front of
    its loop)."""
    from pysolvers_amd import _native as N
    system, b = tb._system(psk, name), _rhs(name)
    first = _raw(system, b)
    assert first[0] == N.PSK_OK and first[3].exit == N.PSK_EXIT_TOLERANCE and first[3].iters > 1
    rc, x, h, r = _raw(system, np.zeros(b.size))
    assert rc == N.PSK_OK
    assert tuple(getattr(r, f) for f in tb.INT_FIELDS) == (N.PSK_CONVERGED, 1, N.PSK_EXIT_NONE, 1, 0, 0, 0)
    assert r.resid == 0.0 and r.resid_recursive == 0.0 and r.norm_b == 0.0 and not np.any(x) and r.msg == b""
    _same(first, _raw(system, b), name)


@pytest.mark.parametrize("stop", ["tolerance", "maxiter10"])
@pytest.mark.parametrize("name,prec", [("cd17", "jacobi"), ("rand513", "identity")])
def test_check_every_never_shows(psk, name, prec, stop):
    """The poll chunk (ctl.check_every: 1, 3 and the default) shows in nothing: x, the history and every integer field
    of the result, spmv_launches included (it counts launches that did their work, not enqueued ones)."""
    from pysolvers_amd import _native as N
    system, b = tb._system(psk, name, prec), _rhs(name)
    kw = {} if stop == "tolerance" else dict(maxiter=10)
    runs = [_raw(system, b, check_every=C, **kw) for C in (1, 3, 0)]
    r0 = runs[0][3]
    assert all(run[0] == N.PSK_OK for run in runs)
    if stop == "tolerance":
        assert (r0.exit, r0.hist_len) == (N.PSK_EXIT_TOLERANCE, r0.iters) and 10 < r0.iters < MAXITER
        assert r0.spmv_launches == r0.iters + 1
    else:
        assert (r0.status, r0.success, r0.exit) == (N.PSK_MAXITER, 0, N.PSK_EXIT_MAXITER)
        assert r0.iters == 9 and r0.hist_len == 10 and r0.spmv_launches == 10
    for i, run in enumerate(runs[1:]):
        _same(runs[0], run, (name, prec, stop, i + 1))


def test_sharded_matrices(psk):
    """A matrix sharded over one rank solves, to the bits of the unsharded matrix; more than one rank is refused (a
    dry communicator: no collectives needed to refuse)."""
    from pysolvers_amd import _native as N
    m = 17
    b = _rhs("fd17_cheb")
    one = psk.Linear.Communicator(1, 0, dry=True)
    two = psk.Linear.Communicator(2, 0, dry=True)
    try:
        whole = _raw((psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m), None), b)
        dS = psk.Linear.fd_laplacian_2d_sharded(-1.0, 1.0, m, one)
        assert dS.n == m * m
        shard = _raw((dS, None), b)
        assert whole[0] == shard[0] == N.PSK_OK and whole[3].status == N.PSK_CONVERGED
        _same(whole, shard, "one rank")
        d2 = psk.Linear.fd_laplacian_2d_sharded(-1.0, 1.0, m, two)
        assert _raw((d2, None), np.ones(d2.n))[0] == N.PSK_ERR_UNSUPPORTED
        assert b"sharded" in N.lib.psk_last_error()
        del dS, d2
    finally:
        one.destroy()
        two.destroy()


# ---- determinism ---------------------------------------------------------------------------------------------------

def test_two_solves_are_bitwise_equal(psk):
    a, b = _solve(psk, "cd64", 8), _solve(psk, "cd64", 8)
    assert a.iters() == b.iters()
    assert np.array_equal(_bits(a.info["hist"]), _bits(b.info["hist"]))
    assert np.array_equal(_bits(a.soln()), _bits(b.soln()))


def test_every_kind_of_rhs_gives_the_same_bits(psk):
    import torch
    from pysolvers_amd.Linear import DeviceVector
    b = _rhs("rand1100")
    host = _solve(psk, "rand1100", 4)
    dv = _solve(psk, "rand1100", 4, b=DeviceVector.from_numpy(b))
    tt = _solve(psk, "rand1100", 4, b=torch.as_tensor(np.array(b), dtype=torch.float64, device="cuda"))
    assert isinstance(dv.soln(), DeviceVector) and tt.soln().is_cuda
    for st, x in ((dv, dv.soln().numpy()), (tt, tt.soln().cpu().numpy())):
        assert st.iters() == host.iters()
        assert np.array_equal(_bits(st.info["hist"]), _bits(host.info["hist"]))
        assert np.array_equal(_bits(x), _bits(host.soln()))


# ---- Newton ----------------------------------------------------------------------------------------------------------

def test_newton_bratu_with_idrs_steps(psk):
    """FD-Bratu 32^2 (examples/FDBratu2D.py): Newton with IDR(4) + Jacobi steps succeeds, and the final ||F|| meets
    Newton's own stopping rule ||F|| <= tau ||F_0|| + tau (Newton.py:54)."""
    from pysolvers_amd.Nonlinear import NewtonSolver
    from oracle import newton
    func = newton.Bratu2D(m=32)
    tau = 1.0e-12
    lin = psk.IDRs(control=psk.CommonSolverArgs(showIters=False, showFinal=False),
                   precond=psk.JacobiPreconditionerType(), s=4)
    ns = NewtonSolver(control=psk.CommonSolverArgs(tau=tau, maxiter=10, showIters=False, showFinal=False),
                      solver=lin, fixLinTol=False, minLinTol=1.0e-6, freezePrec=True)
    assert isinstance(ns.solver, psk.IDRsSolver) and ns.solver.s() == 4
    st = ns.solve(func, func.initialU())
    assert st.success(), st.msg()
    normF0 = np.linalg.norm(func.evalF(func.initialU()))
    assert np.linalg.norm(func.evalF(st.soln())) <= tau * normF0 + tau
    # handleConvergence(i, ...) reports i + 1 after i steps, each with one linear solve
    assert len(ns.linear_iters) == st.iters() - 1 and all(k >= 1 for k in ns.linear_iters)
