"""GPU tests of the device-resident MINRES solver (psk_minres, minres.hip; pysolvers_amd.Linear.MINRES).

Bars (written here, not inferred):
* Residual history against tests/minres_oracle.py (pinned to scipy's iterates by tests/test_minres_cpu.py):
  |h_dev[k] - h_oracle[k]| <= RTOL_RESID ||b|| = 1e-10 ||b|| (the project's solver-parity bar) for k in the PREFIX on
  which the oracle's own three dot-product orders (np.dot, math.fsum, 512-element chunks) agree within 2e-11 ||b||.
  The device performs the oracle's operations in the oracle's order, only its dot products sum in another order
  (gridsum), and the Lanczos recurrence amplifies that rounding: past the prefix two CPU summation orders part by
  about 1e-3 ||b||, so nothing can be asserted there. 1e-10 is 5x the 2e-11 cap. A case takes part only with a
  prefix of >= 10 iterations, or with a prefix that is the three CPU runs' whole history; the test asserts it, so a
  case cannot drop out silently.
* Equal iteration counts only where the three CPU runs agree on them and no oracle history entry lies within a
  relative 1e-6 of tau ||b|| (minres_oracle.counts_comparable).
* True residual ||b - A x||_2, computed on the host with scipy: <= tau ||b|| under the identity (the solver's own
  stopping rule); under Jacobi <= sqrt(d_max / d_min) tau ||b|| (the test is made in the M^-1 norm; sqrt(cond(M)) is
  the exact bound between the two norms) with success() true. st.resid() equals the host's value to 1e-13 ||b||:
  both are sqrt of a sum of n squares of the same residual vector up to the rounding of one SpMV row sum each,
  a few 1e-16 ||A|| ||x|| per entry, far below 1e-13 ||b|| at these sizes.
* Run to run, check_every, and host / DeviceVector / CUDA-tensor right-hand sides: bitwise.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import cheby_oracle
import minres_oracle as mo
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


# name -> preconditioner. sfd<m>: the plain shifted FD operator; ssfd<m>: its scaled form S A S; rand<n>:
# rand_sym_indef; fd17: the SPD 17^2 Laplacian (the general preconditioners need an SPD M, and get it from an SPD A)
CASES = {"sfd17": "identity", "ssfd17": "identity", "ssfd17_j": "jacobi", "ssfd23_j": "jacobi", "ssfd33_j": "jacobi",
         "sfd33": "identity", "rand1100": "identity", "rand511": "identity", "rand512": "identity",
         "rand513": "identity", "rand1025": "identity", "fd17_cheb": "cheb", "fd17_ic": "ic"}
SIX = ["sfd17", "ssfd17", "ssfd17_j", "ssfd23_j", "ssfd33_j", "sfd33"]


@functools.lru_cache(maxsize=None)
def _problem(name):
    base = name.split("_")[0]
    if base.startswith("ssfd"):
        A, b = mo.shifted_fd(int(base[4:]), True)
    elif base.startswith("sfd"):
        A, b = mo.shifted_fd(int(base[3:]), False)
    elif base.startswith("rand"):
        n = int(base[4:])
        A, b = mo.rand_sym_indef(n, 7 if n == 1100 else n)
    elif base == "fd17":
        A = (-fdlap.fd_laplacian_2d(-1.0, 1.0, 17)).tocsr()
        b = np.random.default_rng(len(name) + 17).standard_normal(A.shape[0])
    else:
        raise KeyError(name)
    b.setflags(write=False)
    return A, b


def _matrix(name):
    return _problem(name)[0]


def _rhs(name):
    return _problem(name)[1]


def _oracle_prec(name):
    A = _matrix(name)
    return {"jacobi": lambda: krylov.jacobi_form(A), "identity": lambda: mo.identity,
            "ic": lambda: krylov.ic_form(A), "cheb": lambda: cheby_oracle.Chebyshev(A, degree=3)}[CASES[name]]()


def _device_prec(psk, name):
    return {"jacobi": psk.JacobiPreconditionerType, "identity": psk.IdentityPreconditionerType,
            "ic": psk.RightIC, "cheb": lambda: psk.Chebyshev(degree=3)}[CASES[name]]()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(the oracle under its three dot orders, the agreeing prefix): computed once, shared, never written to."""
    res, prefix = mo.spread(_matrix(name), _rhs(name), M=_oracle_prec(name), tau=TAU, maxiter=MAXITER)
    for r in res:
        r["hist"].setflags(write=False)
        r["soln"].setflags(write=False)
    return res, prefix


def _solve(psk, name, A=None, b=None, **ctl):
    solver = psk.MINRES(control=_ctl(psk, **ctl), precond=_device_prec(psk, name)).makeSolver()
    return solver.solve(_matrix(name) if A is None else A, _rhs(name) if b is None else b)


def _check_prefix_parity(name, st):
    res, prefix = _reference(name)
    whole = all(len(r["hist"]) == prefix for r in res)
    assert prefix >= 10 or whole, (name, prefix, [len(r["hist"]) for r in res])
    if name in SIX or name.startswith("rand"):
        assert prefix >= 10, (name, prefix)
    nb = np.linalg.norm(_rhs(name))
    h, ho = st.info["hist"], res[0]["hist"]
    assert len(h) >= prefix, (name, len(h), prefix)
    dev = np.max(np.abs(h[:prefix] - ho[:prefix])) / nb
    print("%s: prefix %d of %d, history deviation %.3e ||b||, iters %d (oracle %s)"
          % (name, prefix, len(ho), dev, st.iters(), [r["iters"] for r in res]))
    assert dev <= RTOL_RESID, (name, dev)
    assert st.success(), (name, st.msg())
    if mo.counts_comparable(res, TAU):
        assert st.iters() == res[0]["iters"], (name, st.iters(), res[0]["iters"])


def _check_true_residual(name, st):
    """the true residual by scipy on the host against the bar of the case's norm, and against st.resid()"""
    A, b = _matrix(name), _rhs(name)
    nb = np.linalg.norm(b)
    tr = np.linalg.norm(b - A @ np.asarray(st.soln()))
    kind = CASES[name]
    if kind == "identity":
        bound = TAU * nb
    elif kind == "jacobi":
        d = A.diagonal()
        bound = np.sqrt(d.max() / d.min()) * TAU * nb
    else:
        bound = None                                  # cond(M) of a general preconditioner is not at hand
    print("%s: true residual %.3e ||b|| (tau = %.0e), resid() - host = %.2e ||b||" % (name, tr / nb, TAU,
                                                                                      (st.resid() - tr) / nb))
    assert st.success() and st.info["status"] == "converged"
    if bound is not None:
        assert tr <= bound, (name, tr / nb)
    assert abs(st.resid() - tr) <= 1e-13 * nb, (name, st.resid(), tr)


@pytest.mark.parametrize("name", SIX + ["rand1100", "fd17_cheb", "fd17_ic"])
def test_prefix_parity_with_the_oracle(psk, name):
    st = _solve(psk, name)
    _check_prefix_parity(name, st)
    _check_true_residual(name, st)
    assert len(st.info["hist"]) == st.iters()
    assert st.info["spmv_launches"] == st.iters() + 1          # one per iteration, + the true residual's
    assert st.info["resid_recursive"] == st.info["hist"][-1] <= TAU * st.info["norm_b"]
    if CASES[name] == "identity":                              # scale is exactly 1 and the residual never grows
        assert st.info["hist"][0] <= st.info["norm_b"]


@pytest.mark.parametrize("name", ["sfd17", "sfd33"])
def test_every_spmv_layout_gives_the_same_solve(psk, name):
    """The plain shifted operators admit every layout (constant diagonals, two distinct values); forced as
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


def test_grouped_gridsum(psk):
    """Plain shifted FD at m = 363, sigma = 1.5 given: n = 131,769 is 258 vector tiles, past the 256-tile one-level
    limit of the gridsum, with odd n. Jacobi, tau = 0, maxiter = 12: the 12 entries agree with the oracle (12 is
    far inside any prefix: after 12 steps of a three-term recurrence the dot orders differ by a few ulps)."""
    A, b = mo.shifted_fd(363, False, sigma=1.5)
    assert A.shape[0] == 131769 and -(-A.shape[0] // 512) == 258
    ref = mo.minres(A, b, M=krylov.jacobi_form(A), maxiter=12, tau=0.0)
    st = psk.MINRES(control=_ctl(psk, maxiter=12, tau=0.0), precond=psk.JacobiPreconditionerType()).makeSolver().solve(A, b)
    h = st.info["hist"]
    assert len(h) == len(ref["hist"]) == 12 and st.info["status"] == "maxiter" and st.info["spmv_launches"] == 12
    dev = np.max(np.abs(h - ref["hist"])) / np.linalg.norm(b)
    print("m = 363: history deviation %.3e ||b|| over 12 iterations" % dev)
    assert dev <= RTOL_RESID, dev
    assert np.linalg.norm(st.soln() - ref["soln"]) <= 1e-10 * np.linalg.norm(ref["soln"])


def test_solution_includes_the_last_update(psk):
    """x carries the w and x update of the iteration whose finisher raised `done`: within 1e-10 (relative) of the
    oracle's final x on a case whose counts are comparable — one missing update phi w would be off by about
    ||r|| / |lambda|_min, orders above that."""
    names = [n for n in SIX + ["rand1100"] if mo.counts_comparable(_reference(n)[0], TAU)]
    assert names, "no case with comparable counts"
    for name in names[:2]:
        res, prefix = _reference(name)
        st = _solve(psk, name)
        assert st.iters() == res[0]["iters"]
        err = np.linalg.norm(st.soln() - res[0]["soln"]) / np.linalg.norm(res[0]["soln"])
        print("%s: final x deviates %.3e (relative) from the oracle's" % (name, err))
        assert err <= 1e-10, (name, err)


def test_one_by_one_and_swap(psk):
    st = psk.MINRES(control=_ctl(psk)).makeSolver().solve(sp.csr_matrix(np.array([[-2.5]])), np.array([2.0]))
    assert st.success() and st.iters() == 1 and st.soln()[0] == -0.8 and np.array_equal(st.info["hist"], [0.0])
    st = psk.MINRES(control=_ctl(psk)).makeSolver().solve(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])),
                                                          np.array([1.0, 0.0]))
    assert st.success() and st.iters() == 2
    assert np.array_equal(st.info["hist"], [1.0, 0.0]) and np.array_equal(st.soln(), [0.0, 1.0])
    assert st.info["spmv_launches"] == 3


def test_zero_rhs_forms_no_preconditioner(psk):
    A = _matrix("ssfd17_j")

    class Counting(psk.JacobiPreconditionerType):
        formed = 0

        def form(self, M):
            Counting.formed += 1
            return super().form(M)

    solver = psk.MINRES(control=_ctl(psk), precond=Counting()).makeSolver()
    st = solver.solve(A, np.zeros(A.shape[0]))
    assert st.success() and st.iters() == 1 and Counting.formed == 0
    assert np.array_equal(st.soln(), np.zeros(A.shape[0]))


def test_breakdowns_through_the_python_layer(psk):
    d = sp.diags([1.0, -1.0]).tocsr()
    st = psk.MINRES(control=_ctl(psk), precond=psk.JacobiPreconditionerType()).makeSolver().solve(d, np.array([1.0, 2.0]))
    assert not st.success() and st.iters() == 0 and st.msg() == "preconditioner not positive definite"
    assert st.info["status"] == "breakdown" and len(st.info["hist"]) == 0
    st = psk.MINRES(control=_ctl(psk)).makeSolver().solve(sp.csr_matrix(np.ones((2, 2))), np.array([1.0, -1.0]))
    assert not st.success() and st.iters() == 0 and st.msg() == "breakdown gamma==0"


def test_caller_norm_sets_the_threshold(psk):
    """A caller's norm (here 2 ||.||_2) sets the threshold through norm_b; under the identity the true residual is
    re-tested in that norm, under Jacobi it is not and the device's 2-norm value is reported."""
    for name in ("sfd17", "ssfd17_j"):
        solver = psk.MINRES(control=_ctl(psk, norm=lambda v: 2.0 * float(np.linalg.norm(v))),
                            precond=_device_prec(psk, name)).makeSolver()
        A, b = _matrix(name), _rhs(name)
        st = solver.solve(A, b)
        nb = np.linalg.norm(b)
        assert st.success() and st.info["norm_b"] == 2.0 * nb
        tr = np.linalg.norm(b - A @ st.soln())
        assert abs(st.resid() - (2.0 * tr if name == "sfd17" else tr)) <= 1e-13 * nb
        assert st.info["hist"][-1] <= TAU * 2.0 * nb < st.info["hist"][-2]


# ---- psk_minres itself: the whole psk_result per exit kind, the stamp's generation, check_every --------------------
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
    """One psk_minres call on host vectors: (x, hist, result)."""
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
    N.check(N.lib.psk_minres(dA.handle, M.device_handle if M is not None else None, N.ptr(b), N.ptr(x),
                             ctypes.byref(ctl), ctypes.byref(res), N.ptr(hist), N.PSK_HOST), "psk_minres")
    return x, hist[:res.hist_len].copy(), res


def _same(a, b, tag):
    (xa, ha, ra), (xb, hb, rb) = a, b
    assert xa.tobytes() == xb.tobytes(), tag
    assert ha.tobytes() == hb.tobytes(), tag
    assert [getattr(ra, f) for f in INT_FIELDS] == [getattr(rb, f) for f in INT_FIELDS], tag
    for f in ("resid", "resid_recursive", "norm_b"):
        assert np.float64(getattr(ra, f)).tobytes() == np.float64(getattr(rb, f)).tobytes(), (tag, f)
    assert ra.msg == rb.msg, tag


def _jacobi_of(psk, diag):
    """a Jacobi preconditioner with M^-1 = diag(1 / diag), formed from the diagonal matrix itself"""
    return psk.JacobiPreconditionerType().form(psk.DeviceCSR.from_scipy(sp.diags(np.asarray(diag, dtype=float)).tocsr()))


@pytest.mark.parametrize("kind", ["refused_at_init", "refused_at_one", "gamma_zero", "maxiter_fail", "maxiter_no_fail",
                                  "zero_b_jacobi", "zero_b_general"])
def test_whole_result_per_exit_kind(psk, kind):
    """status, success, exit, iters, hist_len, spmv_launches, resid, resid_recursive of every exit that is not a
    tolerance exit (those: test_prefix_parity_with_the_oracle). spmv_launches counts the SpMV launches that did
    their work: one per iteration that ran, none behind `done`, and no true-residual launch except on a
    tolerance exit."""
    from pysolvers_amd import _native as N
    mi = 5
    if kind == "refused_at_init":            # diag(1, -1), b = (1, 2), M^-1 = diag(1, -1): b.z = -3
        dA = psk.DeviceCSR.from_scipy(sp.diags([1.0, -1.0]).tocsr())
        x, h, r = _raw((dA, _jacobi_of(psk, [1.0, -1.0])), np.array([1.0, 2.0]))
        want = (N.PSK_BREAKDOWN, 0, N.PSK_EXIT_DOT_BREAKDOWN, 0, 0, 0, 0)
        assert np.isnan(r.resid) and r.resid_recursive == r.norm_b == np.sqrt(5.0)
        assert r.msg == b"preconditioner not positive definite"
    elif kind == "refused_at_one":           # the path graph, b = e1, M^-1 = diag(1, 1, -1): r2.z = -1 at k = 1
        dA = psk.DeviceCSR.from_scipy(sp.csr_matrix(np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])))
        x, h, r = _raw((dA, _jacobi_of(psk, [1.0, 1.0, -1.0])), np.array([1.0, 0.0, 0.0]))
        want = (N.PSK_BREAKDOWN, 0, N.PSK_EXIT_DOT_BREAKDOWN, 1, 1, 2, 0)
        assert np.isnan(r.resid) and r.resid_recursive == 1.0 and np.array_equal(h, [1.0])
        assert r.msg == b"preconditioner not positive definite"
    elif kind == "gamma_zero":               # ones(2, 2), b = (1, -1): A b = 0, so y = 0, alfa = 0, beta = 0
        dA = psk.DeviceCSR.from_scipy(sp.csr_matrix(np.ones((2, 2))))
        x, h, r = _raw((dA, None), np.array([1.0, -1.0]))
        want = (N.PSK_BREAKDOWN, 0, N.PSK_EXIT_DOT_BREAKDOWN, 0, 0, 1, 0)
        assert np.isnan(r.resid) and r.resid_recursive == r.norm_b == np.sqrt(2.0)
        assert r.msg == b"breakdown gamma==0"
    elif kind.startswith("maxiter"):
        fail = kind == "maxiter_fail"
        x, h, r = _raw(_system(psk, "ssfd17_j"), _rhs("ssfd17_j"), maxiter=mi, fail_on_maxiter=int(fail))
        want = (N.PSK_MAXITER, 0, N.PSK_EXIT_MAXITER, mi - 1, mi, mi, 0) if fail else \
            (N.PSK_CONVERGED, 1, N.PSK_EXIT_MAXITER, mi, mi, mi, 0)
        assert h[-1] > TAU * r.norm_b                        # not a tolerance exit: no true residual is measured
        assert r.resid == h[-1] and r.resid_recursive == h[-1]
        assert r.msg == (b"failure to converge" if fail else b"")
        ref = mo.minres(_matrix("ssfd17_j"), _rhs("ssfd17_j"), M=_oracle_prec("ssfd17_j"), maxiter=mi, tau=TAU,
                        fail_on_maxiter=fail)
        assert np.max(np.abs(h - ref["hist"])) <= RTOL_RESID * r.norm_b       # 5 <= the case's prefix
        # x holds all five updates, whichever way the loop ended
        assert np.linalg.norm(x - ref["soln"]) <= 1e-10 * np.linalg.norm(ref["soln"])
    else:
        name = "ssfd17_j" if kind == "zero_b_jacobi" else "fd17_cheb"
        x, h, r = _raw(_system(psk, name), np.zeros(_matrix(name).shape[0]))
        want = (N.PSK_CONVERGED, 1, N.PSK_EXIT_NONE, 1, 0, 0, 0)
        assert r.resid == 0.0 and r.resid_recursive == 0.0 and r.norm_b == 0.0
        assert not np.any(x) and r.msg == b""
    assert tuple(getattr(r, f) for f in INT_FIELDS) == want, (kind, [getattr(r, f) for f in INT_FIELDS])
    assert len(h) == r.hist_len
    assert (r.spmv_ms, r.gather_ms, r.halo_ms) == (0.0, 0.0, 0.0)


def test_tau_zero_runs_to_maxiter_with_a_finite_history(psk):
    st = _solve(psk, "ssfd17_j", maxiter=30, tau=0.0)
    assert not st.success() and st.info["status"] == "maxiter" and st.iters() == 29
    h = st.info["hist"]
    assert len(h) == 30 and np.all(np.isfinite(h)) and np.all(np.diff(h) <= 0)
    assert st.info["spmv_launches"] == 30


@pytest.mark.parametrize("name", ["ssfd17_j", "fd17_cheb"])
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
@pytest.mark.parametrize("name", ["ssfd17_j", "rand513", "fd17_cheb"])
def test_check_every_never_shows(psk, name, stop):
    """The poll chunk (ctl.check_every: 1, 3, and 16 > maxiter = 10) shows in nothing: x (the last iteration's owed
    update included), the history and every integer field of the result, spmv_launches included."""
    from pysolvers_amd import _native as N
    system, b = _system(psk, name), _rhs(name)
    kw = {} if stop == "tolerance" else dict(maxiter=10)
    runs = [_raw(system, b, check_every=C, **kw) for C in (1, 3, 16)]
    r0 = runs[0][2]
    if stop == "tolerance":
        assert (r0.status, r0.success, r0.exit) == (N.PSK_CONVERGED, 1, N.PSK_EXIT_TOLERANCE)
        assert 10 < r0.iters < MAXITER and r0.hist_len == r0.iters and r0.spmv_launches == r0.iters + 1
    else:
        assert (r0.status, r0.success, r0.exit) == (N.PSK_MAXITER, 0, N.PSK_EXIT_MAXITER)
        assert r0.iters == 9 and r0.hist_len == 10 and r0.spmv_launches == 10
    for i, run in enumerate(runs[1:]):
        _same(runs[0], run, (name, stop, i + 1))


# ---- determinism -----------------------------------------------------------------------------------------------------

def test_two_solves_are_bitwise_equal(psk):
    a, b = _solve(psk, "ssfd33_j"), _solve(psk, "ssfd33_j")
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
