"""GPU tests of psk_pcg_multi (pcg_multi.hip): several right-hand sides in one PCG loop, every column an independent PCG.

Matrices: tests/pcg_replay.py's generators (random SPD at n = 1, 2, the tile edges 255, 256, 257, 513 of the 256-row
tiles and 65537 = 257 tiles, the first two-level gridsum; FD sides 17 and 363) and two "arrow" matrices built in
tests/pcg_multi_oracle.py (row and column 5 full; at n = 1100 the hub's tile holds more entries than one 1280-entry
staging chunk, at n = 1500 the hub row alone does). Preconditioners: identity and Jacobi. nrhs = 1, 2, 3, 4.

1. Replay, per column (the method of tests/pcg_replay.py): given the device's own alphas and udr (psk_lab_pcg_multi_
   internals) the host replays the column's x, r, p and Ap, which must match BIT FOR BIT at depths 1, 2 and 9 (capped by
   n). Every grid sum is held to pcg_replay.check_sum's bound against math.fsum of its terms. Which exact sum, read from
   the kernels: ALL of them are exact_dot (ROUNDED products): p.Ap (pcgm_spmm_kernel: acc = eq * sum, as spmv_row_value),
   b.b and the init's u.r (pcgm_init_kernel: bv * bv, uv * bv), and kernel U's r.r and u.r (pcgm_update_kernel runs one
   row per lane, so each lane holds ONE product per sum, rn * rn and u * rn, rounded before the wave total adds it;
   there is no fma chain as in psk_pcg's K2, hence exact_dot and not exact_dot_fma).
2. Independence: a column's bits do not depend on its position or on the other columns; identical calls are bitwise equal.
3. Mixed stopping: columns that stop at different iterations, a b = 0 column, an underflowing column, a column that
   breaks down; statuses against the oracle, frozen columns against the same call with the other columns zeroed, the
   sentinel tail of every history untouched.
4. Against psk_pcg column by column and against the reference's golden runs.
5. Rules and refusals. 6. No gridsum error after the whole file (every solve ends with gridsum_check; the last test runs
   one more of each solver).

Largest |device - exact| / dot_bound over all cases on an MI355X (a record, not a bar to tighten): b.b 7.8e-3, p.Ap
1.2e-2, r.r 7.8e-3, u.r 1.0e-2. The whole file takes about 11 s.

The psk_result fields compared bitwise between calls leave out the device-wide ones (loop_ms, spmv_ms, spmv_launches:
include/psk.h), which describe the whole call, not the column.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import pcg_multi_oracle as mo
import pcg_replay as pr
from conftest import golden_matrix, load_golden, solver_cases

pytestmark = pytest.mark.gpu

TAU = 1e-8
SENTINEL = np.float64(np.nan)
FIELDS = ("status", "success", "iters", "hist_len", "exit")
FLOATS = ("resid", "resid_recursive", "norm_b")


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU visible to libpsk"
    return pysolvers_amd


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _same(a, c):
    return np.array_equal(_bits(a), _bits(c))


@functools.lru_cache(maxsize=None)
def _matrix(name):
    return mo.matrix(name)


@functools.lru_cache(maxsize=None)
def _columns(name):
    B = mo.columns(name)
    B.setflags(write=False)
    return B


class Dev:
    """One matrix in HBM with its preconditioner; psk_pcg_multi, psk_pcg and the lab view through the C ABI."""

    def __init__(self, psk, A, prec, layout=None):
        from pysolvers_amd import _native as N
        self.N, self.lab, self.psk = N, N.load_lab(), psk
        self.A, self.n = A, A.shape[0]
        self.dA = psk.DeviceCSR.from_scipy(A)
        if layout is not None:
            self.dA.set_layout(layout)
        self.prec = {"jacobi": psk.JacobiPreconditionerType, "identity": psk.IdentityPreconditionerType,
                     "ilu0": psk.RightILU0}[prec]().form(self.dA)
        self.ph = None if self.prec.device_kind == N.PSK_PREC_IDENTITY else self.prec.device_handle
        self.dinv = np.reciprocal(A.diagonal()) if prec == "jacobi" else None

    def ctl(self, maxiter, tau, fail, check_every=0):
        return self.N.PskCtl(maxiter=maxiter, tau=tau, fail_on_maxiter=int(fail), restart=0, check_every=check_every,
                             time_kernels=0, norm_b=0.0)

    def multi_rc(self, B, maxiter=200, tau=TAU, fail=True, nrhs=None, check_every=0):
        """(rc, X, hist, res): hist is (m, maxiter), filled with the sentinel before the call"""
        N = self.N
        Bp = np.ascontiguousarray(B, dtype=np.float64)
        m = Bp.shape[1] if nrhs is None else nrhs
        X = np.full_like(Bp, SENTINEL)
        res = (N.PskResult * max(m, 1))()
        hist = np.full((max(m, 1), max(maxiter, 1)), SENTINEL)
        ctl = self.ctl(maxiter, tau, fail, check_every)
        rc = N.lib.psk_pcg_multi(self.dA.handle, self.ph, m, N.ptr(Bp), N.ptr(X), ctypes.byref(ctl), res, N.ptr(hist),
                                 N.PSK_HOST)
        return rc, X, hist, res

    def multi(self, B, **kw):
        rc, X, hist, res = self.multi_rc(B, **kw)
        self.N.check(rc, "psk_pcg_multi")
        return X, hist, res

    def single(self, b, maxiter=200, tau=TAU, fail=True):
        N = self.N
        bp = np.ascontiguousarray(b, dtype=np.float64)
        x = np.full_like(bp, SENTINEL)
        res = N.PskResult()
        hist = np.full(max(maxiter, 1), SENTINEL)
        ctl = self.ctl(maxiter, tau, fail)
        N.check(N.lib.psk_pcg(self.dA.handle, self.ph, N.ptr(bp), N.ptr(x), ctypes.byref(ctl), ctypes.byref(res),
                              N.ptr(hist), N.PSK_HOST), "psk_pcg")
        return x, hist, res

    def internals(self, maxiter, nrhs):
        N = self.N
        kp = 2 if nrhs <= 2 else 4
        w = dict(alphas=np.full((nrhs, maxiter + 1), np.nan), udr=np.full((nrhs, maxiter + 1), np.nan),
                 pap=np.full((nrhs, maxiter + 1), np.nan), r=np.full((self.n, kp), np.nan), p=np.full((self.n, kp), np.nan),
                 Ap=np.full((self.n, kp), np.nan), x=np.full((self.n, kp), np.nan), state=np.full((nrhs, 10), np.nan))
        N.check(self.lab.psk_lab_pcg_multi_internals(self.dA.handle, maxiter, nrhs, N.ptr(w["alphas"]), N.ptr(w["udr"]),
                                                     N.ptr(w["pap"]), N.ptr(w["r"]), N.ptr(w["p"]), N.ptr(w["Ap"]),
                                                     N.ptr(w["x"]), N.ptr(w["state"])), "psk_lab_pcg_multi_internals")
        return w


def _result_same(ra, rb, tag):
    assert [getattr(ra, f) for f in FIELDS] == [getattr(rb, f) for f in FIELDS], (tag, [getattr(ra, f) for f in FIELDS],
                                                                                   [getattr(rb, f) for f in FIELDS])
    for f in FLOATS:
        assert _same([getattr(ra, f)], [getattr(rb, f)]), (tag, f, getattr(ra, f), getattr(rb, f))
    assert ra.msg == rb.msg, tag


def _tail_untouched(hist, res, tag):
    for j in range(hist.shape[0]):
        L = res[j].hist_len if j < len(res) else 0
        assert np.all(_bits(hist[j, L:]) == _bits([SENTINEL])[0]) and np.all(np.isfinite(hist[j, :L])), (tag, j, L)


RATIOS = {}


def _check_sum(tag, kind, value, exact, a, c):
    ok, ratio = pr.check_sum(value, exact, a, c)
    RATIOS[(tag, kind)] = max(RATIOS.get((tag, kind), 0.0), ratio)
    assert ok, (tag, kind, value, exact, ratio)


# ---- 1. replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", mo.PRECS)
@pytest.mark.parametrize("name", mo.CASES)
def test_replay_per_column(psk, name, prec):
    A = _matrix(name)
    dev = Dev(psk, A, prec)
    n = dev.n
    Ks = mo.depths(n)
    for nrhs in (1, 2, 3, 4):
        tag = "%s %s nrhs=%d" % (name, prec, nrhs)
        B = np.ascontiguousarray(_columns(name)[:, :nrhs])
        runs = {}
        for K in Ks:
            X, hist, res = dev.multi(B, maxiter=K, tau=0.0, fail=False)
            w = dev.internals(K, nrhs)
            runs[K] = (X, hist, res, w)
            assert _same(X, w["x"][:, :nrhs]), tag
            for v in ("x", "r", "p"):
                assert not np.any(w[v][:, nrhs:]), (tag, v, "padding columns are b = 0 columns")
            _tail_untouched(hist, res, tag)
        Kmax = Ks[-1]
        wm = runs[Kmax][3]
        for j in range(nrhs):
            b = B[:, j]
            alphas, udr, pap = wm["alphas"][j, :Kmax], wm["udr"][j, :Kmax], wm["pap"][j, :Kmax]
            assert np.all(np.isfinite(alphas)) and np.all(np.isfinite(udr)), (tag, j)
            assert _same(alphas, udr / pap), (tag, j)
            rp = pr.replay(A, b, dev.dinv, alphas, udr, Kmax)
            st = wm["state"][j]
            _check_sum(tag, "b.b", st[8], pr.exact_dot(b, b), b, b)
            assert _same([st[4]], [np.sqrt(st[8])]), (tag, j, "normB")
            for k in range(Kmax):
                _check_sum(tag, "p.Ap", pap[k], pr.exact_dot(rp["p"][k], rp["Ap"][k]), rp["p"][k], rp["Ap"][k])
                _check_sum(tag, "u.r", udr[k], pr.exact_dot(rp["u"][k], rp["r"][k]), rp["u"][k], rp["r"][k])
            for K in Ks:
                X, hist, res, w = runs[K]
                # the shallower runs are bitwise prefixes of the deepest
                assert _same(w["alphas"][j, :K], alphas[:K]) and _same(w["udr"][j, :K], udr[:K]), (tag, j, K)
                assert _same(hist[j, :K], runs[Kmax][1][j, :K]), (tag, j, K)
                assert res[j].status == dev.N.PSK_CONVERGED and res[j].iters == K and res[j].hist_len == K, (tag, j, K)
                assert _same(w["x"][:, j], rp["x"][K]), (tag, j, K, "x")
                assert _same(w["r"][:, j], rp["r"][K]), (tag, j, K, "r")
                assert _same(w["p"][:, j], rp["p"][K - 1]), (tag, j, K, "p")
                assert _same(w["Ap"][:, j], rp["Ap"][K - 1]), (tag, j, K, "Ap")
                rr = w["state"][j, 9]
                _check_sum(tag, "r.r", rr, pr.exact_dot(rp["r"][K], rp["r"][K]), rp["r"][K], rp["r"][K])
                assert _same([hist[j, K - 1]], [np.sqrt(rr)]), (tag, j, K, "hist")
                assert _same([res[j].resid], [hist[j, K - 1]]), (tag, j, K)


# ---- 2. independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", mo.PRECS)
@pytest.mark.parametrize("name", ["rand513", "fd17"])
def test_a_column_does_not_depend_on_the_others(psk, name, prec):
    dev = Dev(psk, _matrix(name), prec)
    B = np.array(_columns(name))
    a = dev.multi(B)
    B2 = B.copy()
    B2[:, 1] = 0.0
    B2[:, 2] *= 7.0
    B2[:, 3] = np.random.default_rng(5).standard_normal(dev.n)
    b = dev.multi(B2)
    c = dev.multi(np.ascontiguousarray(B[:, ::-1]))
    assert a[2][0].status == dev.N.PSK_CONVERGED and a[2][0].iters > 3
    for (X, hist, res), j in ((b, 0), (c, 3)):
        assert _same(X[:, j], a[0][:, 0]) and _same(hist[j], a[1][0]), (name, prec, j)
        _result_same(res[j], a[2][0], (name, prec, j))
    # the reversed call is the first one column by column
    for j in range(4):
        assert _same(c[0][:, 3 - j], a[0][:, j]) and _same(c[1][3 - j], a[1][j])
        _result_same(c[2][3 - j], a[2][j], (name, prec, "rev", j))
    # two identical calls
    a2 = dev.multi(B)
    assert _same(a2[0], a[0]) and _same(a2[1], a[1])
    for j in range(4):
        _result_same(a2[2][j], a[2][j], (name, prec, "again", j))
        assert a2[2][j].spmv_launches == a[2][j].spmv_launches == a[2][0].spmv_launches


# ---- 3. mixed stopping ------------------------------------------------------------------------------------------------
def _check_against_oracle(dev, B, X, hist, res, want, tag, maxiter=200):
    N = dev.N
    status = {"converged": N.PSK_CONVERGED, "maxiter": N.PSK_MAXITER, "breakdown": N.PSK_BREAKDOWN}
    exits = {"none": N.PSK_EXIT_NONE, "tolerance": N.PSK_EXIT_TOLERANCE, "maxiter": N.PSK_EXIT_MAXITER,
             "breakdown": N.PSK_EXIT_DOT_BREAKDOWN}
    for j, o in enumerate(want):
        got = (res[j].status, res[j].exit, res[j].iters, res[j].hist_len, bool(res[j].success))
        assert got == (status[o["status"]], exits[o["exit"]], o["iters"], len(o["hist"]), o["success"]), (tag, j, got, o)
        assert res[j].msg.decode() == (o["msg"] or ""), (tag, j)
        if len(o["hist"]):
            assert np.max(np.abs(hist[j, :len(o["hist"])] - o["hist"])) <= 1e-10 * o["norm_b"], (tag, j)
    _tail_untouched(hist, res, tag)
    # a frozen column is bitwise what the same call gives with the other columns zeroed
    for j in range(B.shape[1]):
        Z = np.zeros_like(B)
        Z[:, j] = B[:, j]
        Xz, hz, rz = dev.multi(Z, maxiter=maxiter)
        assert _same(Xz[:, j], X[:, j]) and _same(hz[j], hist[j]), (tag, j)
        _result_same(rz[j], res[j], (tag, "alone", j))


@pytest.mark.parametrize("prec", mo.PRECS)
def test_mixed_stopping(psk, prec):
    """[random, 0, an eigenvector of the stencil (stops at iteration 1), random * 1e-200 (b.b underflows to 0: the b = 0
    exit, as psk_pcg and the reference take it)] on FD 17^2"""
    dev = Dev(psk, _matrix("fd17"), prec)
    B = mo.mixed_columns(17)
    X, hist, res = dev.multi(B)
    want = mo.pcg_multi(dev.A, B, dinv=dev.dinv, maxiter=200, tau=TAU)
    assert len({o["iters"] for o in want}) >= 2 and want[2]["iters"] == 1 and want[0]["iters"] > 10
    _check_against_oracle(dev, B, X, hist, res, want, ("mixed", prec))
    assert not np.any(X[:, 1]) and not np.any(X[:, 3])
    assert res[0].spmv_launches == res[3].spmv_launches == want[0]["iters"]    # the loop ran as long as its last column


def test_a_column_that_breaks_down_stops_alone(psk):
    """b = ones under Jacobi on diag(+2, -2, ...): u.r = 0 exactly, the breakdown at the start, beside a column that
    converges and a zero column; and dot(p, Ap) == 0 on the zero matrix beside a zero column"""
    D = mo.indefinite_diagonal()
    dev = Dev(psk, D, "jacobi")
    B = mo.breakdown_columns()
    X, hist, res = dev.multi(B, maxiter=50)
    want = mo.pcg_multi(D, B, dinv=dev.dinv, maxiter=50, tau=TAU)
    assert [o["status"] for o in want] == ["converged", "breakdown", "converged"]
    _check_against_oracle(dev, B, X, hist, res, want, "u.r breakdown", maxiter=50)
    assert np.isnan(res[1].resid) and res[1].msg == b"breakdown dot(u,r)==0" and not np.any(X[:, 1])
    assert _same(X[:, 0], want[0]["soln"])
    x1, h1, r1 = dev.single(B[:, 1], maxiter=50)
    _result_same(res[1], r1, "psk_pcg's breakdown")
    n = 300
    Z = Dev(psk, sp.csr_matrix((n, n)), "identity")
    Bz = np.zeros((n, 2))
    Bz[:, 0] = np.random.default_rng(3).standard_normal(n)
    X, hist, res = Z.multi(Bz, maxiter=10)
    x1, h1, r1 = Z.single(Bz[:, 0], maxiter=10)
    assert res[0].status == Z.N.PSK_BREAKDOWN and res[0].msg == b"breakdown dot(p, Ap)==0" and res[0].iters == 0
    _result_same(res[0], r1, "zero matrix")
    assert not np.any(X) and res[1].exit == Z.N.PSK_EXIT_NONE
    _tail_untouched(hist, res, "zero matrix")


# ---- 4. against the single-vector solver and the reference ---------------------------------------------------------------
@pytest.mark.parametrize("prec", mo.PRECS)
@pytest.mark.parametrize("name", ["rand513", "fd17", "arrow1100"])
def test_against_psk_pcg_column_by_column(psk, name, prec):
    dev = Dev(psk, _matrix(name), prec)
    B = np.array(_columns(name))
    X, hist, res = dev.multi(B, maxiter=400)
    for j in range(4):
        b = B[:, j]
        x1, h1, r1 = dev.single(b, maxiter=400)
        assert (res[j].status, res[j].exit) == (r1.status, r1.exit), (name, prec, j)
        runs = [mo.pcg_multi(dev.A, b[:, None], dinv=dev.dinv, maxiter=400, tau=TAU, dot=d)[0] for d in mo.DOTS]
        if mo.counts_comparable(runs, TAU):
            assert res[j].iters == r1.iters == runs[0]["iters"], (name, prec, j, res[j].iters, r1.iters)
        nb = np.linalg.norm(b)
        true_multi = np.linalg.norm(b - dev.A @ X[:, j])
        true_single = np.linalg.norm(b - dev.A @ x1)
        print("%s %s col %d: iters %d / %d, true residual %.3e / %.3e (tau ||b|| = %.3e)"
              % (name, prec, j, res[j].iters, r1.iters, true_multi, true_single, TAU * nb))
        assert true_multi <= 2.0 * max(true_single, TAU * nb), (name, prec, j, true_multi, true_single)


@pytest.mark.parametrize("file", ["pcg_dh10_jacobi.npz", "pcg_fd64_jacobi.npz"])
def test_golden_right_hand_side_in_column_zero(psk, file):
    """the reference's golden run of this fixture, with exactly the bars tests/test_gpu_parity.py holds psk_pcg to
    (its _check_against_golden: iteration count, history, resid and solution), through solveMany"""
    from test_gpu_parity import _check_against_golden
    case = [c for c in solver_cases("pcg") if c["file"] == file][0]
    d = load_golden(file)
    A = golden_matrix(d)
    n = A.shape[0]
    B = np.random.default_rng(8).standard_normal((n, 3))
    B[:, 0] = d["b"]
    ctl = psk.CommonSolverArgs(maxiter=case["maxiter"], tau=case["tau"], failOnMaxiter=bool(case["fail_on_maxiter"]),
                               showIters=False, showFinal=False)
    sts = psk.PCG(control=ctl, precond=psk.Jacobi()).makeSolver().solveMany(A, B)
    assert len(sts) == 3
    _check_against_golden(sts[0], d, case)


# ---- 5. rules and refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fail", (True, False))
def test_maxiter_rules(psk, fail):
    dev = Dev(psk, _matrix("fd17"), "jacobi")
    B = np.array(_columns("fd17"))
    mi = 5
    X, hist, res = dev.multi(B, maxiter=mi, fail=fail)
    N = dev.N
    for j in range(4):
        x1, h1, r1 = dev.single(B[:, j], maxiter=mi, fail=fail)
        want = (N.PSK_MAXITER, 0, mi - 1, mi, N.PSK_EXIT_MAXITER) if fail else (N.PSK_CONVERGED, 1, mi, mi, N.PSK_EXIT_MAXITER)
        assert tuple(getattr(res[j], f) for f in FIELDS) == want == tuple(getattr(r1, f) for f in FIELDS), (j, fail)
        assert res[j].msg == r1.msg == (b"failure to converge" if fail else b"")
        assert res[j].resid == hist[j, mi - 1] == res[j].resid_recursive and np.all(np.isfinite(X[:, j]))
        assert res[j].spmv_launches == mi
    _tail_untouched(hist, res, "maxiter")
    # maxiter = 0: no iteration; x = 0, as psk_pcg reports it
    X, hist, res = dev.multi(B, maxiter=0, fail=fail)
    x1, h1, r1 = dev.single(B[:, 0], maxiter=0, fail=fail)
    _result_same(res[0], r1, "maxiter 0")
    assert not np.any(X) and res[0].spmv_launches == 0


def test_tau_zero_runs_to_maxiter_with_a_finite_history(psk):
    dev = Dev(psk, _matrix("rand513"), "identity")
    X, hist, res = dev.multi(np.array(_columns("rand513")), maxiter=12, tau=0.0, fail=True)
    for j in range(4):
        assert res[j].status == dev.N.PSK_MAXITER and res[j].hist_len == 12 and np.all(np.isfinite(hist[j]))
        assert np.all(np.isfinite(X[:, j]))


def test_refusals(psk):
    from pysolvers_amd import _native as N
    dev = Dev(psk, _matrix("fd17"), "identity")
    B = np.array(_columns("fd17"))
    for nrhs in (0, 5, -1):
        assert dev.multi_rc(B, nrhs=nrhs)[0] == N.PSK_ERR_ARG, nrhs
    ilu = Dev(psk, _matrix("fd17"), "ilu0")
    rc = ilu.multi_rc(B)[0]
    assert rc == N.PSK_ERR_UNSUPPORTED and b"preconditioner" in N.lib.psk_last_error()
    # X aliasing B
    ctl, res = dev.ctl(10, TAU, True), (N.PskResult * 4)()
    Bp = np.ascontiguousarray(B)
    assert N.lib.psk_pcg_multi(dev.dA.handle, None, 4, N.ptr(Bp), N.ptr(Bp), ctypes.byref(ctl), res, None,
                               N.PSK_HOST) == N.PSK_ERR_ARG
    # a matrix sharded over more than one rank (a dry communicator: no collectives needed to refuse)
    comm = psk.Linear.Communicator(2, 0, dry=True)
    dS = psk.Linear.fd_laplacian_2d_sharded(-1.0, 1.0, 17, comm)
    Bs = np.ones((dS.n, 2))
    Xs = np.empty_like(Bs)
    assert N.lib.psk_pcg_multi(dS.handle, None, 2, N.ptr(Bs), N.ptr(Xs), ctypes.byref(ctl), res, None,
                               N.PSK_HOST) == N.PSK_ERR_UNSUPPORTED
    assert b"sharded" in N.lib.psk_last_error()
    # a 1-D B in solveMany
    solver = psk.PCG(control=psk.CommonSolverArgs(showIters=False, showFinal=False)).makeSolver()
    with pytest.raises(AssertionError):
        solver.solveMany(dev.A, B[:, 0])


def _solve_many_matches_solve(psk, precond, A, B, capsys=None):
    ctl = psk.CommonSolverArgs(maxiter=300, tau=TAU, showIters=False, showFinal=False)
    sts = psk.PCG(control=ctl, precond=precond()).makeSolver().solveMany(A, B)
    assert len(sts) == B.shape[1]
    for j, st in enumerate(sts):
        b = np.ascontiguousarray(B[:, j])
        one = psk.PCG(control=ctl, precond=precond()).makeSolver().solve(A, b)
        assert st.success() and one.success() and st.msg() == one.msg(), j
        assert abs(st.iters() - one.iters()) <= 1, (j, st.iters(), one.iters())   # other dot orders: a threshold may fall
        L = min(len(st.info["hist"]), len(one.info["hist"]))                       # between the two histories
        assert L >= st.iters() - 1 and np.max(np.abs(st.info["hist"][:L] - one.info["hist"][:L])) <= 1e-10 * np.linalg.norm(b)
        assert st.resid() == st.info["hist"][-1]
        assert np.linalg.norm(b - A @ st.soln()) <= 2.0 * max(np.linalg.norm(b - A @ one.soln()), TAU * np.linalg.norm(b))
    return sts


def test_solve_many_six_columns_in_groups_of_four_and_two(psk):
    A = _matrix("rand513")
    B = np.random.default_rng(21).standard_normal((513, 6))
    B[:, 4] = 0.0                                     # a zero column in the second group
    ctl = psk.CommonSolverArgs(maxiter=300, tau=TAU, showIters=False, showFinal=False)
    sts = psk.PCG(control=ctl, precond=psk.Jacobi()).makeSolver().solveMany(A, B)
    assert len(sts) == 6 and sts[4].iters() == 1 and sts[4].resid() == 0 and not np.any(sts[4].soln())
    keep = [0, 1, 2, 3, 5]
    _solve_many_matches_solve(psk, psk.Jacobi, A, np.ascontiguousarray(B[:, keep]))
    # the second group's columns are what a call of their own gives: groups share nothing
    alone = psk.PCG(control=ctl, precond=psk.Jacobi()).makeSolver().solveMany(A, np.ascontiguousarray(B[:, 4:]))
    assert _same(alone[1].soln(), sts[5].soln()) and _same(alone[1].info["hist"], sts[5].info["hist"])


def test_solve_many_falls_back_for_ilu0(psk):
    A = _matrix("fd17")
    B = np.array(_columns("fd17")[:, :3])
    ctl = psk.CommonSolverArgs(maxiter=300, tau=TAU, showIters=False, showFinal=False)
    sts = psk.PCG(control=ctl, precond=psk.RightILU0()).makeSolver().solveMany(A, B)
    for j, st in enumerate(sts):
        one = psk.PCG(control=ctl, precond=psk.RightILU0()).makeSolver().solve(A, np.ascontiguousarray(B[:, j]))
        assert st.success() and st.iters() == one.iters() and _same(st.soln(), one.soln())   # the same code path
        assert _same(st.info["hist"], one.info["hist"])


def test_device_arrays_give_the_bits_of_host_arrays(psk):
    dev = Dev(psk, _matrix("rand257"), "jacobi")
    N = dev.N
    B = np.ascontiguousarray(_columns("rand257")[:, :3])
    X, hist, res = dev.multi(B)
    dB, dX = psk.DeviceVector.from_numpy(B.ravel()), psk.DeviceVector(B.size)
    res2 = (N.PskResult * 3)()
    hist2 = np.full_like(hist, SENTINEL)
    ctl = dev.ctl(200, TAU, True)
    N.check(N.lib.psk_pcg_multi(dev.dA.handle, dev.ph, 3, dB._p, dX._p, ctypes.byref(ctl), res2, N.ptr(hist2),
                                N.PSK_DEVICE), "psk_pcg_multi")
    assert _same(dX.numpy().reshape(B.shape), X) and _same(hist2, hist)
    for j in range(3):
        _result_same(res2[j], res[j], ("device", j))
    assert _same(dB.numpy(), B.ravel())               # B is only read


def test_a_solve_that_ends_at_the_init_leaves_no_stamp_and_psk_pcg_is_unchanged(psk):
    """all columns zero: the init raises the done stamp. The solves that follow, of either solver, on the same matrix
    (the workspace is shared) are bitwise what they were before; check_every = 1 polls after every iteration, where a
    stamp left behind would stop the loop early."""
    dev = Dev(psk, _matrix("rand513"), "jacobi")
    B = np.array(_columns("rand513"))
    x0, h0, r0 = dev.single(B[:, 0])
    m0 = dev.multi(B, check_every=1)
    X, hist, res = dev.multi(np.zeros_like(B))
    assert not np.any(X) and all(res[j].exit == dev.N.PSK_EXIT_NONE and res[j].iters == 1 for j in range(4))
    assert res[0].spmv_launches == 0
    _tail_untouched(hist, res, "zeros")
    m1 = dev.multi(B, check_every=1)
    assert _same(m1[0], m0[0]) and _same(m1[1], m0[1]) and m1[2][0].iters == m0[2][0].iters > 3
    x1, h1, r1 = dev.single(B[:, 0])
    assert _same(x1, x0) and _same(h1, h0)
    _result_same(r1, r0, "psk_pcg after the multi solves")


def test_forced_layouts_read_the_same_csr_arrays(psk):
    """the loop reads the plain CSR arrays whatever layout the SpMV uses: same bits under csr, sliced and diag"""
    A = _matrix("fd17")
    B = np.array(_columns("fd17"))
    ref = None
    for layout in ("csr", "sliced", "diag"):
        dev = Dev(psk, A, "jacobi", layout=layout)
        assert dev.dA.layout == layout
        got = dev.multi(B)
        ref = ref or got
        assert _same(got[0], ref[0]) and _same(got[1], ref[1])


# ---- 6. the last test of the file ---------------------------------------------------------------------------------
def test_no_gridsum_error_after_the_whole_file(psk):
    """every solve ends with gridsum_check, which reports an expired wait, a wrong grid or a ticket counter left
    non-zero by ANY earlier launch on the stream: one more solve of each kind after everything above"""
    dev = Dev(psk, _matrix("rand65537"), "jacobi")
    B = np.array(_columns("rand65537"))
    X, hist, res = dev.multi(B, maxiter=3, tau=0.0, fail=False)
    x, h, r = dev.single(B[:, 0], maxiter=3, tau=0.0, fail=False)
    assert all(res[j].iters == 3 for j in range(4)) and r.iters == 3
    worst = {}
    for (tag, kind), v in RATIOS.items():
        worst[kind] = max(worst.get(kind, 0.0), v)
    print("largest |device - exact| / dot_bound:", {k: "%.3g" % v for k, v in sorted(worst.items())})
