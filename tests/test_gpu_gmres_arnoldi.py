"""GPU tests of the GMRES Arnoldi kernels on their own (gmres.hip: gm_start_kernel, gm_mgs_kernel,
gm_normalize_kernel with the device Givens code, gm_update_x_kernel), read through psk_lab_gmres_internals: the
basis Q, the unrotated and rotated Hessenberg columns, the rotations, g, y and the device state the last solve left
in the matrix's workspace. The measures are tests/gmres_oracle.py's, in np.longdouble, applied alike to the CPU
Arnoldi's arrays and to the device's.

Bars (written here, not inferred from the device):
(a) Arnoldi relation rho_k = ||A M^-1 q_k - Q[:, :k+2] H[:k+2, k]|| / ||A M^-1 q_k||: max_k on the device <= 4 x the
    largest max_k of the CPU Arnoldi under np.dot, math.fsum and 512-element chunk sums on the same case.
(b) omega = max_ij |q_i.q_j - delta_ij|: device <= 10 x the largest of the three CPU runs.
(c) every MGS dot: |h_jk - q_j.u_j| <= gamma_{n+2} |q_j|^T|u_j| and |h_{k+1,k}^2 - u.u| <= 2 gamma_{n+2} u.u, the u_j
    rebuilt in longdouble from the device's Q and H; gamma_m = m eps / (1 - m eps).
(d) the rotations: R, CS, g and the history are the bits krylov's Givens code gives on the device's own H and beta.
(f) x = [DInv] Q y to gamma_{m+1} |DInv| |Q||y| per component, R y = g to gamma_m |R||y| per component, and the last
    history entry against the host's ||b - A x|| to 1e-10 ||b||.
(g) exact Arnoldi breakdowns (every intermediate 0, +-1 or a power of two, one nonzero term per sum): history and x
    are krylov.gmres's bits.
(h) the steps the host enqueues behind convergence (its poll lags by two steps) leave the workspace untouched, and
    their number is the one that lag gives: spmv_launches, iters, hist_len, exit and status against krylov's solve
    where the cycle ends inside the lag, just past it, never, and in a later cycle; b = 0 enqueues no step, and the
    solve behind it repeats the bits of the one before.
psk_gmres never clears its basis or its rotations, so every solve here runs on a workspace psk_lab_gmres_prefill
zeroed: what is zero afterwards was not written.

Measured on an MI355X (device, largest of the three CPU orders, their ratio; every case takes the CPU runs' number
of steps):
    case      steps   max rho    oracle     ratio    omega      oracle     ratio
    rand511     23    3.684e-16  5.304e-16  0.69     2.989e-06  6.715e-06  0.45
    rand512     22    4.468e-16  5.770e-16  0.77     2.427e-06  4.157e-06  0.58
    rand513     22    3.067e-16  4.882e-16  0.63     1.008e-06  1.281e-05  0.08
    rand1025    22    5.405e-16  9.466e-16  0.57     1.347e-06  4.130e-06  0.33
    cd33        88    4.970e-16  5.012e-16  0.99     2.768e-06  1.279e-05  0.22
    dh8         55    5.246e-16  5.502e-16  0.95     7.592e-05  1.057e-04  0.72
    fd17        89    5.553e-16  5.798e-16  0.96     1.883e-15  2.142e-15  0.88   (last of 18 cycles of 5)
omega is taken over the built basis including q_{k+1} of the converging step, whose divisor h_{k+1,k} is tiny: that
column alone carries the 1e-6 to 1e-4 (the three CPU orders spread over a decade there).
(c) worst error / bound: 1.4e-2 for the h_jk, 1.8e-2 for the norms (both dh8). (d) holds bitwise as written: the
device's f64 sqrt and division round as numpy's do. (f) rand1025: 0.29 and 0.18 of the bounds; 1030 columns: 3.2e-3
and 1.0e-2, ||b - A x|| and the last history entry both 4.614333e-03 ||b||, loop_ms 2288 (533k launches).
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import bicgstab_oracle as bo
import cheby_oracle
import gmres_oracle as go
from conftest import GOLDEN
from oracle import fdlap, krylov

pytestmark = pytest.mark.gpu

TAU = 1e-10
MAXITER = 200
RTOL_RESID = 1e-10      # the project's solver-parity bar

# name -> preconditioner; the right-hand side is seeded by the name
CASES = {"rand511": "jacobi", "rand512": "jacobi", "rand513": "jacobi", "rand1025": "jacobi", "cd33": "identity",
         "dh8": "jacobi"}
FD17 = "fd17"           # Chebyshev(2), restart 5: the general-preconditioner and restarted path


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
    if name == "cd33":
        return bo.cd_matrix(33, 0.5)
    if name == "dh8":
        return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr()
    if name == FD17:
        return fdlap.fd_laplacian_2d(-1.0, 1.0, 17).tocsr()
    n = int(name[4:])
    return bo.random_nonsym(n, seed=n)


@functools.lru_cache(maxsize=None)
def _rhs(name):
    b = np.random.default_rng(len(name) + 17).standard_normal(_matrix(name).shape[0])
    b.setflags(write=False)
    return b


def _prec_kind(name):
    return "cheb" if name == FD17 else CASES[name]


@functools.lru_cache(maxsize=None)
def _minv(name):
    """M^-1 as the double-rounded operation the device applies."""
    A = _matrix(name)
    return {"jacobi": lambda: krylov.jacobi_form(A), "identity": lambda: krylov.identity_apply,
            "cheb": lambda: cheby_oracle.Chebyshev(A, degree=2)}[_prec_kind(name)]()


def _restart(name):
    return 5 if name == FD17 else 0


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The CPU Arnoldi under its three dot orders: (max rho, omega) of each run's last cycle, and the np.dot run's
    iteration count. Computed once, shared."""
    A, b, M = _matrix(name), _rhs(name), _minv(name)
    out = []
    for dot in bo.DOTS:
        s = go.solve(A, b, restart=_restart(name), maxiter=MAXITER, tau=TAU, precond=M, dot=dot)
        c = s["cycles"][-1]
        m = c["k"] + 1
        out.append((np.max(go.arnoldi_residuals(A, M, c["Q"], c["H"], m)), go.orthogonality(c["Q"], m + 1),
                    s["iters"], len(s["cycles"])))
    return out


class Device:
    """One matrix in HBM with its preconditioner, and psk_gmres / the lab view through the C ABI."""

    def __init__(self, psk, A, prec):
        from pysolvers_amd import _native as N
        self.N, self.lab = N, N.load_lab()
        self.A = A
        self.n = A.shape[0]
        self.dA = psk.DeviceCSR.from_scipy(A)
        self.prec = {"jacobi": psk.JacobiPreconditionerType, "identity": psk.IdentityPreconditionerType,
                     "cheb": lambda: psk.Chebyshev(degree=2)}[prec]().form(self.dA)
        self.ph = None if self.prec.device_kind == N.PSK_PREC_IDENTITY else self.prec.device_handle
        self.gen = 1 if prec == "cheb" else 0

    def solve(self, b, maxiter=MAXITER, tau=TAU, restart=0, fail=True, prefill=True):
        """(psk_result, x, the caller's history buffer: NaN wherever the solve wrote nothing)"""
        N = self.N
        self.key = (maxiter, restart)
        if prefill:
            N.check(self.lab.psk_lab_gmres_prefill(self.dA.handle, maxiter, restart, self.gen, 0), "prefill")
        ctl = N.PskCtl(maxiter=maxiter, tau=tau, fail_on_maxiter=int(fail), restart=restart, check_every=0,
                       time_kernels=0, norm_b=0.0)
        res = N.PskResult()
        hist = np.full(max(maxiter, 1), np.nan)
        bp = np.ascontiguousarray(b, dtype=np.float64)
        x = np.empty_like(bp)
        N.check(N.lib.psk_gmres(self.dA.handle, self.ph, N.ptr(bp), N.ptr(x), ctypes.byref(ctl), ctypes.byref(res),
                                N.ptr(hist), N.PSK_HOST), "psk_gmres")
        return res, x, hist

    def internals(self, cols=None):
        """dict(Q n x cols, H, R (K+1) x K, CS K x 2, g, y, done, brk, kconv, normB, tauNormB, rec) of the last
        solve."""
        N = self.N
        maxiter, restart = self.key
        K = max(1, restart if 0 < restart < maxiter else maxiter)
        cols = K + 1 if cols is None else cols
        Q = np.full((cols, self.n), np.nan)               # row j = column j of the basis
        H, R = np.full((K, K + 1), np.nan), np.full((K, K + 1), np.nan)
        CS, g, y, st = np.full((K, 2), np.nan), np.full(K + 1, np.nan), np.full(K + 1, np.nan), np.full(6, np.nan)
        N.check(self.lab.psk_lab_gmres_internals(self.dA.handle, maxiter, restart, self.gen, cols, N.ptr(Q), N.ptr(H),
                                                 N.ptr(R), N.ptr(CS), N.ptr(g), N.ptr(y), N.ptr(st)),
                "psk_lab_gmres_internals")
        return dict(Q=Q.T, H=H.T, R=R.T, CS=CS, g=g, y=y, done=int(st[0]), brk=int(st[1]), kconv=int(st[2]),
                    normB=st[3], tauNormB=st[4], rec=st[5], K=K)


_RUNS = {}


def _run(psk, name):
    """The case's solve and its workspace, once per module: (Device, result, x, history buffer, internals)."""
    if name not in _RUNS:
        dev = Device(psk, _matrix(name), _prec_kind(name))
        res, x, hist = dev.solve(_rhs(name), restart=_restart(name))
        w = dev.internals()
        for v in (x, hist, w["Q"], w["H"], w["R"], w["CS"], w["g"], w["y"]):
            v.setflags(write=False)
        assert res.success and res.status == 0 and res.exit == dev.N.PSK_EXIT_TOLERANCE, (name, res.msg)
        assert w["done"] == 1 and w["brk"] == 0
        assert res.iters >= 5 and res.hist_len == res.iters, (name, res.iters)   # no case degenerates silently
        assert res.iters == (res.iters - 1) // w["K"] * w["K"] + w["kconv"] + 1
        _RUNS[name] = (dev, res, x, hist, w)
    return _RUNS[name]


ALL = list(CASES) + [FD17]


@pytest.mark.parametrize("name", ALL)
def test_arnoldi_relation_and_orthogonality(psk, name):
    """(a), (b); for fd17 the last of at least three cycles (e)."""
    dev, res, x, hist, w = _run(psk, name)
    A, M = _matrix(name), _minv(name)
    m = w["kconv"] + 1
    ora = _oracle(name)
    if name == FD17:
        assert res.iters > 10 and all(o[3] >= 3 for o in ora)          # at least three cycles, device and oracle
    rho = np.max(go.arnoldi_residuals(A, M, w["Q"], w["H"], m))
    omega = go.orthogonality(w["Q"], m + 1)
    rho_o, omega_o = max(o[0] for o in ora), max(o[1] for o in ora)
    print("%s: iters %d (oracle %s)  rho %.3e  oracle %.3e  ratio %.2f | omega %.3e  oracle %.3e  ratio %.2f"
          % (name, res.iters, [o[2] for o in ora], rho, rho_o, rho / rho_o, omega, omega_o, omega / omega_o))
    assert rho <= 4 * rho_o, (name, rho, rho_o)
    assert omega <= 10 * omega_o, (name, omega, omega_o)


@pytest.mark.parametrize("name", ALL)
def test_every_mgs_dot_against_its_exact_value(psk, name):
    """(c)"""
    dev, res, x, hist, w = _run(psk, name)
    wh, wn = go.mgs_dot_errors(_matrix(name), _minv(name), w["Q"], w["H"], w["kconv"] + 1)
    print("%s: worst |h - q.u| / bound %.3e, worst |h^2 - u.u| / bound %.3e" % (name, wh, wn))
    assert wh <= 1 and wn <= 1, (name, wh, wn)


@pytest.mark.parametrize("name", ALL)
def test_givens_bitwise_from_the_device_hessenberg(psk, name):
    """(d): restart = 0 solves are one cycle from beta = normB; for fd17's last cycle R and CS only."""
    dev, res, x, hist, w = _run(psk, name)
    m = w["kconv"] + 1
    first = name != FD17
    R, CS, g, h = go.givens_replay(np.array(w["H"]), w["normB"] if first else None, m)
    for k in range(m):
        assert np.array_equal(_bits(w["R"][:k + 2, k]), _bits(R[:k + 2, k])), (name, k)
    assert np.array_equal(_bits(w["CS"][:m]), _bits(CS[:m])), name
    if first:
        assert np.array_equal(_bits(w["g"][:m + 1]), _bits(g[:m + 1])), name
        assert not w["g"][m + 1:].any()
        assert np.array_equal(_bits(hist[:m]), _bits(h)), name
        assert w["rec"] == hist[m - 1] and w["tauNormB"] == TAU * w["normB"] and w["normB"] == res.norm_b
        bl = np.asarray(_rhs(name), dtype=go.LD)           # gm_start_kernel: the square root of a dot of n terms
        assert abs(w["normB"] - np.sqrt(bl @ bl)) <= go.gamma(len(bl) + 2) * w["normB"]
        assert np.array_equal(_bits(w["Q"][:, 0]), _bits(_rhs(name) / w["normB"]))      # q_0 = b / beta


def _finalize_checks(name, A, w, x, m, dinv):
    ex = go.update_x_error(w["Q"], w["y"], x, m, dinv)
    et = go.triangular_error(w["R"], w["y"], w["g"], m)
    print("%s: m %d  |x - [DInv] Q y| / bound %.3e  |R y - g| / bound %.3e" % (name, m, ex, et))
    assert ex <= 1, (name, ex)
    assert et <= 1, (name, et)


def test_finalize_on_rand1025(psk):
    """(f), the cheap one: x against DInv (Q y), and R y = g."""
    dev, res, x, hist, w = _run(psk, "rand1025")
    A = _matrix("rand1025")
    _finalize_checks("rand1025", A, w, x, w["kconv"] + 1, np.reciprocal(A.diagonal()))
    assert np.linalg.norm(_rhs("rand1025") - A @ x) <= TAU * np.linalg.norm(_rhs("rand1025"))


def test_finalize_with_more_than_1024_basis_vectors(psk):
    """(f): 1030 columns; gm_update_x_kernel stages y[:1024] in LDS and reads the rest from HBM. The single slow
    case of this file."""
    n, maxiter = 1200, 1030
    A = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1], format="csr")
    b = np.random.default_rng(1).standard_normal(n)
    dev = Device(psk, A, "identity")
    res, x, hist = dev.solve(b, maxiter=maxiter, tau=1e-14, fail=False)
    print("tridiag1200: loop_ms %.1f, iters %d, hist[-1] / ||b|| %.3e" % (res.loop_ms, res.iters,
                                                                      hist[maxiter - 1] / np.linalg.norm(b)))
    assert res.success and res.exit == dev.N.PSK_EXIT_MAXITER and res.iters == maxiter - 1
    assert res.hist_len == maxiter and np.all(np.isfinite(hist))
    w = dev.internals(cols=maxiter)
    assert w["done"] == 0 and w["brk"] == 0
    _finalize_checks("tridiag1200", A, w, x, maxiter, None)
    nb = np.linalg.norm(b)
    true = np.linalg.norm(b - A @ x)
    print("tridiag1200: ||b - A x|| / ||b|| %.6e, hist[-1] / ||b|| %.6e" % (true / nb, hist[maxiter - 1] / nb))
    assert abs(true - hist[maxiter - 1]) <= RTOL_RESID * nb


# ---- (g) exact Arnoldi breakdowns --------------------------------------------------------------------------------

def _shift4():
    n, idx = 1025, [0, 511, 512, 1024]
    d = np.full(n, 2.0)
    d[idx] = 0.0
    A = (sp.diags(d) + sp.coo_matrix((np.ones(4), ([idx[(i + 1) % 4] for i in range(4)], idx)), shape=(n, n))).tocsr()
    A.eliminate_zeros()
    b = np.zeros(n)
    b[0] = 4.0
    return A, b


def test_breakdown_at_step_three_across_three_tiles(psk):
    A, b = _shift4()
    ref = krylov.gmres(A, b, maxiter=50, tau=1e-12)
    assert ref["success"] and ref["iters"] == 4 and np.array_equal(ref["hist"], [4.0, 4.0, 4.0, 0.0])
    dev = Device(psk, A, "identity")
    res, x, hist = dev.solve(b, maxiter=50, tau=1e-12)
    N = dev.N
    assert res.exit == N.PSK_EXIT_ARNOLDI_BREAKDOWN and res.success and res.status == N.PSK_CONVERGED
    assert res.iters == 4 and res.hist_len == 4 and res.resid == 0.0 and res.spmv_launches >= 4
    assert np.array_equal(_bits(hist[:4]), _bits(ref["hist"])) and np.all(np.isnan(hist[4:]))
    assert np.array_equal(_bits(x), _bits(ref["soln"])) and x[1024] == 4.0
    w = dev.internals()
    assert (w["done"], w["brk"], w["kconv"]) == (1, 1, 3)
    want = np.zeros((1025, 4))
    want[[0, 511, 512, 1024], [0, 1, 2, 3]] = 1.0
    assert np.array_equal(_bits(w["Q"][:, :4]), _bits(want))
    # neither the brk branch nor the steps enqueued behind it wrote a column
    assert not _bits(w["Q"][:, 4:]).any()
    assert not _bits(w["H"][:, 4:]).any() and not _bits(w["R"][:, 4:]).any()
    assert w["H"][4, 3] == 0.0 and w["H"][0, 3] == 1.0


def test_shift_under_gmres2_is_the_oracle_bit_for_bit(psk):
    """The step-3 case with restart = 2. GMRES(2) cannot leave b on a cyclic shift of order 4: every cycle returns
    dx = 0 and the solve runs its 25 cycles to maxiter with every history entry exactly 4 (tests/
    test_gmres_oracle_cpu.py); the cycle starts, the residual SpMV and the accumulating finalize stay exact."""
    A, b = _shift4()
    ref = krylov.gmres_restarted(A, b, 2, maxiter=50, tau=1e-12)
    dev = Device(psk, A, "identity")
    res, x, hist = dev.solve(b, maxiter=50, tau=1e-12, restart=2)
    N = dev.N
    assert not ref["success"] and not res.success and res.status == N.PSK_MAXITER and res.exit == N.PSK_EXIT_MAXITER
    assert res.iters == ref["iters"] == 49 and res.hist_len == 50
    assert np.array_equal(_bits(hist), _bits(ref["hist"]))
    assert np.array_equal(_bits(x), _bits(ref["soln"]))
    w = dev.internals()
    assert (w["done"], w["brk"]) == (0, 0)


def test_breakdown_at_step_zero_with_jacobi(psk):
    A = sp.diags(2.0 ** np.arange(-3, 4)).tocsr()
    b = np.zeros(7)
    b[5] = 3.0
    ref = krylov.gmres(A, b, maxiter=50, tau=1e-12, precond=krylov.jacobi_form(A))
    dev = Device(psk, A, "jacobi")
    res, x, hist = dev.solve(b, maxiter=50, tau=1e-12)
    assert res.exit == dev.N.PSK_EXIT_ARNOLDI_BREAKDOWN and res.success and res.iters == ref["iters"] == 1
    assert np.array_equal(_bits(hist[:1]), _bits(ref["hist"])) and hist[0] == 0.0 and res.hist_len == 1
    assert np.array_equal(_bits(x), _bits(ref["soln"])) and x[5] == 0.75
    w = dev.internals()
    assert (w["done"], w["brk"], w["kconv"]) == (1, 1, 0) and not _bits(w["Q"][:, 1:]).any()


@pytest.mark.parametrize("prec", ["identity", "jacobi"])
def test_one_by_one(psk, prec):
    A = sp.csr_matrix(np.array([[3.0]]))
    b = np.array([-2.0])
    M = krylov.jacobi_form(A) if prec == "jacobi" else krylov.identity_apply
    ref = krylov.gmres(A, b, maxiter=50, tau=1e-12, precond=M)
    dev = Device(psk, A, prec)
    res, x, hist = dev.solve(b, maxiter=50, tau=1e-12)
    assert res.exit == dev.N.PSK_EXIT_ARNOLDI_BREAKDOWN and res.success and res.iters == ref["iters"] == 1
    assert np.array_equal(_bits(hist[:1]), _bits(ref["hist"]))
    assert np.array_equal(_bits(x), _bits(ref["soln"])) and x[0] == b[0] / 3.0
    w = dev.internals()
    assert (w["done"], w["brk"], w["kconv"]) == (1, 1, 0) and w["Q"][0, 0] == -1.0 and not _bits(w["Q"][:, 1:]).any()


# ---- (h) steps launched after `done`; determinism ----------------------------------------------------------------

def test_steps_enqueued_behind_convergence_leave_no_trace(psk):
    dev, res, x, hist, w = _run(psk, "rand513")
    kc = w["kconv"]
    assert kc + 3 < w["K"]                                   # the host did enqueue steps behind step kc
    assert not _bits(w["Q"][:, kc + 2:]).any()
    assert not _bits(w["H"][:, kc + 1:]).any() and not _bits(w["R"][:, kc + 1:]).any()
    assert not _bits(w["CS"][kc + 1:]).any() and not w["g"][kc + 2:].any()
    assert res.hist_len == kc + 1 and np.all(np.isfinite(hist[:kc + 1])) and np.all(np.isnan(hist[kc + 1:]))
    assert w["rec"] == hist[kc]
    # a second solve on the same matrix: the same bits
    res2, x2, hist2 = dev.solve(_rhs("rand513"))
    assert res2.iters == res.iters
    assert np.array_equal(_bits(hist2[:kc + 1]), _bits(hist[:kc + 1])) and np.array_equal(_bits(x2), _bits(x))
    # ... and without the zeroed workspace (what the basis holds beforehand is never read)
    res3, x3, hist3 = dev.solve(_rhs("rand513"), prefill=False)
    assert np.array_equal(_bits(hist3[:kc + 1]), _bits(hist[:kc + 1])) and np.array_equal(_bits(x3), _bits(x))


def _diag7():
    A = sp.diags(2.0 ** np.arange(-3, 4)).tocsr()
    b = np.zeros(7)
    b[5] = 3.0
    return A, b


# name -> (system, preconditioner, maxiter, restart, tau, the exit taken); FD17 is _run's solve
HOST_LOOP = {"diag7_maxiter50": (_diag7, "jacobi", 50, 0, 1e-12, "ARNOLDI_BREAKDOWN"),   # kc = 0, inside the lag
             "diag7_maxiter2": (_diag7, "jacobi", 2, 0, 1e-12, "ARNOLDI_BREAKDOWN"),     # Kc < kc + 3
             "shift4": (_shift4, "identity", 50, 0, 1e-12, "ARNOLDI_BREAKDOWN"),         # kc = 3 = lag + 1
             "shift4_gmres2": (_shift4, "identity", 50, 2, 1e-12, "MAXITER"),            # 25 full cycles
             FD17: (lambda: (_matrix(FD17), _rhs(FD17)), "cheb", MAXITER, 5, TAU, "TOLERANCE")}


def _spmvs_enqueued(iters, converged, maxiter, restart):
    """The SpMVs psk_gmres enqueues. The host learns of `done` two steps late: a cycle of Kc steps that converged at
    its step kc enqueued min(Kc, kc + 3) Arnoldi SpMVs, any other cycle Kc; every restart cycle starts with the
    residual's SpMV, and a convergence exit ends with the true residual's."""
    K = max(1, restart if 0 < restart < maxiter else maxiter)
    if not converged:
        return maxiter + (maxiter + K - 1) // K - 1
    full, kc = divmod(iters - 1, K)
    return full * K + min(min(K, maxiter - full * K), kc + 3) + full + 1


@pytest.mark.parametrize("name", list(HOST_LOOP))
def test_host_loop_counts_and_the_done_stamp(psk, name):
    """What the host enqueued (spmv_launches) and reported, against krylov's solve; then b = 0 on the same matrix
    (no step, no SpMV), and the first solve again behind it: the same bits, so no stamp outlives its solve."""
    system, prec, maxiter, restart, tau, exit_name = HOST_LOOP[name]
    A, b = system()
    M = _minv(FD17) if prec == "cheb" else krylov.jacobi_form(A) if prec == "jacobi" else krylov.identity_apply
    ref = (krylov.gmres_restarted(A, b, restart, maxiter=maxiter, tau=tau, precond=M) if restart else
           krylov.gmres(A, b, maxiter=maxiter, tau=tau, precond=M))
    if name == FD17:
        dev, res, x, hist, _ = _run(psk, name)
    else:
        dev = Device(psk, A, prec)
        res, x, hist = dev.solve(b, maxiter=maxiter, tau=tau, restart=restart)
    N = dev.N
    want_exit = getattr(N, "PSK_EXIT_" + exit_name)
    want = _spmvs_enqueued(ref["iters"], want_exit != N.PSK_EXIT_MAXITER, maxiter, restart)
    print("%s: iters %d (oracle %d) hist_len %d exit %d status %d spmv_launches %d (formula %d)"
          % (name, res.iters, ref["iters"], res.hist_len, res.exit, res.status, res.spmv_launches, want))
    assert res.iters == ref["iters"] and res.hist_len == len(ref["hist"])
    assert res.exit == want_exit and bool(res.success) == ref["success"]
    assert res.status == (N.PSK_CONVERGED if ref["success"] else N.PSK_MAXITER)
    assert res.spmv_launches == want
    res0, x0, hist0 = dev.solve(np.zeros_like(b), maxiter=maxiter, tau=tau, restart=restart)
    assert (res0.spmv_launches, res0.iters, res0.hist_len) == (0, 1, 0)
    assert res0.success and res0.status == N.PSK_CONVERGED and res0.exit == N.PSK_EXIT_NONE and res0.norm_b == 0.0
    assert not x0.any() and np.all(np.isnan(hist0))
    res2, x2, hist2 = dev.solve(b, maxiter=maxiter, tau=tau, restart=restart)
    assert (res2.iters, res2.hist_len, res2.exit, res2.status, res2.spmv_launches) == \
        (res.iters, res.hist_len, res.exit, res.status, res.spmv_launches)
    assert np.array_equal(_bits(x2), _bits(x))
    assert np.array_equal(_bits(hist2[:res.hist_len]), _bits(hist[:res.hist_len]))


def test_every_kind_of_rhs_gives_the_same_bits(psk):
    import torch
    from pysolvers_amd.Linear import DeviceVector
    dev, res, x, hist, w = _run(psk, "rand513")
    b = _rhs("rand513")
    ctl = psk.CommonSolverArgs(showIters=False, showFinal=False, maxiter=MAXITER, tau=TAU)

    def solve(rhs):
        return psk.GMRES(control=ctl, precond=psk.JacobiPreconditionerType()).makeSolver().solve(_matrix("rand513"),
                                                                                                  rhs)
    host = solve(b)
    dv = solve(DeviceVector.from_numpy(b))
    tt = solve(torch.as_tensor(np.array(b), dtype=torch.float64, device="cuda"))
    assert isinstance(dv.soln(), DeviceVector) and tt.soln().is_cuda
    assert host.iters() == res.iters and np.array_equal(_bits(host.soln()), _bits(x))
    assert np.array_equal(_bits(host.info["hist"]), _bits(hist[:res.hist_len]))
    for st, xs in ((dv, dv.soln().numpy()), (tt, tt.soln().cpu().numpy())):
        assert st.iters() == host.iters()
        assert np.array_equal(_bits(st.info["hist"]), _bits(host.info["hist"]))
        assert np.array_equal(_bits(xs), _bits(host.soln()))


def test_lab_view_rejects_what_the_workspace_cannot_hold(psk):
    dev, res, x, hist, w = _run(psk, "dh8")
    N, lab = dev.N, dev.lab
    none = [None] * 7
    assert lab.psk_lab_gmres_internals(dev.dA.handle, MAXITER, 0, 0, MAXITER + 2, *none) == N.PSK_ERR_ARG   # cols > K+1
    assert lab.psk_lab_gmres_internals(dev.dA.handle, 10 * MAXITER, 0, 0, 1, *none) == N.PSK_ERR_ARG        # too small
    assert lab.psk_lab_gmres_internals(dev.dA.handle, MAXITER, 0, 0, 1, *none) == N.PSK_OK
