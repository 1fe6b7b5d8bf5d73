"""GPU tests of the PCG kernels on their own (pcg.hip K0 / K2 / K3 / pcg_flush_kernel / the general path's kernels,
pcg_state.hpp, the SpMV layouts' dot epilogue and flush role), read through psk_lab_pcg_internals: r, the ring of p
buffers, Ap, u, x, alphas, udr, the history, the three grid sums and the device state the last solve left in the
matrix's workspace. The method is tests/pcg_replay.py's: given the device's own scalars every vector is replayed on the
host and must match BIT FOR BIT; every reduction is compared with the exact sum of the replayed terms within
dot_bound = (n - 1) 2^-53 sum|a_i c_i| (plus the half spacing of the exact value's own rounding, pcg_replay.check_sum).

Scalars: psk_pcg on host vectors with tau = 0, failOnMaxiter = 0 and maxiter = j for j = 1 .. K. The p.Ap sum run j
leaves behind is pTAp_{j-1}, which gives every alpha_k = udr[k] / pTAp_k, also where the kernels store none (the
stopping iteration; the general path). The runs must be bitwise prefixes of one another.

Which exact sum a grid sum is held to is read from its kernel (pcg_replay's docstring): rounded products for p.Ap and
for the Jacobi / identity init's b.b and u.r, unrounded products for K2's r.r and u.r, the general init's sums and
pcg_dot_kernel's u.r.

Depths come from the build's ring depth and flush period (psk_lab_pcg_stagger): with 8 and 7, K = 1, 2, 7, 8, 9, 16,
17 on the small shapes and 2, 9 on the 131k shapes.

No depth exceeds n (pcg_replay.depths): n = 1 runs K = 1 and n = 2 runs K = 1, 2.

Largest |device - exact| / dot_bound per case on an MI355X (a record, not a bar to tighten; the three forced layouts
of an FD case gave the same figures, as their sums are bit-identical):
    case                       p.Ap      r.r       u.r, udr  normB^2
    rand1 jacobi, identity     0         0         0         0
    rand2 jacobi, identity     0         0         0         1.78
    rand511 jacobi             3.36e-03  3.63e-03  3.27e-03  0
    rand511 identity           3.82e-03  3.52e-03  3.70e-03  0
    rand512 jacobi             3.70e-03  3.16e-03  3.11e-03  4.04e-03
    rand512 identity           3.23e-03  3.63e-03  3.63e-03  4.04e-03
    rand513 jacobi             3.58e-03  2.72e-03  2.59e-03  3.77e-03
    rand513 identity           2.95e-03  2.03e-03  4.28e-03  3.77e-03
    rand1025 jacobi            1.70e-03  1.20e-03  1.87e-03  9.78e-04
    rand1025 identity          1.77e-03  1.74e-03  1.74e-03  9.78e-04
    rand131072 jacobi          1.21e-05  8.33e-06  9.73e-06  7.64e-06
    rand131072 identity        1.01e-05  0         1.39e-05  7.64e-06
    rand131073 jacobi          1.20e-05  1.24e-05  1.50e-05  0
    rand131073 identity        1.11e-05  7.94e-06  1.19e-05  0
    fd17 jacobi (3 layouts)    4.09e-03  5.83e-03  6.58e-03  0
    fd17 identity              3.49e-03  3.57e-03  6.47e-03  0
    fd362 jacobi               9.34e-06  0         1.46e-05  7.64e-06
    fd362 identity             1.49e-05  0         8.21e-06  7.64e-06
    fd363 jacobi               7.42e-06  0         1.50e-05  0
    fd363 identity             8.76e-06  1.49e-05  1.50e-05  0
    fd17 cheb3                 5.28e-03  5.04e-03  6.68e-03  0
    fd17 ilu0                  3.76e-03  6.61e-03  5.63e-03  0
    rand513 cheb3              6.35e-03  4.37e-03  4.03e-03  0
    rand513 ilu0               3.70e-03  3.83e-03  3.62e-03  0
    rand131073 cheb3           1.31e-05  8.90e-06  1.35e-05  0
    rand131073 ilu0            1.23e-05  0         1.07e-05  0
Every sum is within 0.7% of its bound; the one figure above 1 is normB^2 at n = 2, where the bound is below one
spacing and squaring the rounded square root of a correct sum already costs more (_check_norm allows that, "one more
ulp"; the sum behind it, read as normB between the square roots of the bound's ends, is inside). On the CPU, np.dot
itself is 1.29 x the bound at n = 2 (tests/test_pcg_replay_cpu.py), which is why check_sum adds the exact value's own
half spacing. The whole file takes about 11 s.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import cheby_oracle
import pcg_replay as pr

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL_WORD = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU visible to libpsk"
    return pysolvers_amd


@functools.lru_cache(maxsize=None)
def _stagger():
    """(S, ring depth) of the build."""
    from pysolvers_amd import _native as N
    s, ring = N.I32(), N.I32()
    N.check(N.load_lab().psk_lab_pcg_stagger(ctypes.byref(s), ctypes.byref(ring)), "psk_lab_pcg_stagger")
    assert 0 <= s.value < ring.value
    return s.value, ring.value


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _same(a, c):
    return np.array_equal(_bits(a), _bits(c))


@functools.lru_cache(maxsize=None)
def _matrix(name):
    return pr.matrix(name)


@functools.lru_cache(maxsize=None)
def _rhs(name):
    b = pr.rhs(name)
    b.setflags(write=False)
    return b


class Device:
    """One matrix in HBM with its preconditioner, psk_pcg and the lab view through the C ABI."""

    def __init__(self, psk, A, prec, layout=None):
        from pysolvers_amd import _native as N
        self.N, self.lab = N, N.load_lab()
        self.A, self.n = A, A.shape[0]
        self.dA = psk.DeviceCSR.from_scipy(A)
        if layout is not None:
            self.dA.set_layout(layout)
            assert self.dA.layout == layout
        self.prec = {"jacobi": psk.JacobiPreconditionerType, "identity": psk.IdentityPreconditionerType,
                     "cheb3": lambda: psk.Chebyshev(degree=3), "ilu0": psk.RightILU0}[prec]().form(self.dA)
        self.ph = None if self.prec.device_kind == N.PSK_PREC_IDENTITY else self.prec.device_handle
        self.gen = 1 if prec in ("cheb3", "ilu0") else 0
        # the apply the replay uses: DInv as an array, the Chebyshev oracle (bitwise the device's, tests/
        # test_gpu_cheby.py), or, for ILU(0), whose triangular solves are not a bitwise function of the factor alone,
        # the device preconditioner's own applyRight (the PCG kernels are what is under test)
        self.host_apply = {"identity": lambda: None, "jacobi": lambda: np.reciprocal(A.diagonal()),
                           "cheb3": lambda: cheby_oracle.Chebyshev(A, degree=3),
                           "ilu0": lambda: (lambda v: np.array(self.prec.applyRight(np.array(v))))}[prec]()

    def staggers(self):
        on = self.N.I32(-1)
        self.N.check(self.lab.psk_lab_pcg_staggers(self.dA.handle, self.ph, ctypes.byref(on)), "psk_lab_pcg_staggers")
        return on.value == 1

    def solve(self, b, maxiter, tau=0.0, fail=False, check_every=0, prefill=False):
        N = self.N
        if prefill:
            N.check(self.lab.psk_lab_pcg_prefill(self.dA.handle, maxiter, self.gen, 1, FILL), "psk_lab_pcg_prefill")
        ctl = N.PskCtl(maxiter=maxiter, tau=tau, fail_on_maxiter=int(fail), restart=0, check_every=check_every,
                       time_kernels=0, norm_b=0.0)
        res = N.PskResult()
        hist = np.full(max(maxiter, 1), np.nan)
        bp = np.ascontiguousarray(b, dtype=np.float64)
        x = np.full_like(bp, np.nan)
        N.check(N.lib.psk_pcg(self.dA.handle, self.ph, N.ptr(bp), N.ptr(x), ctypes.byref(ctl), ctypes.byref(res),
                              N.ptr(hist), N.PSK_HOST), "psk_pcg")
        return res, x, hist

    def internals(self, maxiter):
        """What the last solve (host vectors, this maxiter) left: dict of arrays; NaN wherever nothing was copied."""
        N = self.N
        _, depth = _stagger()
        n = self.n
        w = dict(r=np.full(n, np.nan), ring=np.full((depth, n), np.nan), Ap=np.full(n, np.nan), u=np.full(n, np.nan),
                 x=np.full(n, np.nan), alphas=np.full(maxiter + 1, np.nan), udr=np.full(maxiter + 1, np.nan),
                 hist=np.full(maxiter + 1, np.nan), sums=np.full(3, np.nan), state=np.full(8, np.nan))
        N.check(self.lab.psk_lab_pcg_internals(self.dA.handle, maxiter, self.gen, 1, N.ptr(w["r"]), N.ptr(w["ring"]),
                                               N.ptr(w["Ap"]), N.ptr(w["u"]), N.ptr(w["x"]), N.ptr(w["alphas"]),
                                               N.ptr(w["udr"]), N.ptr(w["hist"]), N.ptr(w["sums"]), N.ptr(w["state"])),
                "psk_lab_pcg_internals")
        st = w.pop("state")
        w.update(done=int(st[0]), brk_kind=int(st[1]), iters=int(st[2]), resid=st[3], normB=st[4], tauNormB=st[5],
                 live=int(st[6]), x_written=int(st[7]))
        return w


def _prefix_runs(dev, b, K):
    """psk_pcg with maxiter = 1 .. K (tau = 0, failOnMaxiter = 0); the workspace and the returned x after each."""
    runs = []
    for j in range(1, K + 1):
        res, x, hist = dev.solve(b, maxiter=j)
        w = dev.internals(j)
        w["x_out"], w["hist_out"], w["res"] = x, hist, res
        runs.append(w)
    return runs


RATIOS = {}


def _note(tag, kind, ratio):
    row = RATIOS.setdefault(tag, {})
    row[kind] = max(row.get(kind, 0.0), ratio)


def _check_sum(tag, kind, value, exact, a, c):
    ok, ratio = pr.check_sum(value, exact, a, c)
    _note(tag, kind, ratio)
    assert ok, (tag, kind, value, exact, ratio)


def _check_norm(tag, kind, norm, exact, a, c):
    """A norm the device stores (normB, a history entry) is the correctly rounded square root of a grid sum: its
    square against the exact sum to one more ulp than a sum gets, and the norm itself inside the square roots of the
    bound's two ends (sqrt is monotone and correctly rounded on both sides)."""
    bound = pr.dot_bound(a, c)
    err = abs(norm * norm - exact)
    _note(tag, kind, err / bound if bound > 0 else 0.0)
    assert err <= bound + 1.5 * np.spacing(exact), (tag, kind, norm, exact)
    slack = bound + 0.5 * np.spacing(exact)                # what pcg_replay.check_sum allows the sum itself
    lo, hi = np.nextafter(exact - slack, -np.inf), np.nextafter(exact + slack, np.inf)
    assert np.sqrt(max(lo, 0.0)) <= norm <= np.sqrt(hi), (tag, kind, norm, exact)


def _check_case(dev, name, tag, b, depths):
    """Everything sections "scalars", "bitwise" and "reductions" ask of one matrix / preconditioner / layout."""
    S, depth = _stagger()
    A, n, gen = dev.A, dev.n, dev.gen
    Kmax = max(depths)
    runs = _prefix_runs(dev, b, Kmax)
    last = runs[-1]
    # ---- the runs stop where they were told to, and are bitwise prefixes of one another
    for j, w in enumerate(runs, start=1):
        assert (w["done"], w["brk_kind"], w["iters"], w["live"], w["x_written"]) == (1, 0, j, j - 1, 1), (tag, j)
        assert w["res"].iters == j and w["res"].hist_len == j and w["res"].success, (tag, j)
        assert _same(w["hist"][:j], last["hist"][:j]) and _same(w["hist_out"][:j], w["hist"][:j]), (tag, j)
        assert _same(w["udr"][:j], last["udr"][:j]), (tag, j)
        assert w["normB"] == last["normB"] and w["tauNormB"] == 0.0 and w["resid"] == w["hist"][j - 1], (tag, j)
        if not gen:
            assert _same(w["alphas"][:j - 1], last["alphas"][:j - 1]), (tag, j)
    pTAp = np.array([w["sums"][0] for w in runs])          # run j leaves p_{j-1}.Ap_{j-1}
    udr = last["udr"][:Kmax]
    assert np.all(np.isfinite(pTAp)) and np.all(pTAp != 0.0) and np.all(np.isfinite(udr)) and np.all(udr != 0.0), tag
    alphas = udr / pTAp                                     # :118, one rounding
    if not gen:                                             # stored by K3 of every iteration but the stopping one
        assert _same(last["alphas"][:Kmax - 1], alphas[:Kmax - 1]), tag
    rp = pr.replay(A, b, dev.host_apply, alphas, udr, Kmax)
    # ---- reductions that do not depend on the depth: the init's sums and every iteration's p.Ap and u.r
    init_dot = pr.exact_dot_fma if gen else pr.exact_dot   # pcg_gen_init2_kernel chains fma; K0 rounds its products
    _check_norm(tag, "normB2", last["normB"], init_dot(b, b), b, b)
    _check_sum(tag, "udr", udr[0], init_dot(rp["u"][0], rp["r"][0]), rp["u"][0], rp["r"][0])
    for k in range(Kmax):
        _check_sum(tag, "pAp", pTAp[k], pr.exact_dot(rp["p"][k], rp["Ap"][k]), rp["p"][k], rp["Ap"][k])
        if k >= 1:
            _check_sum(tag, "udr", udr[k], pr.exact_dot_fma(rp["u"][k], rp["r"][k]), rp["u"][k], rp["r"][k])
    # ---- after run K
    for K in depths:
        w = runs[K - 1]
        at = (tag, K)
        assert _same(w["r"], rp["r"][K]), at
        assert _same(w["Ap"], rp["Ap"][K - 1]), at                       # A p_{K-1}, scipy's bits
        assert _same(w["x"], rp["x"][K]) and _same(w["x_out"], rp["x"][K]), at
        if gen:
            assert _same(w["ring"][0], rp["p"][K - 1]), at               # p in place; the stopping K3 leaves it
            assert np.all(np.isnan(w["ring"][1:])), at
            assert _same(w["u"], rp["u"][K]), at                         # u = M.applyRight(r_K)
        else:
            for i in range(max(0, K - depth + 1), K):                    # every live p_i
                assert _same(w["ring"][i % depth], rp["p"][i]), (at, i)
            assert np.all(np.isnan(w["u"])), at                          # never stored on this path
        _check_sum(tag, "pAp", w["sums"][0], pr.exact_dot(rp["p"][K - 1], rp["Ap"][K - 1]), rp["p"][K - 1],
                   rp["Ap"][K - 1])
        rK, uK = rp["r"][K], rp["u"][K]
        rr = pr.exact_dot_fma(rK, rK)
        _check_sum(tag, "rr", w["sums"][1], rr, rK, rK)
        assert _same(w["hist"][K - 1], np.sqrt(w["sums"][1])), at        # self.norm(r): one correctly rounded sqrt
        _check_norm(tag, "hist2", w["hist"][K - 1], rr, rK, rK)
        _check_sum(tag, "udr", w["sums"][2], pr.exact_dot_fma(uK, rK), uK, rK)
    return runs, rp


def _fmt_row(tag):
    row = RATIOS.get(tag, {})
    return "%-26s %9.2e %9.2e %9.2e %9.2e" % (tag, row.get("pAp", 0), row.get("rr", 0), row.get("udr", 0),
                                              row.get("normB2", 0))


# ---- the elementwise (Jacobi / identity) paths -------------------------------------------------------------------

RAND = [("rand%d" % n, p) for n in pr.RAND_SMALL + pr.RAND_LARGE for p in ("jacobi", "identity")]


@pytest.mark.parametrize("name, prec", RAND)
def test_random_spd_vector_tile_edges_and_gridsum_geometry(psk, name, prec):
    """JAC = 1 (DInv streamed) and JAC = 0 on unsorted CSR rows; n = 513 and 1025 are the one-element odd tails of
    K0 / K2 / K3, 131072 the last one-level gridsum and 131073 the first two-level one, its last tile one element."""
    A, b = _matrix(name), _rhs(name)
    dev = Device(psk, A, prec)
    assert not dev.staggers()
    tag = "%s %s" % (name, prec)
    _check_case(dev, name, tag, b, pr.depths(A.shape[0], *_stagger()))
    print(_fmt_row(tag))


FD = [("fd%d" % m, p, lay) for m in pr.FD_SIDES for p in ("jacobi", "identity") for lay in ("diag", "csr", "sliced")]


@pytest.mark.parametrize("name, prec, layout", FD)
def test_stencil_layouts(psk, name, prec, layout):
    """JAC = 2 (one DInv value) and JAC = 0 with each SpMV layout forced: diag brings the init fused into the first
    SpMV, the pair-row SpMV's flush role and the staggered flush; csr and sliced keep K0 and the uniform flush."""
    S, _ = _stagger()
    A, b = _matrix(name), _rhs(name)
    dev = Device(psk, A, prec, layout=layout)
    assert dev.staggers() == (layout == "diag" and S > 0), (name, layout)
    tag = "%s %s %s" % (name, prec, layout)
    _check_case(dev, name, tag, b, pr.depths(A.shape[0], *_stagger()))
    print(_fmt_row(tag))


# ---- the general-preconditioner path (pcg_gen_*, pcg_dot_kernel) -------------------------------------------------

@pytest.mark.parametrize("name, prec", pr.GENERAL)
def test_general_preconditioner_kernels(psk, name, prec):
    A, b = _matrix(name), _rhs(name)
    dev = Device(psk, A, prec)
    assert dev.gen == 1 and not dev.staggers()
    tag = "%s %s" % (name, prec)
    _check_case(dev, name, tag, b, pr.depths(A.shape[0], *_stagger()))
    print(_fmt_row(tag))


# ---- stops other than maxiter -------------------------------------------------------------------------------------

def _fd45():
    from oracle import fdlap
    A = fdlap.fd_laplacian_2d(-1.0, 1.0, 45).tocsr()          # 2025 rows: 4 K3 tiles, an odd tail element
    return A, A @ np.random.default_rng(45).random(45 * 45)


@pytest.mark.parametrize("case", ["rand1025 uniform", "fd45 staggered"])
def test_tolerance_stop_inside_a_flush_period(psk, case):
    """tau set so that the solve stops at an iteration k with k mod ring not in {0, ring - 1}, check_every 1 and 16
    (the host then queues 2 and up to 47 iterations behind the stop): r, Ap, the live ring rows and x are the replay
    stopped at k, and nothing past the stop was written (the workspace was filled with 0xA5 first)."""
    S, depth = _stagger()
    if case.startswith("rand"):
        A, b = _matrix("rand1025"), _rhs("rand1025")
        dev = Device(psk, A, "jacobi")
        assert not dev.staggers()
    else:
        A, b = _fd45()
        dev = Device(psk, A, "jacobi", layout="diag")
        assert dev.staggers() == (S > 0)
    maxiter = 128
    # the device's own history picks the stop: the first k past the first flush period, strictly inside a period,
    # that undercuts every earlier residual by a clear margin
    _, _, h = dev.solve(b, maxiter=6 * depth)
    k = next(k for k in range(depth + 1, 6 * depth)
             if k % depth not in (0, depth - 1) and h[k] < 0.999 * h[:k].min())
    assert maxiter >= k + 3 * 16 + 2                       # room for everything check_every = 16 queues behind the stop
    tau = 0.5 * (h[k] + h[:k].min()) / np.linalg.norm(b)
    K = k + 1
    runs = _prefix_runs(dev, b, K)                          # the scalars, from maxiter stops
    pTAp = np.array([w["sums"][0] for w in runs])
    udr = runs[-1]["udr"][:K]
    rp = pr.replay(A, b, dev.host_apply, udr / pTAp, udr, K)
    for ce in (1, 16):
        res, x, hist = dev.solve(b, maxiter=maxiter, tau=tau, fail=True, check_every=ce, prefill=True)
        w = dev.internals(maxiter)
        at = (case, k, ce)
        assert res.success and res.exit == dev.N.PSK_EXIT_TOLERANCE and res.iters == K and res.hist_len == K, at
        assert (w["done"], w["brk_kind"], w["iters"], w["live"], w["x_written"]) == (1, 0, K, k, 1), at
        assert _same(w["hist"][:K], runs[-1]["hist"][:K]) and _same(w["udr"][:K], udr), at
        assert _same(w["alphas"][:k], (udr / pTAp)[:k]), at
        assert _same(w["r"], rp["r"][K]) and _same(w["Ap"], rp["Ap"][k]), at
        assert _same(w["x"], rp["x"][K]) and _same(x, rp["x"][K]), at
        for i in range(max(0, K - depth + 1), K):
            assert _same(w["ring"][i % depth], rp["p"][i]), (at, i)
        # the kernels queued behind `done` wrote nothing: no p_K over the oldest ring row, no scalar past the stop
        if K >= depth:
            assert _same(w["ring"][K % depth], rp["p"][K - depth]), at
        else:
            assert np.all(_bits(w["ring"][K % depth]) == FILL_WORD), at
        assert np.all(_bits(w["hist"][K:]) == FILL_WORD), at
        assert np.all(_bits(w["alphas"][k:]) == FILL_WORD), at
        assert np.all(_bits(w["udr"][K:]) == FILL_WORD), at
        assert w["sums"][0] == pTAp[k], at                  # no later SpMV published a sum either


def _null_space_system(t):
    """tests/test_gpu_pcg_stagger.py's: A = I + the 4-neighbour adjacency of an m x m grid (m = 6t - 1), b = v0 + v1
    with A v0 = 0 and A v1 = -v1. Every sum is one of integers: alpha_0 = -1.75, beta_0 = 0.75, p_1 = 1.75 v0 and
    dot(p_1, A p_1) == 0.0 exactly, whatever the summation order."""
    m = 6 * t - 1
    T = sp.diags([np.ones(m - 1), np.ones(m - 1)], [-1, 1])
    A = (sp.identity(m * m) + sp.kron(sp.identity(m), T) + sp.kron(T, sp.identity(m))).tocsr()
    A.sort_indices()
    i = np.arange(1, m + 1)
    u0 = np.round(np.sin(np.pi * i / 2))
    u1 = np.round(np.sin(2 * np.pi * i / 3) * 2 / np.sqrt(3))
    v0, v1 = np.outer(u0, u1).ravel(), np.outer(u1, u1).ravel()
    assert not (A @ v0).any() and np.array_equal(A @ v1, -v1)
    return A, v0 + v1


def _half_null_system(n3):
    """tests/test_gpu_parity.py's diag(2, 0, 0), b = (1, 1, 0), repeated n3 times over interleaved rows: alpha_0 = 1,
    r_1 = (-1, 1, 0), beta_0 = 1, p_1 = (0, 2, 0) lies in the null space and dot(p_1, A p_1) == 0.0; all sums are of
    integers."""
    d = np.tile([2.0, 0.0, 0.0], n3)
    A = sp.csr_matrix((d[::3], (np.arange(0, 3 * n3, 3), np.arange(0, 3 * n3, 3))), shape=(3 * n3, 3 * n3))
    return A, np.tile([1.0, 1.0, 0.0], n3)


@pytest.mark.parametrize("case", ["uniform", "staggered"])
def test_breakdown_leaves_r_and_flushes_x(psk, case):
    """dot(p, Ap) == 0 at k = 1 after one good iteration whose x update is still deferred: pcg_flush_kernel (the
    uniform rule on CSR rows over 4 tiles, the staggered one in the diagonal layout over 9 tiles in 5 blocks) returns
    the replay's x_1, and r is still r_1."""
    S, depth = _stagger()
    if case == "uniform":
        A, b = _half_null_system(600)
        dev = Device(psk, A, "identity")
        assert not dev.staggers()
    else:
        A, b = _null_space_system(11)
        dev = Device(psk, A, "identity", layout="diag")
        assert dev.staggers() == (S > 0)
    first = _prefix_runs(dev, b, 1)[0]                      # pTAp_0
    udr0, pTAp0 = first["udr"][0], first["sums"][0]
    maxiter = 10
    res, x, hist = dev.solve(b, maxiter=maxiter, tau=1e-8, fail=True, prefill=True)
    w = dev.internals(maxiter)
    assert res.status == dev.N.PSK_BREAKDOWN and res.exit == dev.N.PSK_EXIT_DOT_BREAKDOWN and res.iters == 1
    assert (w["done"], w["brk_kind"], w["iters"], w["live"]) == (2, 2, 1, 0) and res.hist_len == 1
    assert w["sums"][0] == 0.0 and w["udr"][0] == udr0 and w["alphas"][0] == udr0 / pTAp0
    rp = pr.replay(A, b, None, [udr0 / pTAp0], w["udr"][:2], 1)
    assert _same(w["r"], rp["r"][1]) and _same(w["ring"][0], rp["p"][0]) and _same(w["ring"][1 % depth], rp["p"][1])
    assert not (A @ rp["p"][1]).any() and not w["Ap"].any()           # A p_1 = 0: the breakdown is exact
    assert _same(w["x"], rp["x"][1]) and _same(x, rp["x"][1])
    assert _same(hist[:1], [np.sqrt(w["sums"][1])]) and np.all(_bits(w["hist"][1:]) == FILL_WORD)
    assert np.all(_bits(w["alphas"][1:]) == FILL_WORD) and np.all(_bits(w["udr"][2:]) == FILL_WORD)


# ---- the lab entry points themselves ------------------------------------------------------------------------------

def test_lab_view_rejects_what_the_workspace_cannot_hold(psk):
    A, b = _matrix("rand513"), _rhs("rand513")
    dev = Device(psk, A, "jacobi")
    N, lab, h = dev.N, dev.lab, dev.dA.handle
    none = [None] * 10
    assert lab.psk_lab_pcg_internals(None, 4, 0, 1, *none) == N.PSK_ERR_ARG
    dev.solve(b, maxiter=4)
    assert lab.psk_lab_pcg_internals(h, 4, 0, 1, *none) == N.PSK_OK
    assert lab.psk_lab_pcg_internals(h, 100000, 0, 1, *none) == N.PSK_ERR_ARG     # the scalar arrays would not fit
    assert lab.psk_lab_pcg_prefill(h, 4, 0, 1, 256) == N.PSK_ERR_ARG and lab.psk_lab_pcg_prefill(None, 4, 0, 1, 0) == N.PSK_ERR_ARG
    assert lab.psk_lab_pcg_prefill(h, 100000, 0, 1, FILL) == N.PSK_OK             # grows the buffers
    assert lab.psk_lab_pcg_internals(h, 100000, 0, 1, *none) == N.PSK_OK
