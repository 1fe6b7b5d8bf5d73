"""PCG's staggered x flush (pcg_state.hpp): in the diagonal pair layout the deferred x updates are applied a block
of rows at a time by extra streaming workgroups of the in-loop SpMV launches, and K3 touches x only on the iteration
that ends the solve. The CSR layout of the same matrix keeps the uniform flush in K3, so diag against CSR compares
two paths; x and the residual history must agree bit for bit wherever the solve stops."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# FD sides: 529 rows (odd, 2 K3 tiles: more blocks than tiles), 2025 (odd: the tail element path), 10000, and
# 131769 (258 tiles, two-level gridsum)
SIDES = (23, 45, 100, 363)


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU visible to libpsk"
    return pysolvers_amd


@pytest.fixture(scope="module")
def stagger():
    from pysolvers_amd import _native as N
    s, ring = N.I32(), N.I32()
    N.check(N.load_lab().psk_lab_pcg_stagger(ctypes.byref(s), ctypes.byref(ring)), "psk_lab_pcg_stagger")
    assert 1 <= s.value < ring.value, "built without the staggered flush: diag and CSR would run the same path"
    return s.value, ring.value


_systems = {}


def _system(psk, m):
    """(scipy A, b, device A in the diagonal layout), built once per side."""
    if m not in _systems:
        from oracle import fdlap
        A = fdlap.fd_laplacian_2d(-1.0, 1.0, m)
        b = A @ np.random.default_rng(1000 + m).random(m * m)
        dA = psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m)
        assert dA.layout == "diag"
        # the two sides of every comparison below do take different paths
        assert _staggers(dA)
        dA.set_layout("csr")
        assert not _staggers(dA)
        dA.set_layout("diag")
        _systems[m] = (A, b, dA)
    return _systems[m]


def _staggers(dA):
    """psk_pcg's own choice for a Jacobi/identity solve of dA in its current layout (psk_lab_pcg_staggers)."""
    from pysolvers_amd import _native as N
    on = N.I32(-1)
    N.check(N.load_lab().psk_lab_pcg_staggers(dA.handle, None, ctypes.byref(on)), "psk_lab_pcg_staggers")
    assert on.value in (0, 1)
    return on.value == 1


def _ctl(psk, **kw):
    return psk.CommonSolverArgs(showIters=False, showFinal=False, **kw)


def _prec(psk, jac):
    return psk.Jacobi() if jac == "jacobi" else psk.IdentityPreconditionerType()


def _oracle_prec(A, jac):
    from oracle import krylov
    return krylov.jacobi_form(A) if jac == "jacobi" else krylov.identity_apply


@pytest.mark.parametrize("jac", ["identity", "jacobi"])
@pytest.mark.parametrize("m", SIDES)
def test_maxiter_sweep_diag_equals_csr_and_oracle(psk, stagger, m, jac):
    """maxiter 1 .. 2S+3 with tau = 0, failOnMaxiter both ways: every stop position within (and across) a period
    of the schedule, from solves that end before a block was ever stored to ones where every block was."""
    from oracle import krylov
    S, _ = stagger
    A, b, dA = _system(psk, m)
    for maxiter in range(1, 2 * S + 4):
        for fail in (True, False):
            ctl = _ctl(psk, maxiter=maxiter, tau=0.0, failOnMaxiter=fail)
            runs = {}
            for lay in ("diag", "csr"):
                dA.set_layout(lay)
                runs[lay] = psk.PCG(control=ctl, precond=_prec(psk, jac)).makeSolver().solve(dA, b)
            dA.set_layout("diag")
            d, c = runs["diag"], runs["csr"]
            tag = (m, jac, maxiter, fail)
            assert d.iters() == c.iters() and bool(d.success()) == bool(c.success()), tag
            assert np.array_equal(d.soln(), c.soln()), tag
            assert np.array_equal(d.info["hist"], c.info["hist"]), tag
            ref = krylov.pcg(A, b, maxiter=maxiter, tau=0.0, fail_on_maxiter=fail, precond=_oracle_prec(A, jac))
            assert d.iters() == ref["iters"] and bool(d.success()) == bool(ref["success"]), tag
            np.testing.assert_allclose(d.soln(), ref["soln"], rtol=1e-12, atol=1e-14, err_msg=str(tag))
            np.testing.assert_allclose(d.info["hist"], ref["hist"], rtol=1e-12, err_msg=str(tag))


@pytest.mark.parametrize("m", [45, 100])
def test_convergence_stop_inside_a_period(psk, stagger, m):
    """tau chosen so that the solve converges at iteration k for one k of every residue class mod S the oracle's
    history reaches: x equals the CSR layout's bit for bit, and a second solve on the same objects (the host's
    polling lag enqueues iterations past the stop both times; the workspace is reused) returns the same bits."""
    from oracle import krylov
    S, _ = stagger
    A, b, dA = _system(psk, m)
    nb = np.linalg.norm(b)
    hist = np.asarray(krylov.pcg(A, b, maxiter=4000, tau=1e-13, precond=krylov.jacobi_form(A))["hist"])
    picks = {}
    # iterations that undercut every earlier residual by a clear margin; class r takes its first one from 2 + 11 r
    # on, so the stops spread from the first period (blocks never stored yet) over a dozen later ones
    for k in range(2, len(hist)):
        lo = hist[:k].min()
        if hist[k] < lo * (1.0 - 1e-3) and k % S not in picks and k >= 2 + 11 * (k % S):
            picks[k % S] = (k, 0.5 * (hist[k] + lo) / nb)
    assert len(picks) == S, sorted(picks)
    assert any(k % S != 0 for k, _ in picks.values())
    for k, tau in sorted(picks.values()):
        ref = krylov.pcg(A, b, maxiter=4000, tau=tau, precond=krylov.jacobi_form(A))
        assert len(ref["hist"]) == k + 1
        ctl = _ctl(psk, maxiter=4000, tau=tau)
        sols = {}
        for lay in ("diag", "csr"):
            dA.set_layout(lay)
            s = psk.PCG(control=ctl, precond=psk.Jacobi()).makeSolver()
            st1 = s.solve(dA, b)
            st2 = s.solve(dA, b)
            assert st1.success() and st1.iters() == st2.iters() == ref["iters"], (m, k, lay)
            assert len(st1.info["hist"]) == k + 1
            assert np.array_equal(st1.soln(), st2.soln()), (m, k, lay)
            sols[lay] = st1.soln()
        dA.set_layout("diag")
        assert np.array_equal(sols["diag"], sols["csr"]), (m, k)
        np.testing.assert_allclose(sols["diag"], ref["soln"], rtol=1e-10, atol=1e-13)


def _flush_expected(x, ring, alphas, k, first_of_row):
    """numpy applying, row by row, the updates first .. k - 1 in iteration order (two roundings each)."""
    depth = ring.shape[0]
    out = x.copy()
    for f in np.unique(first_of_row):
        rows = first_of_row == f
        if f >= k:
            continue   # nothing pending: the rows keep the x they hold
        v = np.zeros(rows.sum()) if f == 0 else out[rows]
        for j in range(f, k):
            v = v + alphas[j] * ring[j % depth][rows]
        out[rows] = v
    return out


def _null_space_system(t):
    """A = I + the 4-neighbour adjacency of an m x m grid, m = 6t - 1 (all entries 1.0: the diagonal pair layout
    takes it), and b = v0 + v1 with A v0 = 0, A v1 = -v1: v0 = u0 (x) u1, v1 = u1 (x) u1 for the path's
    eigenvectors u0 = (1, 0, -1, 0, ...) (eigenvalue 0) and u1 = (1, -1, 0, 1, -1, 0, ...) (eigenvalue -1), whose
    squared norms are 3t and 4t. Unpreconditioned CG is then exact in float64 whatever the summation order (every
    sum is one of integers or of multiples of 1/16): alpha_0 = 28 t^2 / (-16 t^2) = -1.75, r_1 = v0 - 0.75 v1,
    beta_0 = 21 / 28 = 0.75, p_1 = 1.75 v0, A p_1 = 0 and dot(p_1, A p_1) == 0.0: a breakdown at k = 1 with
    iteration 0's x update still deferred."""
    import scipy.sparse as sp
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


@pytest.mark.parametrize("t", [1, 11, 21])
def test_breakdown_in_the_diagonal_layout_flushes_every_block(psk, stagger, t):
    """A dot(p, Ap) == 0 breakdown at k = 1 reached in the diagonal pair layout, through psk_pcg: SpMV launch 1
    has brought block 1 up to date, every other block still has iteration 0 pending and was never stored. The
    host's end-of-solve branch (per-block pending ranges, blocks that own no tile, pcg_flush_kernel) must return
    x_1 = 0 + alpha_0 p_0 = -1.75 b on every row, bit for bit, as the CSR layout's uniform flush does.
    n = 25 (one tile: six blocks own none), 4225 (9 tiles in 5 blocks), 15625 (31 tiles, all 7 blocks)."""
    from pysolvers_amd import _native as N
    from oracle import krylov
    A, b = _null_space_system(t)
    ref = krylov.pcg(A, b, maxiter=10, tau=1e-8)
    assert not ref["success"] and ref["iters"] == 1 and "p, Ap" in ref["msg"]
    dA = psk.DeviceCSR.from_scipy(A)
    assert dA.layout == "diag" and _staggers(dA)
    xs = {}
    for lay in ("diag", "csr"):
        dA.set_layout(lay)
        assert _staggers(dA) == (lay == "diag")
        ctl = N.PskCtl(maxiter=10, tau=1e-8, fail_on_maxiter=1, restart=0, check_every=0, time_kernels=0)
        res = N.PskResult()
        x = np.full(A.shape[0], np.nan)
        hist = np.full(10, np.nan)
        N.check(N.lib.psk_pcg(dA.handle, None, N.ptr(b), N.ptr(x), ctypes.byref(ctl), ctypes.byref(res), N.ptr(hist),
                              N.PSK_HOST), "psk_pcg")
        assert res.status == 2 and res.iters == 1, (lay, res.status, res.iters)   # PSK_BREAKDOWN at k = 1
        assert res.hist_len == 1 and hist[0] == ref["hist"][0]
        xs[lay] = x
    assert np.array_equal(xs["diag"], 0.0 + (-1.75) * b)
    assert np.array_equal(xs["diag"], xs["csr"])


@pytest.mark.parametrize("n", [529, 2025, 131769])
def test_breakdown_flush_kernel_per_block_ranges(psk, stagger, n):
    """pcg_flush_kernel at every later stop position, which no exact breakdown reaches end to end (the test above
    stops at k = 1): the kernel through the lab entry point on a random ring and alphas, k = 1 .. 2S+3. Every row
    ends at x with its own block's pending updates applied in order, bit for bit; also with the uniform rule of
    the paths that are not staggered. What is pending comes from replaying the launches, not from the schedule
    function."""
    from pysolvers_amd import _native as N
    S, depth = stagger
    rng = np.random.default_rng(n)
    ring = rng.standard_normal((depth, n))
    nv = (n + 511) // 512
    per = (nv + S - 1) // S
    blk = (np.arange(n) // 512) // per
    for k in range(1, 2 * S + 4):
        alphas = rng.standard_normal(k)
        x0 = rng.standard_normal(n)
        # replay: SpMV launch j = 1 .. k brought block j mod S up to date (iterations < j); 0: never stored
        upto = np.zeros(S, dtype=np.int64)
        for j in range(1, k + 1):
            upto[j % S] = j
        first = upto[blk]
        for stag, fr in ((1, first), (0, np.full(n, k - k % depth))):
            x = x0.copy()
            N.check(N.load_lab().psk_lab_pcg_flush(n, k, stag, N.ptr(x), N.ptr(np.ascontiguousarray(ring)),
                                                   N.ptr(alphas)), "psk_lab_pcg_flush")
            assert np.array_equal(x, _flush_expected(x0, ring, alphas, k, fr)), (n, k, stag)
