"""psk_pcg's host loop (pcg.hip: plan, init, iteration, finish, report; solve_loop.hpp StampPoll): neither the poll
chunk (ctl.check_every) nor the sampled timing (ctl.time_kernels: the 64-slot event ring, its harvest, the sharded
gather / halo samples) may show in a result, and the timing counts what psk.h says it counts."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIDES = (23, 100)   # 529 rows (two K3 tiles) and 10000


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU visible to libpsk"
    return pysolvers_amd


_systems = {}


def _system(psk, m):
    if m not in _systems:
        from oracle import fdlap
        A = fdlap.fd_laplacian_2d(-1.0, 1.0, m)
        b = A @ np.random.default_rng(1000 + m).random(m * m)
        dA = psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m)
        assert dA.layout == "diag"
        _systems[m] = (b, dA)
    return _systems[m]


def _pcg(h, M, b, **kw):
    """One psk_pcg call on host vectors: (x, hist, result)."""
    from pysolvers_amd import _native as N
    ctl = N.PskCtl(restart=0, **kw)
    res = N.PskResult()
    x = np.full(b.size, np.nan)
    hist = np.zeros(ctl.maxiter + 1)
    N.check(N.lib.psk_pcg(h, M, N.ptr(b), N.ptr(x), ctypes.byref(ctl), ctypes.byref(res), N.ptr(hist), N.PSK_HOST),
            "psk_pcg")
    return x, hist[:res.hist_len].copy(), res


def _jacobi(h, jac):
    from pysolvers_amd import _native as N
    M = ctypes.c_void_p()
    if jac == "jacobi":
        N.check(N.lib.psk_prec_create(h, N.PSK_PREC_JACOBI, ctypes.byref(M)), "jacobi")
    return M


def _same(a, b, tag):
    (xa, ha, ra), (xb, hb, rb) = a, b
    assert xa.tobytes() == xb.tobytes(), tag
    assert ha.tobytes() == hb.tobytes(), tag
    assert (ra.iters, ra.status, ra.exit, ra.success) == (rb.iters, rb.status, rb.exit, rb.success), tag
    assert np.float64(ra.resid).tobytes() == np.float64(rb.resid).tobytes(), tag


@pytest.mark.parametrize("stop", ["converge", "maxiter10"])
@pytest.mark.parametrize("lay", ["diag", "csr"])
@pytest.mark.parametrize("jac", ["identity", "jacobi"])
@pytest.mark.parametrize("m", SIDES)
def test_check_every_never_shows(psk, m, jac, lay, stop):
    from pysolvers_amd import _native as N
    b, dA = _system(psk, m)
    kw = dict(maxiter=4000, tau=1e-8, fail_on_maxiter=1) if stop == "converge" else \
        dict(maxiter=10, tau=1e-8, fail_on_maxiter=1)
    dA.set_layout(lay)
    try:
        M = _jacobi(dA.handle, jac)
        runs = [_pcg(dA.handle, M, b, check_every=C, time_kernels=0, **kw) for C in (1, 3, 7, 0) for _ in range(2)]
        if M:
            N.lib.psk_prec_destroy(M)
    finally:
        dA.set_layout("diag")
    r0 = runs[0][2]
    if stop == "converge":
        assert r0.success == 1 and r0.status == N.PSK_CONVERGED and 10 < r0.iters < 4000
        assert r0.hist_len == r0.iters
    else:
        assert r0.success == 0 and r0.status == N.PSK_MAXITER and r0.iters == 9 and r0.hist_len == 10
    for i, run in enumerate(runs[1:]):
        _same(runs[0], run, (m, jac, lay, stop, i + 1))


TIMED = dict(maxiter=150, tau=0.0, fail_on_maxiter=0, check_every=0)   # 150 samples at stride 1: the ring wraps twice


@pytest.mark.parametrize("lay", ["diag", "csr"])
@pytest.mark.parametrize("jac", ["identity", "jacobi"])
@pytest.mark.parametrize("m", SIDES)
def test_timing_never_shows_and_counts_its_samples(psk, m, jac, lay):
    from pysolvers_amd import _native as N
    b, dA = _system(psk, m)
    dA.set_layout(lay)
    try:
        M = _jacobi(dA.handle, jac)
        runs = {S: _pcg(dA.handle, M, b, time_kernels=S, **TIMED) for S in (0, 1, 4)}
        if M:
            N.lib.psk_prec_destroy(M)
    finally:
        dA.set_layout("diag")
    assert runs[0][2].iters == 150 and runs[0][2].hist_len == 150
    assert runs[0][2].spmv_launches == 0 and runs[0][2].spmv_ms == 0.0
    for S in (1, 4):
        _same(runs[0], runs[S], (m, jac, lay, S))
        res = runs[S][2]
        # the diagonal layout's iteration 0 runs its SpMV inside the fused init launch: not sampled
        assert res.spmv_launches == -(-150 // S) - (1 if lay == "diag" else 0), (m, jac, lay, S, res.spmv_launches)
        assert res.spmv_ms > 0.0
        assert res.gather_ms == 0.0 and res.halo_ms == 0.0 and res.comm_samples == 0


def test_sharded_timed_path_single_rank(psk):
    """The sharded loop through a real RCCL communicator of one rank (as test_gpu_shards'
    test_rccl_single_rank_pcg_matches_unsharded): every sampled iteration also times its p.Ap gather; with no
    peers no halo exchange is sampled."""
    from pysolvers_amd import _native as N
    m = 64
    n = m * m
    uid = (ctypes.c_uint8 * N.PSK_UNIQUE_ID_BYTES)()
    N.check(N.lib.psk_comm_unique_id(uid), "unique id")
    comm = ctypes.c_void_p()
    N.check(N.lib.psk_comm_init(1, 0, uid, ctypes.byref(comm)), "comm init")
    h = ctypes.c_void_p()
    rb, re = ctypes.c_int64(), ctypes.c_int64()
    N.check(N.lib.psk_csr_create_fd2d_dist(-1.0, 1.0, m, comm, ctypes.byref(h), ctypes.byref(rb), ctypes.byref(re)),
            "fd2d_dist")
    assert (rb.value, re.value) == (0, n)
    b = np.random.default_rng(7).random(n)
    M = _jacobi(h, "jacobi")
    runs = {S: _pcg(h, M, b, time_kernels=S, **TIMED) for S in (0, 4)}
    N.lib.psk_prec_destroy(M)
    N.lib.psk_csr_destroy(h)
    N.lib.psk_comm_destroy(comm)
    assert runs[0][2].iters == 150 and runs[0][2].comm_samples == 0
    _same(runs[0], runs[4], "sharded")
    res = runs[4][2]
    assert res.comm_samples == res.spmv_launches == -(-150 // 4)
    assert res.spmv_ms > 0.0
    assert res.halo_ms == 0.0
