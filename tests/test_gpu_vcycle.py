"""GPU tests of the standalone AMG V-cycle solver (AMGVCycle / AMGVCycleSolver, psk_vcycle).

Bars (written here, not inferred):
* against the reference's own runs (vcycle.npz, tests/golden/make_vcycle.py): iters, success, msg and the history
  length EQUAL on every case (the generator asserts every converging case keeps its residuals >= 5% away from the
  threshold); ||x - x_ref|| <= 1e-10 ||x_ref|| (the AMG bar of test_gpu_amg.py: only the triangular and coarse
  solves round differently and each cycle contracts); |hist_k - hist_ref_k| <= 1e-10 sqrt(||A||_1 ||A||_inf) ||x_ref||
  (dr = A dx, ||A||_2 <= sqrt(||A||_1 ||A||_inf)); the host's ||b - A x|| of the device's own x equals resid to
  1e-12 relative (the SpMV's bits; only the norm's summation order differs).
* against AMGPreconditioner.apply with tau = 0 (the same kernels, never an early exit): bitwise.
* check_every = 1 / default, run to run, and DeviceVector / CUDA-tensor right-hand sides: bitwise.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, golden_matrix, load_golden

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "manifest_vcycle.json")) as _f:
    MANIFEST = json.load(_f)
CASES = MANIFEST["cases"]


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    return pysolvers_amd


@pytest.fixture(scope="module")
def fix():
    return load_golden("vcycle.npz")


def _solver(psk, maxiter=60, tau=1e-10, fom=True, L=2, smoother="gs", show=False, name="AMGVCycle", **ctl_kw):
    ctl = psk.CommonSolverArgs(maxiter=maxiter, tau=tau, failOnMaxiter=fom, showIters=show, showFinal=show, **ctl_kw)
    kw = {"smoother": psk.JacobiSmoother} if smoother == "jacobi" else {}
    return psk.AMGVCycleSolver(ctl, numLevels=L, name=name, **kw)


def _negfd(m):
    from oracle import fdlap
    return -fdlap.fd_laplacian_2d(-1.0, 1.0, m)


def _bits(v):
    return np.asarray(v).view(np.uint64)


def _matrix(fix, name):
    """The fixture's matrix in its stored (unsorted) entry order, on arrays of its own: scipy sorts a matrix IN PLACE
    behind abs(A) and A.sum_duplicates(), and golden_matrix shares the module-wide fixture's arrays."""
    return golden_matrix({k: np.copy(v) for k, v in fix.items() if k.startswith(name + "_") and v.ndim <= 1
                          and k[len(name) + 1:] in ("n", "data", "indices", "indptr")}, prefix=name + "_")


def _hist_bar(A, x_ref):
    """1e-10 sqrt(||A||_1 ||A||_inf) ||x_ref||, from the stored entries (A itself is left as it is)."""
    a = np.abs(A.data)
    n1 = np.bincount(A.indices, weights=a, minlength=A.shape[1]).max()
    ninf = np.add.reduceat(a, A.indptr[:-1])[np.diff(A.indptr) > 0].max()
    return 1e-10 * np.sqrt(n1 * ninf) * np.linalg.norm(x_ref)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_matches_reference(psk, fix, case):
    tag, name = case["tag"], case["matrix"]
    A, b = _matrix(fix, name), fix[name + "_b"]
    st = _solver(psk, maxiter=case["maxiter"], tau=case["tau"], fom=case["fail_on_maxiter"], L=case["num_levels"],
                 smoother=case["smoother"]).solve(A, b)
    hist, hist_ref, x_ref = st.info["hist"], fix[tag + "_hist"], fix[tag + "_soln"]
    assert st.iters() == case["iters"] == int(fix[tag + "_iters"])
    assert bool(st.success()) == case["success"]
    assert st.msg() == case["msg"]
    assert len(hist) == case["hist_len"] == len(hist_ref)
    x = st.soln()
    ex = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    bar = _hist_bar(A, x_ref)
    eh = np.max(np.abs(hist - hist_ref))
    r = np.linalg.norm(b - A @ x)
    print("%s: x_rel=%.3e hist_abs=%.3e (bar %.3e) resid=%.6e host=%.6e" % (tag, ex, eh, bar, st.resid(), r))
    assert ex <= 1e-10
    assert eh <= bar
    assert abs(r - st.resid()) <= 1e-12 * st.resid()
    assert st.resid() == hist[-1]
    if case["converged"]:
        assert r < case["tau"] * np.linalg.norm(b)


# ---------------------------------------------------------------------------------------------
def _tridiag(n):
    return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()


@pytest.mark.parametrize("what,L,k", [("fd128", 3, 1), ("fd128", 3, 3), ("fd512", 4, 2), ("tri145", 2, 2)])
def test_bitwise_against_the_preconditioner_apply(psk, what, L, k):
    """maxiter = k, tau = 0, no failure runs exactly the k cycles AMGPreconditioner(numIters=k, tau=0).apply runs,
    through the same kernels. -FD 512^2 L=4: the paired Gauss-Seidel launch has several bands there and
    vc_check_kernel spans 1024 blocks in 64 ticket groups; -FD 128^2: 64 blocks; n = 145: one block, partial."""
    from pysolvers_amd.Linear import AMGPreconditioner
    A = _tridiag(145) if what == "tri145" else _negfd(int(what[2:]))
    b = np.random.default_rng(k + L).standard_normal(A.shape[0])
    y = AMGPreconditioner(A, numIters=k, numLevels=L, tau=0.0).apply(b)
    st = _solver(psk, maxiter=k, tau=0.0, fom=False, L=L).solve(A, b)
    assert st.success() and st.iters() == k - 1 and len(st.info["hist"]) == k
    assert np.array_equal(_bits(st.soln()), _bits(y))


def test_bitwise_partial_last_block(psk):
    """n = 300^2 = 351 blocks of 256 and a partial one, more blocks than ticket groups, groups of unequal size."""
    from pysolvers_amd.Linear import AMGPreconditioner
    A = _negfd(300)
    b = np.random.default_rng(300).standard_normal(A.shape[0])
    y = AMGPreconditioner(A, numIters=2, numLevels=3, tau=0.0).apply(b)
    st = _solver(psk, maxiter=2, tau=0.0, fom=False, L=3).solve(A, b)
    assert np.array_equal(_bits(st.soln()), _bits(y))


# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fd128():
    """-FD 128^2, 3 levels, tau = 1e-10 by the oracle loop (spsolve Gauss-Seidel, as the reference), computed once."""
    from vcycle_oracle import vcycle_solve
    A = _negfd(128)
    b = np.random.default_rng(5).standard_normal(A.shape[0])
    ref = vcycle_solve(A, b, num_levels=3, maxiter=60, tau=1e-10, tri=False)
    margin = np.min(np.abs(ref["hist"] / (1e-10 * np.linalg.norm(b)) - 1.0))
    assert ref["success"] and margin >= 0.05, margin   # the count cannot flip on rounding
    return A, b, ref


def test_snapshot_not_a_later_iterate(psk, fd128):
    A, b, ref = fd128
    s = _solver(psk, L=3)
    s.freezeMatrix()
    st = s.solve(A, b)
    assert st.success() and st.iters() == ref["iters"] and len(st.info["hist"]) == ref["iters"]
    # the converging cycle's x: one more cycle would contract the error against the oracle's x by the cycle's rate,
    # and ||b - A x|| of the returned x is the reported, converged residual
    assert np.linalg.norm(st.soln() - ref["soln"]) <= 1e-10 * np.linalg.norm(ref["soln"])
    r = np.linalg.norm(b - A @ st.soln())
    assert abs(r - st.resid()) <= 1e-12 * st.resid() and st.resid() == st.info["hist"][-1]
    # the polling interval and lag never show: check_every = 1, 3, 7 and the default, and a second run, same bits
    for ce in (1, 3, 7, 0):
        s.check_every = ce
        st2 = s.solve(A, b)
        assert st2.iters() == st.iters(), ce
        assert np.array_equal(_bits(st2.soln()), _bits(st.soln())), ce
        assert np.array_equal(_bits(st2.info["hist"]), _bits(st.info["hist"])), ce
        assert st2.resid() == st.resid()


def test_device_and_tensor_rhs_same_bits(psk, fd128):
    import torch
    A, b, ref = fd128
    s = _solver(psk, L=3)
    s.freezeMatrix()
    st = s.solve(A, b)
    sd = s.solve(A, psk.DeviceVector.from_numpy(b))
    assert isinstance(sd.soln(), psk.DeviceVector)
    assert np.array_equal(_bits(sd.soln().numpy()), _bits(st.soln())) and sd.iters() == st.iters()
    tb = torch.as_tensor(b, device="cuda")
    stt = s.solve(A, tb)
    assert isinstance(stt.soln(), torch.Tensor) and stt.soln().is_cuda
    assert np.array_equal(_bits(stt.soln().cpu().numpy()), _bits(st.soln())) and stt.iters() == st.iters()
    assert np.array_equal(_bits(stt.info["hist"]), _bits(st.info["hist"]))
    # a DeviceCSR matrix too
    sm = _solver(psk, L=3).solve(psk.DeviceCSR.from_scipy(A), b)
    assert np.array_equal(_bits(sm.soln()), _bits(st.soln()))


# ---------------------------------------------------------------------------------------------
def test_zero_rhs(psk, fix):
    A = _matrix(fix, "dh8")
    s = _solver(psk)
    st = s.solve(A, np.zeros(A.shape[0]))
    z = MANIFEST["zero_rhs"]
    assert st.iters() == z["iters"] and st.success() == z["success"] and st.resid() == z["resid"]
    assert not np.any(st.soln()) and s._cycleMgr is None        # returned before the hierarchy is built
    sd = s.solve(A, psk.DeviceVector.from_numpy(np.zeros(A.shape[0])))
    assert sd.iters() == 1 and not np.any(sd.soln().numpy())


def test_zero_rhs_in_the_library(psk, fix):
    """psk_vcycle itself: b = 0 gives x = 0, iters 1, exit NONE, no history; then a solve on the same handle."""
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import AMGPreconditioner
    A, b = _matrix(fix, "negfd16"), fix["negfd16_b"]
    M = AMGPreconditioner(A, numIters=1, tau=0.0)
    n = A.shape[0]
    for rhs, want_iters, want_exit in ((np.zeros(n), 1, N.PSK_EXIT_NONE), (b, 11, N.PSK_EXIT_TOLERANCE)):
        ctl = N.PskCtl(maxiter=60, tau=1e-10, fail_on_maxiter=1)
        res, x, hist = N.PskResult(), np.full(n, 7.0), np.zeros(60)
        N.check(N.lib.psk_vcycle(M.device_handle, N.ptr(rhs), N.ptr(x), ctypes.byref(ctl), ctypes.byref(res),
                                 N.ptr(hist), 0, N.PSK_HOST), "psk_vcycle")
        assert (res.status, res.success, res.iters, res.exit) == (N.PSK_CONVERGED, 1, want_iters, want_exit)
        assert res.hist_len == (0 if want_exit == N.PSK_EXIT_NONE else want_iters)
        assert (res.spmv_ms, res.gather_ms, res.halo_ms, res.comm_samples) == (0.0, 0.0, 0.0, 0)
        if want_exit == N.PSK_EXIT_NONE:
            assert not np.any(x) and res.resid == 0.0
    ctl = N.PskCtl(maxiter=0, tau=1e-10, fail_on_maxiter=1)
    assert N.lib.psk_vcycle(M.device_handle, N.ptr(b), N.ptr(x), ctypes.byref(ctl), ctypes.byref(res), None, 0,
                            N.PSK_HOST) == N.PSK_ERR_ARG


# ---- psk_vcycle's host loop: check_every, the number of cycles enqueued, the stamp's generation ----------------
VC_LAG = 1   # kVcLag (vcycle.hip): the poll reads the stamp behind the event VC_LAG chunks back


def _raw(M, b, maxiter=60, check_every=0):
    """One psk_vcycle call on host vectors, tau = 1e-10: (x, hist, result)."""
    from pysolvers_amd import _native as N
    ctl = N.PskCtl(maxiter=maxiter, tau=1e-10, fail_on_maxiter=1, restart=0, check_every=check_every, time_kernels=0,
                   norm_b=0.0)
    res, x, hist = N.PskResult(), np.full(b.size, 7.0), np.zeros(maxiter)
    N.check(N.lib.psk_vcycle(M.device_handle, N.ptr(b), N.ptr(x), ctypes.byref(ctl), ctypes.byref(res), N.ptr(hist),
                             0, N.PSK_HOST), "psk_vcycle")
    return x, hist[:res.hist_len].copy(), res


def _cycles_enqueued(c, C, maxiter):
    """res.spmv_launches of a solve whose cycle c converged, polled in chunks of C cycles (StampPoll::step): in
    front of cycle k = j C the host waits for the event behind chunk j - 1 - VC_LAG, which covers the cycles below
    (j - VC_LAG) C, and stops when the stamp c + 2 is at most (j - VC_LAG) C + 1. So k is the least j C with
    j >= VC_LAG + 1 and c + 2 <= (j - VC_LAG) C + 1, and never more than maxiter."""
    j = VC_LAG + 1
    while c + 2 > (j - VC_LAG) * C + 1:
        j += 1
    return min(j * C, maxiter)


def _same(a, b, tag):
    (xa, ha, ra), (xb, hb, rb) = a, b
    assert np.array_equal(_bits(xa), _bits(xb)), tag
    assert np.array_equal(_bits(ha), _bits(hb)), tag
    assert (ra.iters, ra.status, ra.exit, ra.success, ra.hist_len) == (rb.iters, rb.status, rb.exit, rb.success,
                                                                       rb.hist_len), tag
    assert _bits(np.float64(ra.resid)) == _bits(np.float64(rb.resid)), tag


@pytest.mark.parametrize("what,L", [("fd128", 3), ("tri145", 2)])
def test_check_every_shows_only_in_the_cycles_enqueued(psk, fd128, what, L):
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import AMGPreconditioner
    if what == "fd128":
        A, b, ref = fd128
    else:
        A, b, ref = _tridiag(145), np.random.default_rng(145).standard_normal(145), None
    M = AMGPreconditioner(A, numIters=1, numLevels=L, tau=0.0)
    runs = {C: _raw(M, b, check_every=C) for C in (1, 2, 5)}
    r1 = runs[1][2]
    assert (r1.status, r1.success, r1.exit) == (N.PSK_CONVERGED, 1, N.PSK_EXIT_TOLERANCE)
    assert 2 <= r1.iters < 60 and r1.hist_len == r1.iters and (ref is None or r1.iters == ref["iters"])
    for C in (1, 2, 5):
        _same(runs[1], runs[C], (what, C))
        got, want = runs[C][2].spmv_launches, _cycles_enqueued(r1.iters - 1, C, 60)
        print("%s check_every %d: cycle %d converged, %d enqueued (rule %d)" % (what, C, r1.iters - 1, got, want))
        assert got == want, (what, C, got, want)
    # the cap: maxiter = the converging cycle + 2, below what a chunk of 5 would enqueue
    capped = _raw(M, b, maxiter=r1.iters + 1, check_every=5)
    _same(runs[1], capped, (what, "capped"))
    assert capped[2].spmv_launches == _cycles_enqueued(r1.iters - 1, 5, r1.iters + 1) == r1.iters + 1


def test_a_zero_solve_leaves_no_stamp_behind(psk, fd128):
    """b = 0 stores the stamp 1 under its own generation: the fd128 solve directly after it gives the bits it gave
    before, and enqueues the same number of cycles."""
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import AMGPreconditioner
    A, b, ref = fd128
    M = AMGPreconditioner(A, numIters=1, numLevels=3, tau=0.0)
    first = _raw(M, b)
    assert first[2].iters == ref["iters"] and first[2].exit == N.PSK_EXIT_TOLERANCE
    zero = _raw(M, np.zeros(b.size))
    assert (zero[2].exit, zero[2].iters, zero[2].spmv_launches) == (N.PSK_EXIT_NONE, 1, 0) and not np.any(zero[0])
    after = _raw(M, b)
    _same(first, after, "after b = 0")
    assert after[2].spmv_launches == first[2].spmv_launches


def test_maxiter_one(psk, fix):
    from vcycle_oracle import vcycle_solve
    A, b = _matrix(fix, "negfd16"), fix["negfd16_b"]
    ref = vcycle_solve(A, b, maxiter=1, tau=1e-10, fail_on_maxiter=True)
    for fom in (True, False):
        st = _solver(psk, maxiter=1, fom=fom).solve(A, b)
        assert st.iters() == 0 and bool(st.success()) == (not fom) and len(st.info["hist"]) == 1
        assert st.msg() == ("failure to converge" if fom else None)
        assert np.linalg.norm(st.soln() - ref["soln"]) <= 1e-10 * np.linalg.norm(ref["soln"])
        bar = _hist_bar(A, ref["soln"])
        assert abs(st.resid() - ref["resid"]) <= bar


def test_freeze_matrix_reuses_the_hierarchy(psk, fix):
    A, b = _matrix(fix, "negfd16"), fix["negfd16_b"]
    s = _solver(psk)
    s.solve(A, b)
    h1 = s._cycleMgr
    s.solve(A, b)
    assert s._cycleMgr is not h1 and h1 is not None            # unfrozen: rebuilt (VCycleSolver.py:71)
    s.freezeMatrix()
    h2 = s._cycleMgr
    st = s.solve(A, b)
    assert s._cycleMgr is h2 and st.iters() == 11


def test_custom_norm_is_host_driven(psk, fix):
    from vcycle_oracle import vcycle_solve

    def inf_norm(v):
        return np.linalg.norm(v, np.inf)
    A, b = _matrix(fix, "negfd32"), fix["negfd32_b"]
    ref = vcycle_solve(A, b, maxiter=60, tau=1e-10, norm=inf_norm)
    margin = np.min(np.abs(ref["hist"] / (1e-10 * inf_norm(b)) - 1.0))
    assert ref["success"] and margin >= 0.05, margin
    st = _solver(psk, norm=inf_norm).solve(A, b)
    assert st.success() and st.iters() == ref["iters"] and st.info["host_driven"]
    assert len(st.info["hist"]) == len(ref["hist"])
    assert np.linalg.norm(st.soln() - ref["soln"]) <= 1e-10 * np.linalg.norm(ref["soln"])
    assert st.resid() == inf_norm(b - A @ st.soln())
    # the same cycles as the device loop runs: x after k host-driven cycles == the device loop's x after k
    k = st.iters()
    dev = _solver(psk, maxiter=k, tau=0.0, fom=False).solve(A, b)
    assert np.array_equal(_bits(dev.soln()), _bits(st.soln()))


def test_non_amg_handle_is_refused(psk, fix):
    from pysolvers_amd import _native as N
    A, b = _matrix(fix, "negfd16"), fix["negfd16_b"]
    M = psk.Jacobi().form(psk.DeviceCSR.from_scipy(A))
    ctl, res, x = N.PskCtl(maxiter=5, tau=1e-8, fail_on_maxiter=1), N.PskResult(), np.zeros_like(b)
    with pytest.raises(N.PskError) as e:
        N.check(N.lib.psk_vcycle(M.device_handle, N.ptr(b), N.ptr(x), ctypes.byref(ctl), ctypes.byref(res), None, 0,
                                 N.PSK_HOST), "psk_vcycle")
    assert e.value.code == N.PSK_ERR_ARG


def test_show_iters_prints_the_reference_lines(psk, fix, capsys):
    p = MANIFEST["printed"]
    case = next(c for c in CASES if c["tag"] == p["tag"])
    A, b = _matrix(fix, case["matrix"]), fix[case["matrix"] + "_b"]
    ctl = psk.CommonSolverArgs(maxiter=case["maxiter"], tau=case["tau"], failOnMaxiter=case["fail_on_maxiter"])
    psk.AMGVCycle(ctl, numLevels=case["num_levels"]).makeSolver().solve(A, b)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if " iter=" in ln or " solve " in ln]
    assert lines == p["lines"]
    psk.AMGVCycle(ctl, numLevels=case["num_levels"]).makeSolver(name="vc").solve(A, b)
    named = [ln for ln in capsys.readouterr().out.splitlines() if " iter=" in ln or " solve " in ln]
    assert named == ["vc" + ln for ln in p["lines"]]
