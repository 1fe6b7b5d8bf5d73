"""GPU tests of the device-side AMG setup (setup="device": SmoothedAggregation.py over psk_sa_prolongator,
psk_csr_transpose and psk_csr_matmat).

The bar is equality, written here and not inferred: every operator of the hierarchy has the indptr, indices and
data bit patterns of the host path's (setup="host", pinned against the oracle by the CPU tests), with no product
falling back to scipy, and therefore one preconditioner apply, a PCG+AMG solve and an AMGVCycle solve give the
same bits under both settings.
"""
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# (matrix, levels): the largest row of these hierarchies has 147 products (oracle/amg.py on the CPU), inside the cap
CASES = [("fd24", 3), ("fd48", 3), ("dh8", 2), ("dh8", 3)]


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    return pysolvers_amd


def _matrix(name):
    if name == "dh8":
        return sp.csr_matrix(scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr())
    from oracle import fdlap
    return sp.csr_matrix(-fdlap.fd_laplacian_2d(-1.0, 1.0, int(name[2:])))


@pytest.fixture(scope="module")
def hierarchies():
    """(host, device) hierarchies per case, built once and only read."""
    from pysolvers_amd.Linear import SmoothedAggregationMLHierarchy as H
    return {(name, L): (H(_matrix(name), numLevels=L, setup="host"), H(_matrix(name), numLevels=L, setup="device"))
            for name, L in CASES}


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def _same(X, Y):
    assert X.shape == Y.shape
    assert np.array_equal(X.indptr, Y.indptr)
    assert np.array_equal(X.indices, Y.indices)
    assert np.array_equal(_bits(X.data), _bits(Y.data))


@pytest.mark.parametrize("name,L", CASES)
def test_device_hierarchy_equals_host_bitwise(hierarchies, name, L):
    host, dev = hierarchies[(name, L)]
    assert dev.setup_stats["setup"] == "device" and host.setup_stats["setup"] == "host"
    assert dev.setup_stats["host_products"] == 0                  # no fallback
    assert dev.setup_stats["device_products"] == 3 * (L - 1)      # P, A P and R (A P) per coarse level
    assert host.setup_stats["device_products"] == 0
    for k in range(L):
        _same(dev.matrix(k), host.matrix(k))
    for k in range(L - 1):
        _same(dev.update(k), host.update(k))
        _same(dev.downdate(k), host.downdate(k))
        assert dev.device_update(k).ncols == host.update(k).shape[1]
    assert dev.matrix(0) is dev.matrix(0)                         # downloaded once, cached


def test_amg_apply_identical_bits(psk):
    A = _matrix("fd48")
    v = np.random.default_rng(5).standard_normal(A.shape[0])
    Mh = psk.AMG(numIters=2, numLevels=3).form(A)
    Md = psk.AMG(numIters=2, numLevels=3, setup="device").form(A)
    assert Md.setup == "device" and Md.mlh.setup_stats["host_products"] == 0
    assert Md._A[0] is Md.mlh.device_matrix(0) and Md._P[1] is Md.mlh.device_update(1)   # handed on, no re-upload
    assert np.array_equal(_bits(Md.apply(v)), _bits(Mh.apply(v)))


def test_pcg_amg_identical_bits(psk):
    A = _matrix("fd48")
    b = A @ np.random.default_rng(12345).random(A.shape[0])
    out = {}
    for setup in ("host", "device"):
        ctl = psk.CommonSolverArgs(maxiter=12, tau=1e-8, failOnMaxiter=False, showIters=False, showFinal=False)
        st = psk.PCG(control=ctl, precond=psk.AMG(numIters=2, numLevels=3, setup=setup)).makeSolver().solve(A, b)
        out[setup] = (st.iters(), _bits(st.info["hist"]), _bits(st.soln()))
    assert out["host"][0] == out["device"][0] and len(out["host"][1]) > 0
    assert np.array_equal(out["host"][1], out["device"][1])
    assert np.array_equal(out["host"][2], out["device"][2])


def test_vcycle_solver_identical_bits(psk):
    A = _matrix("dh8")
    b = A @ np.random.default_rng(2).random(A.shape[0])
    out = {}
    for setup in ("host", "device"):
        ctl = psk.CommonSolverArgs(maxiter=8, tau=1e-10, failOnMaxiter=False, showIters=False, showFinal=False)
        s = psk.AMGVCycle(ctl, numLevels=3, setup=setup).makeSolver()
        assert s.setup == setup
        st = s.solve(A, b)
        assert s._cycleMgr.setup == setup
        out[setup] = (st.iters(), _bits(st.info["hist"]), _bits(st.soln()))
    assert out["host"][0] == out["device"][0] and len(out["host"][1]) > 0
    assert np.array_equal(out["host"][1], out["device"][1])
    assert np.array_equal(out["host"][2], out["device"][2])
