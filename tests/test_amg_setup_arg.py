"""The `setup` keyword of the AMG classes, on the CPU: a bad value raises ValueError before anything is built, and
setup="host" (the default) builds exactly the hierarchy the oracle pins (oracle/amg.hierarchy, itself pinned
against the reference's by test_amg_setup.py)."""
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

from conftest import GOLDEN
from oracle import amg


def _dh8():
    return sp.csr_matrix(scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr())


@pytest.mark.parametrize("bad", ["gpu", "Device", "", None, 1])
def test_bad_setup_raises_value_error(bad):
    import pysolvers_amd as psk
    from pysolvers_amd.Linear import AMGPreconditioner, SmoothedAggregationMLHierarchy
    A = sp.identity(4, format="csr")
    with pytest.raises(ValueError):
        psk.AMG(setup=bad)
    with pytest.raises(ValueError):
        AMGPreconditioner(A, setup=bad)
    with pytest.raises(ValueError):
        psk.AMGVCycle(setup=bad)
    with pytest.raises(ValueError):
        psk.AMGVCycleSolver(setup=bad)
    with pytest.raises(ValueError):
        SmoothedAggregationMLHierarchy(A, setup=bad)


def test_setup_is_passed_on():
    import pysolvers_amd as psk
    assert psk.AMG().setup == "host" and psk.AMG(setup="device").setup == "device"
    assert psk.AMGVCycle().setup == "host" and psk.AMGVCycleSolver().setup == "host"
    assert psk.AMGVCycle(setup="device").makeSolver().setup == "device"


def _same(X, Y):
    X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    assert X.shape == Y.shape
    assert np.array_equal(X.indptr, Y.indptr)
    assert np.array_equal(X.indices, Y.indices)
    assert np.array_equal(X.data.view(np.int64), Y.data.view(np.int64))


@pytest.mark.parametrize("L", [2, 3])
def test_host_setup_builds_the_oracle_hierarchy(L):
    from pysolvers_amd.Linear import SmoothedAggregationMLHierarchy
    A = _dh8()
    ops, P, R = amg.hierarchy(A, L)
    for h in (SmoothedAggregationMLHierarchy(A, numLevels=L), SmoothedAggregationMLHierarchy(A, numLevels=L, setup="host")):
        assert h.setup == "host" and h.setup_stats["setup"] == "host" and h.setup_stats["device_products"] == 0
        for k in range(L):
            _same(h.matrix(k), ops[k])
            assert h.device_matrix(k) is None
        for k in range(L - 1):
            _same(h.update(k), P[k])
            _same(h.downdate(k), R[k])
