"""Smoothed-aggregation coarsening (SmoothedAggregation.py:13-229), O(nnz) host setup.

The reference's BuildAggregates is quadratic (phase 2 scans every aggregate for every remaining
node; 253 s at FD 512^2). Here aggregation and the filtered matrix come from
``psk_sa_aggregate`` (C++, pysolvers_amd/csrc/amg_aggregate.hip) with identical results, and the
remaining steps use the same scipy operations the reference uses, so P, R and every coarse operator are
bit-identical to the reference's (tests: oracle/amg.py is pinned against the reference; the CPU
tests check this module against oracle/amg.py).

``setup="device"`` builds the same operators in HBM: per level the matrix is taken on the host (the caller's for
the finest level, one download for each coarser one) for ``psk_sa_aggregate``, then ``psk_sa_prolongator``,
``psk_csr_transpose`` and two ``psk_csr_matmat`` products (pysolvers_amd/csrc/spgemm.hip) give P, R = P^T and
A_c = R (A P) — the same bits in the same stored entry order as the scipy path. A product the device refuses
(PSK_ERR_UNSUPPORTED: a row with more than PSK_SPGEMM_ROW_CAP products) is done by scipy instead (download,
multiply, upload) and counted in ``setup_stats["host_products"]``.
"""
import ctypes
import time

import numpy as np
import scipy.sparse as sp

from .. import _native as N
from .DeviceMatrix import DeviceCSR, matmat
from .MLHierarchy import MLHierarchy

SETUPS = ("host", "device")


def check_setup(setup):
    if setup not in SETUPS:
        raise ValueError("AMG setup must be 'host' or 'device', not %r" % (setup,))
    return setup


def default_tol(lvl):
    return 0.08 * (0.5) ** (lvl - 1)          # Vanek's default (:62-63)


class SmoothedAggregationMLHierarchy(MLHierarchy):
    """SmoothedAggregation.py:13-31. ``tol`` is stored and, as in the reference, not used: every
    level is coarsened with the default tolerance of its level number (SA_coarsen passes only
    lvl to BuildAggregates, :218)."""

    def __init__(self, A_fine, numLevels=2, tol=None, normalize=True, setup="host", device_A=None):
        """setup: "host" (scipy operators) or "device" (operators built in HBM, same bits). device_A: the
        DeviceCSR of A_fine when the caller already holds one (setup="device" uploads A_fine otherwise)."""
        check_setup(setup)
        super().__init__(numLevels=numLevels, normalize=normalize)
        self.tol = tol
        self.normalize = normalize
        self.setup = setup
        self.setup_stats["setup"] = setup
        self._setFineMatrix(sp.csr_matrix(A_fine))
        self._aggregates = [None] * numLevels
        if setup == "device":
            if device_A is None:
                t0 = time.perf_counter()
                device_A = DeviceCSR.from_scipy(self.matrix(numLevels - 1))
                self.setup_stats["seconds"]["transfer"] += time.perf_counter() - t0
            self._dev_ops[numLevels - 1] = device_A
            for lev in reversed(range(numLevels - 1)):
                self._coarsenOnDevice(lev)
            return
        for lev in reversed(range(numLevels - 1)):
            I_up = self.makeProlongator(lev)
            self._setUpdate(lev, I_up)

    def makeProlongator(self, lev):
        I_up, agg = SA_coarsen(self.matrix(lev + 1), tol=self.tol, lvl=lev + 1, times=self.setup_stats["seconds"])
        self.setup_stats["host_products"] += 1
        self._aggregates[lev] = agg
        return I_up

    def _coarsenOnDevice(self, lev):
        """Level lev from level lev + 1: P, R = P^T and A_lev = R (A_{lev+1} P) as DeviceCSR handles."""
        sec = self.setup_stats["seconds"]
        Ah = self.matrix(lev + 1)            # the caller's matrix, or one download (timed as transfer)
        dA = self._dev_ops[lev + 1]
        t0 = time.perf_counter()
        agg, count, afv = BuildAggregates(Ah, lvl=lev + 1)
        self._aggregates[lev] = agg
        t1 = time.perf_counter()
        dP = self._deviceProlongator(dA, Ah, agg, count, afv)
        t2 = time.perf_counter()
        dR = dP.transpose()
        t3 = time.perf_counter()
        dAP = self._deviceProduct(dA, dP)
        dAc = self._deviceProduct(dR, dAP)
        del dAP
        t4 = time.perf_counter()
        sec["aggregate"] += t1 - t0
        sec["prolongator"] += t2 - t1
        sec["transpose"] += t3 - t2
        sec["galerkin"] += t4 - t3
        self._dev_updates[lev], self._dev_downdates[lev], self._dev_ops[lev] = dP, dR, dAc

    def _deviceProlongator(self, dA, Ah, agg, count, afv):
        h = ctypes.c_void_p()
        rc = N.lib.psk_sa_prolongator(dA.handle, N.ptr(agg), count, N.ptr(afv), 2 / 3, N.PSK_HOST, ctypes.byref(h))
        if rc == N.PSK_ERR_UNSUPPORTED:      # a row over the product cap: scipy's lines, then one upload
            self.setup_stats["host_products"] += 1
            n = Ah.shape[0]
            Phat = sp.csr_matrix((np.ones(n), agg, np.arange(n + 1, dtype=np.int32)), shape=(n, count))
            Af = sp.csr_matrix((afv, Ah.indices.copy(), Ah.indptr.copy()), shape=Ah.shape)
            return DeviceCSR.from_scipy(SmoothProlongator(Phat, Ah, Af).tocsr(), rectangular=True)
        N.check(rc, "psk_sa_prolongator")
        self.setup_stats["device_products"] += 1
        return DeviceCSR._adopt(h, count)

    def _deviceProduct(self, dX, dY):
        try:
            C = matmat(dX, dY)
        except N.PskError as e:
            if e.code != N.PSK_ERR_UNSUPPORTED:
                raise
            self.setup_stats["host_products"] += 1   # download, multiply, upload
            return DeviceCSR.from_scipy(dX.to_scipy() * dY.to_scipy(), rectangular=True)
        self.setup_stats["device_products"] += 1
        return C


def BuildAggregates(A, lvl=1):
    """(agg, count, Af_values): aggregate index per node in the reference's list order, and the
    filtered matrix values (BuildAggregates :57-143 + BuildFilteredMatrix :157-183)."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    indptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(A.indices, dtype=np.int32)
    data = np.ascontiguousarray(A.data, dtype=np.float64)
    agg = np.empty(n, dtype=np.int32)
    afv = np.empty(data.shape[0], dtype=np.float64)
    count = ctypes.c_int64()
    N.check(N.lib.psk_sa_aggregate(n, N.ptr(indptr), N.ptr(indices), N.ptr(data), default_tol(lvl), N.ptr(agg),
                                   ctypes.byref(count), N.ptr(afv)), "psk_sa_aggregate")
    return agg, int(count.value), afv


def SmoothProlongator(Phat, A, Af, omega=(2 / 3)):
    """P = (I - omega D^-1 A_f) P_hat, elementwise in the reference's order (:185-205)."""
    S = omega * Af
    dA = A.diagonal()
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    v = S.data / dA[rows]
    S.data[:] = np.where(S.indices == rows, 1 - v, -v)
    return S.dot(Phat)


def SA_coarsen(A, tol=None, lvl=1, times=None):
    """(P, agg) for one level (:208-229); agg[i] = aggregate (coarse node) of fine node i. times: a dict whose
    "aggregate" and "prolongator" entries receive the seconds of the two steps."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    t0 = time.perf_counter()
    agg, count, afv = BuildAggregates(A, lvl=lvl)
    t1 = time.perf_counter()
    Phat = sp.csr_matrix((np.ones(n), agg, np.arange(n + 1, dtype=np.int32)), shape=(n, count))   # :145-155
    Af = sp.csr_matrix((afv, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    P = SmoothProlongator(Phat, A, Af).tocsr()
    if times is not None:
        times["aggregate"] += t1 - t0
        times["prolongator"] += time.perf_counter() - t1
    return P, agg
