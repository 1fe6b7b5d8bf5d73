"""Multilevel hierarchy container (MLHierarchy.py:1-78): operators on the host (setup data).

Level 0 is the coarsest, numLevels-1 the finest. update(k) = I_up[k] maps level k to k+1,
downdate(k) = I_down[k] maps k+1 to k, matrix(k) = A[k] = I_down[k] (A[k+1] I_up[k]).

With ``setup="device"`` (SmoothedAggregationMLHierarchy) the operators are built in HBM and held as DeviceCSR
handles (device_matrix / device_update / device_downdate); matrix(k), update(k) and downdate(k) still return
scipy matrices: they download on first use and cache (the smoothers and the triangular-solve planner read them).
"""
import time
from abc import ABC, abstractmethod


class MLHierarchy(ABC):
    def __init__(self, numLevels=2, normalize=True):
        self._numLevels = numLevels
        self._ops = [None] * numLevels
        self._updates = [None] * numLevels
        self._downdates = [None] * numLevels
        self._normalize = normalize
        # device-built operators (setup="device"): DeviceCSR handles, None where the level lives on the host only
        self._dev_ops = [None] * numLevels
        self._dev_updates = [None] * numLevels
        self._dev_downdates = [None] * numLevels
        self.setup_stats = dict(setup="host", device_products=0, host_products=0,
                                seconds=dict(aggregate=0.0, prolongator=0.0, transpose=0.0, galerkin=0.0,
                                             transfer=0.0))

    @abstractmethod
    def makeProlongator(self, k):
        ...

    def numLevels(self):
        return self._numLevels

    def _host(self, host, dev, k):
        """host[k], downloaded from dev[k] on first use (counted as transfer time)."""
        if host[k] is None and dev[k] is not None:
            t0 = time.perf_counter()
            host[k] = dev[k].to_scipy()
            self.setup_stats["seconds"]["transfer"] += time.perf_counter() - t0
        return host[k]

    def update(self, k):
        return self._host(self._updates, self._dev_updates, k)

    def downdate(self, k):
        return self._host(self._downdates, self._dev_downdates, k)

    def matrix(self, k):
        return self._host(self._ops, self._dev_ops, k)

    def device_update(self, k):
        return self._dev_updates[k]

    def device_downdate(self, k):
        return self._dev_downdates[k]

    def device_matrix(self, k):
        return self._dev_ops[k]

    def _setUpdate(self, k, I_up):
        sec = self.setup_stats["seconds"]
        self._updates[k] = I_up
        t0 = time.perf_counter()
        self._downdates[k] = makeRestrictionOp(I_up, self._normalize)
        t1 = time.perf_counter()
        self._ops[k] = self._downdates[k] * (self._ops[k + 1] * self._updates[k])
        sec["transpose"] += t1 - t0
        sec["galerkin"] += time.perf_counter() - t1
        self.setup_stats["host_products"] += 2

    def _setFineMatrix(self, A_fine):
        self._ops[self._numLevels - 1] = A_fine


def makeRestrictionOp(I_up, normalize=True):
    """I_down = I_up^T (MLHierarchy.py:304-322), sorted columns, duplicates summed.

    The reference's optional row normalisation never reaches the returned matrix (it rescales a
    lil row VIEW whose __itruediv__ rebinds the view's lists, :316-319); measured on DH-8 the
    reference returns I_up^T exactly, so ``normalize`` is accepted and has the same (no) effect.
    """
    R = I_up.transpose(copy=True).tocsr()
    R.sum_duplicates()
    return R
