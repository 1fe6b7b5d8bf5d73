"""Host-only checks of the triangular-solve planner (plan_factor through psk_lab_trisolve_plan; no GPU):
which schedule a factor gets and the six cost-model estimates behind the choice. The device solves are
checked in tests/test_gpu_amg.py, tests/test_gpu_part.py and tests/test_gpu_parity.py."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from pysolvers_amd import _native as N

SCHEDULES = ("syncfree", "band", "lds", "grid", "part", "levels")   # enum TriSchedule (psk_internal.hpp)
NUM_CUS = 256
# waves of a sync-free launch on the MI355X: psk_lab_trisolve_workers' grid (workgroups) x 4
SYNCFREE_WAVES = 1792 * 4
LDS_MAX_ROWS = 18432     # kLdsMaxRows (trisolve.hpp)
INFO = ("levels", "band_K", "band_nblocks", "band_ring_words", "band_narrow", "grid_K", "grid_dict_n", "lv_steps")


def _stencil(w, H, offsets, diag):
    """Symmetric stencil on H lines of w positions, -1 off the diagonal."""
    n = w * H
    q = np.arange(n)
    y, x = q // w, q % w
    rows, cols = [], []
    for dy, dx in offsets:
        for sy, sx in ((dy, dx), (-dy, -dx)):
            yy, xx = y + sy, x + sx
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < H)
            rows.append(q[ok])
            cols.append((yy * w + xx)[ok])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return sp.csr_matrix((np.full(len(rows), -1.0), (rows, cols)), shape=(n, n)) + sp.diags(np.full(n, diag))


def _scattered_lower(n, k):
    """Lower factor with k off-diagonal entries per row (rows i < k: all i of them), one in each k-th of
    [0, i) at a hashed offset: a pattern without structure that is the same on every machine."""
    rows, cols = [], []
    for i in range(1, n):
        if i < k:
            c = np.arange(i)
        else:
            s, j = i // k, np.arange(k)
            c = j * s + (i * 7919 + j * j * 104729 + j * 131) % s
        rows.append(np.full(len(c), i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return sp.csr_matrix((-1.0 / (1 + (rows + cols) % 5), (rows, cols)), shape=(n, n)) + sp.diags(np.full(n, 4.0))


def _shapes():
    five = _stencil(96, 80, [(0, 1), (1, 0)], 4.0)
    nine = _stencil(64, 64, [(0, 1), (1, -1), (1, 0), (1, 1)], 8.0)
    chain = sp.diags([np.full(2000, 2.0), np.full(1999, -1.0)], [0, -1])
    return {"five_U": (sp.triu(five), True), "five_L": (sp.tril(five), False), "nine_U": (sp.triu(nine), True),
            "chain": (chain, False), "diagonal": (sp.diags(np.full(5000, 3.0)), False),
            "scattered": (_scattered_lower(3000, 12), False)}


SHAPES = {k: (sp.csr_matrix(T), up) for k, (T, up) in _shapes().items()}
STENCILS = ("five_U", "five_L", "nine_U")

# The parent of the commit that introduced plan_factor, on an MI355X: the line PSK_TRISOLVE_VERBOSE=1 prints
# at psk_prec_create_trisolve for each shape (estimates as printed, %.0f, in the order of SCHEDULES; chosen
# schedule). The planner is a refactor of that code: these must not move.
PINNED = {"five_U": ("169 7319 31 50 -1 60", "lds"), "five_L": ("169 7319 31 50 -1 60", "lds"),
          "nine_U": ("184 170 33 51 -1 62", "lds"), "chain": ("1940 1609 301 -1 -1 641", "lds"),
          "diagonal": ("1 3 0 -1 -1 9", "lds"), "scattered": ("85 -1 24 -1 -1 35", "lds")}


def plan(name, num_cus=NUM_CUS, waves=None):
    T, upper = SHAPES[name]
    rp = np.ascontiguousarray(T.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(T.indices, dtype=np.int32)
    va = np.ascontiguousarray(T.data, dtype=np.float64)
    sched, est, info = N.I32(), (N.F64 * 6)(), (N.I64 * 8)()
    N.check(N.load_lab().psk_lab_trisolve_plan(T.shape[0], N.ptr(rp), N.ptr(ci), N.ptr(va), 1 if upper else 0, 0, None,
                                               num_cus, SYNCFREE_WAVES if waves is None else waves,
                                               ctypes.byref(sched), est, info), "psk_lab_trisolve_plan")
    return sched.value, list(est), dict(zip(INFO, list(info)))


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for v in ("PSK_TRISOLVE_LEVELS", "PSK_TRISOLVE_PART", "PSK_TRISOLVE_GRID_DICT", "PSK_BAND_NARROW",
              "PSK_TRISOLVE_VERBOSE"):
        monkeypatch.delenv(v, raising=False)


def _longest_path(T, upper):
    """Rows on the longest dependency path of the factor (numpy, level by level)."""
    n = T.shape[0]
    rows = np.repeat(np.arange(n), np.diff(T.indptr))
    off = T.indices != rows
    r, c = rows[off], T.indices[off]
    lev = np.zeros(n, dtype=np.int64)
    while True:
        new = lev.copy()
        np.maximum.at(new, r, lev[c] + 1)
        if np.array_equal(new, lev):
            return int(lev.max()) + 1
        lev = new


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_levels_is_the_longest_dependency_path(name):
    T, upper = SHAPES[name]
    assert plan(name)[2]["levels"] == _longest_path(T, upper)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_eligibility(name):
    T, upper = SHAPES[name]
    n = T.shape[0]
    sched, est, info = plan(name)
    kmax = int(np.diff(T.indptr).max()) - 1
    assert est[0] >= 0
    if kmax > 8:
        assert est[1] == -1 and info["band_K"] == 0
    assert (est[2] >= 0) == (0 < n <= LDS_MAX_ROWS)
    assert (est[3] >= 0) == (name in STENCILS) and (info["grid_K"] > 0) == (name in STENCILS)
    if name == "scattered":
        assert kmax == 12 and est[3] == -1
    assert est[4] == -1   # the partitioned plan is attempted only above kLdsMaxRows rows
    assert all(e == -1 or e >= 0 for e in est)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_choice_is_the_smallest_eligible_estimate(name):
    """Candidates in the order sync-free, band, LDS, grid, levels, each taking over on a strictly smaller
    estimate: the first of the smallest in that order (no partitioned plan at these sizes)."""
    sched, est, _ = plan(name)
    order = [0, 1, 2, 3, 5]
    best = min((i for i in order if est[i] >= 0), key=lambda i: (est[i], order.index(i)))
    assert sched == best
    assert est[sched] == min(e for e in est if e >= 0)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_environment_forces_and_forbids(name, monkeypatch):
    base = plan(name)
    monkeypatch.setenv("PSK_TRISOLVE_LEVELS", "1")   # built and chosen whenever eligible
    sched, est, info = plan(name)
    assert est[5] >= 0 and sched == 5 and info["lv_steps"] > 0 and info["lv_steps"] % 8 == 0
    assert est[:5] == base[1][:5]
    monkeypatch.setenv("PSK_TRISOLVE_LEVELS", "0")   # never planned
    sched, est, info = plan(name)
    assert est[5] == -1 and sched != 5 and info["lv_steps"] == 0
    monkeypatch.delenv("PSK_TRISOLVE_LEVELS")
    monkeypatch.setenv("PSK_TRISOLVE_PART", "0")     # never planned
    sched, est, info = plan(name)
    assert est[4] == -1 and sched != 4 and (sched, est) == base[:2]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_plan_is_deterministic(name):
    a, b = plan(name), plan(name)
    assert a[0] == b[0] and a[2] == b[2]
    assert np.array_equal(np.array(a[1]).view(np.uint64), np.array(b[1]).view(np.uint64))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_pinned_to_the_parent(name):
    sched, est, _ = plan(name)
    want_est, want_sched = PINNED[name]
    assert ["%.0f" % e for e in est] == want_est.split()
    assert SCHEDULES[sched] == want_sched
