"""CPU tests of the multi-column PCG oracle (tests/pcg_multi_oracle.py), of the inputs tests/test_gpu_pcg_multi.py relies
on, and of the lab layout probe for solver id 6 (no GPU).

* Every column of pcg_multi equals oracle.krylov.pcg on that column alone, bit for bit, under the same dot function:
  x, history, iters, status. oracle.krylov.pcg calls np.dot and its `norm` argument; for the other two dot orders its
  module-level numpy is replaced by a proxy whose dot is the order under test (and norm = sqrt(dot(v, v))), so the very
  same reference lines run.
* The mixed-stopping inputs really stop their columns at different iterations, the breakdown input really breaks down,
  and no history entry of a case whose counts the GPU test compares lies within the dot spread of its threshold
  (counts_comparable).
* psk_lab_solver_layout(6, ...): the regions psk_pcg_multi carves, recomputed here from the sizes alone, in the style
  of tests/test_solver_layout.py.
"""
import ctypes
import itertools
import math
import types

import numpy as np
import pytest

import pcg_multi_oracle as mo
from oracle import fdlap, krylov

TAU = 1e-8


class _NumpyWithDot(types.ModuleType):
    """numpy, except dot"""

    def __init__(self, dot):
        super().__init__("numpy_with_dot")
        self._dot = dot

    def __getattr__(self, name):
        return getattr(np, name)

    def dot(self, a, b):
        return self._dot(a, b)


def _single(monkeypatch, A, b, dinv, dot, **kw):
    """oracle.krylov.pcg on one column with the given dot order"""
    with monkeypatch.context() as mp:
        if dot is not mo.dot_numpy:
            mp.setattr(krylov, "np", _NumpyWithDot(dot))
        prec = krylov.identity_apply if dinv is None else (lambda v: np.multiply(dinv, v))
        return krylov.pcg(A, b, precond=prec, norm=lambda v: math.sqrt(dot(v, v)), **kw)


def _same_bits(a, c):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(c, dtype=np.float64).view(np.uint64))


def _assert_column_is_single(monkeypatch, A, B, dinv, dot, **kw):
    got = mo.pcg_multi(A, B, dinv=dinv, dot=dot, **kw)
    for j, g in enumerate(got):
        ref = _single(monkeypatch, A, np.ascontiguousarray(B[:, j]), dinv, dot, **kw)
        assert g["success"] == ref["success"] and g["iters"] == ref["iters"] and g["msg"] == ref["msg"], (j, g, ref)
        assert _same_bits(g["hist"], ref["hist"]), j
        assert (g["soln"] is None) == (ref["soln"] is None), j
        if ref["soln"] is not None:
            assert _same_bits(g["soln"], ref["soln"]), j
        if ref["resid"] is None:
            assert g["resid"] is None
        else:
            assert _same_bits([g["resid"]], [ref["resid"]]), j
    return got


@pytest.mark.parametrize("dot", mo.DOTS, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", ["rand2", "rand257", "fd17", "arrow1100"])
@pytest.mark.parametrize("prec", mo.PRECS)
def test_every_column_is_the_single_vector_oracle(monkeypatch, name, prec, dot):
    A = mo.matrix(name)
    dinv = np.reciprocal(A.diagonal()) if prec == "jacobi" else None
    B = mo.columns(name)
    _assert_column_is_single(monkeypatch, A, B, dinv, dot, maxiter=400, tau=TAU)
    for fail in (True, False):
        _assert_column_is_single(monkeypatch, A, B, dinv, dot, maxiter=3, tau=0.0, fail_on_maxiter=fail)
    _assert_column_is_single(monkeypatch, A, B[:, :1], dinv, dot, maxiter=0, tau=TAU)


@pytest.mark.parametrize("dot", mo.DOTS, ids=lambda d: d.__name__)
def test_mixed_stopping_columns_stop_at_different_iterations(monkeypatch, dot):
    A = fdlap.fd_laplacian_2d(-1.0, 1.0, 17).tocsr()
    B = mo.mixed_columns(17)
    for dinv in (None, np.reciprocal(A.diagonal())):
        got = _assert_column_is_single(monkeypatch, A, B, dinv, dot, maxiter=200, tau=TAU)
        assert [g["status"] for g in got] == ["converged"] * 4
        assert [g["exit"] for g in got] == ["tolerance", "none", "tolerance", "none"]   # (1e-200 b).(1e-200 b) = 0
        assert got[1]["iters"] == 1 and len(got[1]["hist"]) == 0
        assert got[2]["iters"] == 1 and len(got[2]["hist"]) == 1                        # the eigenvector
        assert got[0]["iters"] > 10


def test_mixed_and_breakdown_counts_are_comparable():
    """the three dot orders agree on every column's status and iters, and nothing sits on a threshold"""
    A = fdlap.fd_laplacian_2d(-1.0, 1.0, 17).tocsr()
    for dinv in (None, np.reciprocal(A.diagonal())):
        runs = [mo.pcg_multi(A, mo.mixed_columns(17), dinv=dinv, maxiter=200, tau=TAU, dot=d) for d in mo.DOTS]
        for j in range(4):
            assert mo.counts_comparable([r[j] for r in runs], TAU), j
            assert mo.spread([r[j] for r in runs]) <= 1e-11
    D = mo.indefinite_diagonal()
    runs = [mo.pcg_multi(D, mo.breakdown_columns(), dinv=np.reciprocal(D.diagonal()), maxiter=50, tau=TAU, dot=d)
            for d in mo.DOTS]
    for r in runs:
        assert [c["status"] for c in r] == ["converged", "breakdown", "converged"]
        assert r[0]["iters"] == 1 and r[0]["hist"][0] == 0.0          # A M^-1 b = b exactly: alpha = 1, r = 0
        assert r[1]["iters"] == 0 and r[1]["msg"] == "breakdown dot(u,r)==0" and len(r[1]["hist"]) == 0
        assert r[2]["exit"] == "none"
    for j in range(3):
        assert mo.counts_comparable([r[j] for r in runs], TAU)


def test_a_frozen_column_does_not_depend_on_the_others():
    A = mo.matrix("rand257")
    B = mo.columns("rand257")
    a = mo.pcg_multi(A, B, maxiter=100, tau=TAU)
    B2 = B.copy()
    B2[:, 1] = 0.0
    B2[:, 2] *= 7.0
    b = mo.pcg_multi(A, B2, maxiter=100, tau=TAU)
    c = mo.pcg_multi(A, np.ascontiguousarray(B[:, ::-1]), maxiter=100, tau=TAU)
    for other in (b[0], c[3]):
        assert other["iters"] == a[0]["iters"] and _same_bits(other["hist"], a[0]["hist"])
        assert _same_bits(other["soln"], a[0]["soln"])


def test_arrow_matrices_have_the_long_row():
    for n in (1100, 1500):
        A = mo.arrow(n)
        assert (A != A.T).nnz == 0
        lens = np.diff(A.indptr)
        assert lens[5] == n and A.indptr[mo.TILE] > 1280            # the hub's tile needs more than one staging chunk
        d = A.diagonal()
        assert np.all(d > np.asarray(abs(A).sum(axis=1)).ravel() - d)
    assert np.diff(mo.arrow(1500).indptr)[5] > 1280                 # and here the hub row alone does


# ---- the lab layout probe, solver id 6 ------------------------------------------------------------------------------
PCG_MULTI = 6
MULTI_STATE = 32 + 4 * 96      # sizeof(PcgMultiState): 2 int32, an int64, a pointer, an int64; per column 4 int32, 2 int64,
                               # 8 doubles
SUMS = 20 * 8                  # p.Ap [4], [r.r, u.r] [8], the init's [b.b, u.r] [8]


def up(v, a=256):
    return (v + a - 1) // a * a


def _layout(n, maxiter, nrhs):
    from pysolvers_amd import _native as N
    off = (N.I64 * 64)()
    cnt = N.I32(64)
    nbytes = (N.I64 * 2)()
    rc = N.load_lab().psk_lab_solver_layout(PCG_MULTI, n, n, maxiter, 0, 0, nrhs, off, ctypes.byref(cnt), nbytes)
    return rc, [off[i] for i in range(cnt.value)], [nbytes[0], nbytes[1]]


@pytest.mark.parametrize("nrhs", (1, 2, 3, 4))
def test_pcg_multi_layout(nrhs):
    kp = 2 if nrhs <= 2 else 4
    for n, maxiter in itertools.product((0, 1, 255, 256, 257), (0, 1, 100)):
        rc, offs, size = _layout(n, maxiter, nrhs)
        assert rc == 0
        # the large workspace: the B / X staging (n x nrhs), then x, r, p, Ap (n x KP each)
        io, vec = up(n * nrhs * 8), up(n * kp * 8)
        want = [0] + [io + i * vec for i in range(4)]
        ext = [n * nrhs * 8] + [n * kp * 8] * 4
        assert offs[:5] == want, (n, maxiter, offs, want)
        assert size[0] == (io + 4 * vec if n > 0 else 256)
        _check(offs[:5], ext, size[0])
        # the small one: the state, the sums, the history (KP x max(maxiter, 1)), alphas, udr and p.Ap (KP x (maxiter + 1))
        it = kp * (maxiter + 1) * 8
        ext = [MULTI_STATE, SUMS, kp * max(maxiter, 1) * 8, it, it, it]
        want, s = [], 0
        for e in ext:
            want.append(s)
            s += up(e)
        assert offs[5:] == want, (n, maxiter, offs[5:], want)
        assert size[1] == s
        _check(offs[5:], ext, size[1])


def _check(offs, extents, size):
    assert len(offs) == len(extents)
    for i, o in enumerate(offs):
        assert o % 256 == 0, (i, o)
    for i in range(len(offs) - 1):
        assert offs[i + 1] >= offs[i] + extents[i], (i, offs)
        assert extents[i] == 0 or offs[i + 1] > offs[i]
    assert offs[-1] + extents[-1] <= size, (offs, extents, size)


def test_pcg_multi_layout_rejects_a_bad_width():
    assert _layout(10, 10, 5)[0] != 0
    assert _layout(10, 10, 0)[0] != 0
