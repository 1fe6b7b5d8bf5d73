"""MINRES without a GPU: the CPU oracle (tests/minres_oracle.py) pinned to scipy's own iterates, the dot-order spread
rule the GPU tests rely on, the hand-checked exits, the workspace layout and the boundary (header, binding, class).

Bars (written here, not inferred):
* Pinned to scipy: the oracle's x_k equal the iterates scipy.sparse.linalg.minres(..., rtol=1e-300, maxiter=60,
  callback=...) hands its callback, for every k it reports, to a relative 1e-12 in the 2-norm. Measured with scipy
  1.15.3: at most 1.3e-15 on the six cases. A wrong recurrence is off by O(1); the three decades are room for
  another BLAS (scipy's inner products and its norm([gbar, beta]) go through it).
* Identity: hist[k] is within 1e-12 ||b|| of ||b - A x_k||_2 (measured at most 4.8e-16).
* The cases are indefinite: eigenvalues of both signs (37, 64 and 110 negative ones at m = 17, 23, 33; min |lambda|
  >= 2e-2).
* Prefix >= 10 (measured 53-142; past it the three orders part by about 1e-3 and their counts by up to 2 of 133-460).
* The hand-checked exits are exact (small integers).
"""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import minres_oracle as mo
from conftest import REPO
from oracle import krylov

TAU = 1e-10
K = 60
# (m, scaled, jacobi)
SIX = [(17, False, False), (17, True, False), (17, True, True), (23, True, True), (33, True, True), (33, False, False)]


@functools.lru_cache(maxsize=None)
def _case(m, scaled):
    A, b = mo.shifted_fd(m, scaled)
    b.setflags(write=False)
    return A, b


def _prec(A, jacobi):
    return krylov.jacobi_form(A) if jacobi else mo.identity


@functools.lru_cache(maxsize=None)
def _iterates(m, scaled, jacobi):
    """(the oracle's result with tau = 0 and maxiter = K, its iterates x_0..x_{K-1})"""
    A, b = _case(m, scaled)
    xs = []
    res = mo.minres(A, b, M=_prec(A, jacobi), maxiter=K, tau=0.0, on_iter=lambda k, x: xs.append(x.copy()))
    return res, xs


@pytest.mark.parametrize("m,scaled,jacobi", SIX)
def test_oracle_is_pinned_to_scipys_iterates(m, scaled, jacobi):
    A, b = _case(m, scaled)
    M = spla.LinearOperator(A.shape, matvec=_prec(A, jacobi), dtype=np.float64) if jacobi else None
    ref = []
    spla.minres(A, np.array(b), rtol=1e-300, maxiter=K, M=M, callback=lambda x: ref.append(np.array(x)))
    _, xs = _iterates(m, scaled, jacobi)
    assert len(xs) == K and 10 <= len(ref) <= K          # scipy may stop on a rule of its own; never this early
    err = max(np.linalg.norm(xs[k] - ref[k]) / np.linalg.norm(ref[k]) for k in range(len(ref)))
    print("m = %d scaled = %s jacobi = %s: %d scipy iterates, max relative deviation %.3e" % (m, scaled, jacobi,
                                                                                             len(ref), err))
    assert err <= 1e-12, err


@pytest.mark.parametrize("m,scaled", [(17, False), (17, True), (33, False)])
def test_identity_history_is_the_true_residual(m, scaled):
    A, b = _case(m, scaled)
    res, xs = _iterates(m, scaled, False)
    nb = np.linalg.norm(b)
    dev = max(abs(res["hist"][k] - np.linalg.norm(b - A @ xs[k])) for k in range(K)) / nb
    print("m = %d scaled = %s: max |hist - ||b - A x_k||| = %.3e ||b||" % (m, scaled, dev))
    assert dev <= 1e-12, dev


@pytest.mark.parametrize("m,want_neg", [(17, 37), (23, 64), (33, 110)])
def test_cases_are_indefinite(m, want_neg):
    for scaled in (False, True):
        A, _ = _case(m, scaled)
        assert abs(A - A.T).max() == 0.0
        ev = np.linalg.eigvalsh(A.toarray())
        assert (ev < 0).sum() == want_neg and (ev > 0).sum() == m * m - want_neg     # inertia survives S A S
        assert np.abs(ev).min() >= 2e-2, (m, scaled, np.abs(ev).min())
        d = A.diagonal()
        assert np.all(d > 0)                                                          # Jacobi is SPD
        assert (d.max() > 2 * d.min()) == scaled                                      # and not a multiple of I


@functools.lru_cache(maxsize=None)
def _spread(m, scaled, jacobi):
    A, b = _case(m, scaled)
    return mo.spread(A, b, M=_prec(A, jacobi), tau=TAU, maxiter=1000)


@pytest.mark.parametrize("m,scaled,jacobi", SIX)
def test_every_dot_order_solves_and_the_prefix_rule_holds(m, scaled, jacobi):
    A, b = _case(m, scaled)
    res, prefix = _spread(m, scaled, jacobi)
    print("m = %d scaled = %s jacobi = %s: prefix %d, iterations %s" % (m, scaled, jacobi, prefix,
                                                                        [r["iters"] for r in res]))
    assert all(r["success"] and r["exit"] == "tolerance" for r in res)
    assert prefix >= 10, prefix
    nb = np.linalg.norm(b)
    for r in res:
        tr = np.linalg.norm(b - A @ r["soln"])
        assert r["resid"] == tr
        if jacobi:      # the test was made in the M^-1 norm: ||r||_2 <= sqrt(cond(M)) tau ||b||
            d = A.diagonal()
            assert tr <= np.sqrt(d.max() / d.min()) * TAU * nb
        else:
            assert tr <= TAU * nb


def test_rand_sym_indef_has_the_stated_shape():
    A, b = mo.rand_sym_indef(1100, 7)
    A = A.copy()       # scipy's arithmetic sorts its operand's rows in place
    assert any(np.any(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) < 0) for i in range(40))   # rows unsorted
    assert abs(A - A.T).max() == 0.0
    d = A.diagonal()
    off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
    assert np.all(np.abs(d) > off + 0.999)                       # strictly diagonally dominant, margin 1 (rounded)
    assert np.all(d[0::2] > 0) and np.all(d[1::2] < 0)           # hence indefinite (Gershgorin: 550 of each sign)
    assert 5.0 <= (A.nnz - 1100) / 1100 <= 6.0
    st = mo.minres(A, b, maxiter=1000, tau=TAU)
    assert st["success"] and np.linalg.norm(b - A @ st["soln"]) <= TAU * np.linalg.norm(b)


# ---- exits, hand-checked ---------------------------------------------------------------------------------------------

def test_one_by_one():
    """A = [-2.5], b = [2]: beta1 = 2, v = 1, y = -2.5, alfa = -2.5, r2 = -2.5 + 1.25 * 2 = 0, beta = 0, gbar = -2.5,
    gamma = 2.5, cs = -1, sn = 0, phi = -2, w = 0.4, x = -0.8, phibar = 0."""
    st = mo.minres(sp.csr_matrix(np.array([[-2.5]])), np.array([2.0]), tau=TAU)
    assert st["success"] and st["iters"] == 1 and np.array_equal(st["hist"], [0.0]) and st["exit"] == "tolerance"
    assert st["soln"][0] == -0.8


def test_two_by_two_swap():
    """[[0, 1], [1, 0]], b = (1, 0): k = 0: v = e1, y = e2, alfa = 0, r2 = e2, beta = 1, gbar = 0, gamma = 1, cs = 0,
    sn = 1, phi = 0, phibar = 1 (x stays 0: MINRES cannot reduce the residual in one step). k = 1: v = e2, y = e1 -
    e1 = 0, alfa = 0, beta = 0, delta = 0, gbar = dbar = 1, gamma = 1, cs = 1, phi = 1, w = e2, x = e2, phibar = 0."""
    st = mo.minres(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), np.array([1.0, 0.0]), tau=TAU)
    assert st["success"] and st["iters"] == 2
    assert np.array_equal(st["hist"], [1.0, 0.0]) and np.array_equal(st["soln"], [0.0, 1.0])


def test_indefinite_preconditioner_is_refused_at_the_init():
    """diag(1, -1), b = (1, 2), M^-1 = diag(1, -1): b.z = 1 - 4 = -3."""
    minv = np.array([1.0, -1.0])
    st = mo.minres(sp.diags([1.0, -1.0]).tocsr(), np.array([1.0, 2.0]), M=lambda v: minv * v, tau=TAU)
    assert st["status"] == "breakdown" and not st["success"] and st["iters"] == 0 and len(st["hist"]) == 0
    assert st["msg"] == "preconditioner not positive definite" and np.isnan(st["resid"])


PATH3 = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])


def test_indefinite_preconditioner_is_refused_at_iteration_one():
    """The path graph on three nodes, b = e1, M^-1 = diag(1, 1, -1): b.z = 1 and iteration 0 (r2 = e2, beta = 1,
    hist[0] = 1) sees only the positive part; iteration 1 has v = e2, y = (e1 + e3) - e1 = e3, alfa = 0, r2 = e3,
    z = -e3, r2.z = -1."""
    minv = np.array([1.0, 1.0, -1.0])
    st = mo.minres(sp.csr_matrix(PATH3), np.array([1.0, 0.0, 0.0]), M=lambda v: minv * v, tau=TAU)
    assert st["status"] == "breakdown" and st["iters"] == 1 and np.array_equal(st["hist"], [1.0])
    assert st["msg"] == "preconditioner not positive definite"


def test_gamma_zero_breakdown():
    """diag(0, 1), b = e1 (b in the null space of a singular A): y = 0, alfa = 0, r2 = 0, beta = 0, gbar = 0."""
    st = mo.minres(sp.csr_matrix(np.array([[0.0, 0.0], [0.0, 1.0]])), np.array([1.0, 0.0]), tau=TAU)
    assert st["status"] == "breakdown" and st["iters"] == 0 and len(st["hist"]) == 0
    assert st["msg"] == "breakdown gamma==0" and np.isnan(st["resid"])


def test_zero_rhs_and_maxiter_rules():
    A, b = _case(17, True)
    z = mo.minres(A, np.zeros(289))
    assert z["success"] and z["iters"] == 1 and z["exit"] == "none" and len(z["hist"]) == 0
    assert np.array_equal(z["soln"], np.zeros(289))
    M = krylov.jacobi_form(A)
    st = mo.minres(A, b, M=M, maxiter=5, tau=TAU, fail_on_maxiter=True)
    assert st["status"] == "maxiter" and not st["success"] and st["iters"] == 4 and len(st["hist"]) == 5
    assert st["msg"] == "failure to converge"
    ok = mo.minres(A, b, M=M, maxiter=5, tau=TAU, fail_on_maxiter=False)
    assert ok["status"] == "converged" and ok["success"] and ok["iters"] == 5 and ok["exit"] == "maxiter"
    assert np.array_equal(ok["hist"], st["hist"]) and np.array_equal(ok["soln"], st["soln"])
    assert np.all(np.diff(st["hist"]) <= 0)                        # MINRES's residual never grows


# ---- the workspace layout (solve_loop.hpp Carve through psk_lab_solver_layout; no GPU) -------------------------------

MINRES_ID = 5           # PSK_LAB_SOLVER_MINRES (4 stays tests/test_solver_layout.py's unknown solver)
GEN = 1
MINRES_STATE = 184      # sizeof(MinresState): 6 int32, 3 int64, 15 doubles, a pointer, an int64


def _up(v, a=256):
    return (v + a - 1) // a * a


@pytest.mark.parametrize("gen", (0, 1))
def test_minres_layout(gen):
    from pysolvers_amd import _native as N
    lab = N.load_lab()
    for n, maxiter in itertools.product((0, 1, 511, 512, 513), (0, 1, 100)):
        off = (N.I64 * 64)()
        cnt = N.I32(64)
        nbytes = (N.I64 * 2)()
        N.check(lab.psk_lab_solver_layout(MINRES_ID, n, n, maxiter, 0, gen * GEN, 1, off, ctypes.byref(cnt), nbytes),
                "psk_lab_solver_layout")
        offs = [off[i] for i in range(cnt.value)]
        # the large workspace: b, x, y, t, the rings of two r, two w and two v, then z for a general preconditioner
        vec, nbig = _up(n * 8), 11 if gen else 10
        assert len(offs) == nbig + 3
        assert offs[:nbig] == [i * vec for i in range(nbig)], (n, maxiter, offs)
        assert nbytes[0] == (nbig * vec if n > 0 else 256)
        # the small one: the state, the 8 sums, the history (one entry more than maxiter)
        assert offs[nbig:] == [0, 256, 512], (n, maxiter, offs[nbig:])
        assert nbytes[1] == 512 + _up((maxiter + 1) * 8)
        for part, ext, size in ((offs[:nbig], [n * 8] * nbig, nbytes[0]),
                                (offs[nbig:], [MINRES_STATE, 64, (maxiter + 1) * 8], nbytes[1])):
            assert all(o % 256 == 0 for o in part)
            for i in range(len(part) - 1):
                assert part[i + 1] >= part[i] + ext[i] and (ext[i] == 0 or part[i + 1] > part[i])
            assert part[-1] + ext[-1] <= size


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_entry_point_declared_and_bound():
    from pysolvers_amd import _native as N
    with open(os.path.join(REPO, "include", "psk.h")) as f:
        text = f.read()
    decl = re.search(r"\bint\s+psk_minres\s*\(([^;]*)\)\s*;", text)
    assert decl is not None
    bi = re.search(r"\bint\s+psk_bicgstab\s*\(([^;]*)\)\s*;", text)
    assert " ".join(decl.group(1).split()) == " ".join(bi.group(1).split())       # psk_bicgstab's signature
    assert N.SIGNATURES["psk_minres"] == N.SIGNATURES["psk_bicgstab"]
    assert hasattr(N.lib, "psk_minres")
    assert N.lib.psk_abi_version() == 4                                           # one entry point, no struct touched
    assert "sqrt(cond(M))" in text and "M^-1 norm" in text                        # the norm convergence is judged in


def test_factory_constructs():
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import MINRES, MINRESSolver, GMRESSolver
    ctl = psk.CommonSolverArgs(maxiter=77, tau=1e-9, showIters=False, showFinal=False)
    s = MINRES(control=ctl, precond=psk.JacobiPreconditionerType(), name="mr").makeSolver()
    assert isinstance(s, MINRESSolver) and isinstance(s, psk.IterativeLinearSolver)
    assert s._entry == "psk_minres" and s.name() == "mr" and s.maxiter() == 77 and s.tau() == 1e-9
    assert isinstance(s.precondType(), psk.JacobiPreconditionerType)
    assert MINRES().makeSolver().name() == "MINRES" and psk.MINRES is MINRES and psk.MINRESSolver is MINRESSolver
    assert MINRESSolver._method == "MINRES" and GMRESSolver._method == "GMRES"
    # a caller's norm re-tests the true residual under the identity only; GMRES always
    assert s._retests_true_residual(N.PSK_PREC_IDENTITY) and not s._retests_true_residual(N.PSK_PREC_JACOBI)
    assert GMRESSolver(ctl)._retests_true_residual(N.PSK_PREC_JACOBI)
