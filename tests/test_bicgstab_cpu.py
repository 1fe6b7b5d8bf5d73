"""BiCGStab without a GPU: the CPU oracle (tests/bicgstab_oracle.py) against a dense solve and on hand-checked
cases, the dot-order spread rule the GPU tests rely on, and the boundary (header, binding, Python class).

Bars: the oracle's x has a true residual <= tau ||b|| (the solver's own stopping rule; no other bar). The
hand-checked cases are exact (small integers, powers of two).
"""
import os
import re

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import bicgstab_oracle as bo
from conftest import GOLDEN, REPO
from oracle import krylov

TAU = 1e-10


def _dh8():
    return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr()


@pytest.mark.parametrize("name", ["cd17", "dh8"])
def test_oracle_solves_the_system(name):
    A = bo.cd_matrix(17, 0.3) if name == "cd17" else _dh8()
    b = np.random.default_rng(len(name) + 17).standard_normal(A.shape[0])
    st = bo.bicgstab(A, b, M=krylov.jacobi_form(A), maxiter=1000, tau=TAU)
    assert st["success"] and st["exit"] == "tolerance" and len(st["hist"]) == st["iters"]
    x = st["soln"]
    assert np.linalg.norm(b - A @ x) <= TAU * np.linalg.norm(b)
    xd = np.linalg.solve(A.toarray(), b)                       # the dense solution meets the same bar,
    assert np.linalg.norm(b - A @ xd) <= TAU * np.linalg.norm(b)   # so both solve the same system to tau
    assert st["resid"] == np.linalg.norm(b - A @ x)


def test_every_dot_order_solves_and_the_prefix_rule_holds():
    """The three summation orders all converge; the table cases agree on >= 10 iterations (the GPU tests assert
    parity on that prefix only); cd17 is the case whose iteration counts are comparable."""
    for name, A in (("cd17", bo.cd_matrix(17, 0.3)), ("cd33", bo.cd_matrix(33, 0.5)), ("dh8", _dh8())):
        b = np.random.default_rng(len(name) + 17).standard_normal(A.shape[0])
        res, prefix = bo.spread(A, b, M=krylov.jacobi_form(A), tau=TAU)
        assert all(r["success"] for r in res), name
        assert prefix >= 10, (name, prefix)
        if name == "cd17":
            assert bo.counts_comparable(res, TAU) and prefix == len(res[0]["hist"])


def test_breakdown_at_iteration_zero():
    """A = [[0, 1], [-1, 0]], b = (1, 0): v = A b = (0, -1), rhat.v = 0."""
    A = sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))
    st = bo.bicgstab(A, np.array([1.0, 0.0]))
    assert st["status"] == "breakdown" and not st["success"] and st["iters"] == 0
    assert st["msg"] == "breakdown dot(rhat,v)==0" and len(st["hist"]) == 0


def test_diagonal_matrix_takes_the_half_step_exit():
    """A = diag(d), Jacobi: A M^-1 b = d (1/d) b. With d powers of two both products are exact, so v = b,
    alpha = 1, s = 0 exactly: the half step ends the solve with hist = [0.0] and x = (1/d) b bitwise. (A
    general d rounds (1/d) and the two products, and s is then only tiny.)"""
    rng = np.random.default_rng(3)
    n = 700
    d = 2.0 ** rng.integers(-3, 4, size=n)
    b = rng.standard_normal(n)
    A = sp.diags(d).tocsr()
    st = bo.bicgstab(A, b, M=krylov.jacobi_form(A), tau=TAU)
    assert st["success"] and st["iters"] == 1 and st["exit"] == "tolerance"
    assert np.array_equal(st["hist"], np.array([0.0]))
    assert np.array_equal(st["soln"].view(np.uint64), ((1.0 / d) * b).view(np.uint64))


def test_one_by_one():
    """A = [[-2.5]], b = [2]: v = -5, alpha = 4 / -10 = -0.4, s = 2 - (-0.4)(-5) = 0, x = -0.4 * 2 = -0.8."""
    st = bo.bicgstab(sp.csr_matrix(np.array([[-2.5]])), np.array([2.0]), tau=TAU)
    assert st["success"] and st["iters"] == 1 and np.array_equal(st["hist"], [0.0])
    assert st["soln"][0] == -0.8


def test_zero_rhs():
    A = bo.cd_matrix(5, 0.3)
    st = bo.bicgstab(A, np.zeros(25))
    assert st["success"] and st["iters"] == 1 and st["exit"] == "none" and len(st["hist"]) == 0
    assert np.array_equal(st["soln"], np.zeros(25))


def test_maxiter_rules():
    A = bo.cd_matrix(17, 0.3)
    b = np.random.default_rng(21).standard_normal(A.shape[0])
    M = krylov.jacobi_form(A)
    st = bo.bicgstab(A, b, M=M, maxiter=5, tau=TAU, fail_on_maxiter=True)
    assert st["status"] == "maxiter" and not st["success"] and st["iters"] == 4 and len(st["hist"]) == 5
    assert st["msg"] == "failure to converge"
    ok = bo.bicgstab(A, b, M=M, maxiter=5, tau=TAU, fail_on_maxiter=False)
    assert ok["status"] == "converged" and ok["success"] and ok["iters"] == 5 and ok["exit"] == "maxiter"
    assert np.array_equal(ok["hist"], st["hist"]) and np.array_equal(ok["soln"], st["soln"])
    z = bo.bicgstab(A, b, M=M, maxiter=30, tau=0.0)
    assert z["status"] == "maxiter" and len(z["hist"]) == 30 and np.all(np.isfinite(z["hist"]))


def test_entry_point_declared_and_bound():
    from pysolvers_amd import _native as N
    with open(os.path.join(REPO, "include", "psk.h")) as f:
        text = f.read()
    decl = re.search(r"\bint\s+psk_bicgstab\s*\(([^;]*)\)\s*;", text)
    assert decl is not None
    gm = re.search(r"\bint\s+psk_gmres\s*\(([^;]*)\)\s*;", text)
    assert " ".join(decl.group(1).split()) == " ".join(gm.group(1).split())       # psk_gmres's signature
    assert N.SIGNATURES["psk_bicgstab"] == N.SIGNATURES["psk_gmres"]
    assert hasattr(N.lib, "psk_bicgstab")


def test_factory_constructs():
    import pysolvers_amd as psk
    from pysolvers_amd.Linear import BiCGStab, BiCGStabSolver, GMRESSolver
    ctl = psk.CommonSolverArgs(maxiter=77, tau=1e-9, showIters=False, showFinal=False)
    s = BiCGStab(control=ctl, precond=psk.JacobiPreconditionerType(), name="bi").makeSolver()
    assert isinstance(s, BiCGStabSolver) and isinstance(s, psk.IterativeLinearSolver)
    assert s._entry == "psk_bicgstab" and s.name() == "bi" and s.maxiter() == 77 and s.tau() == 1e-9
    assert isinstance(s.precondType(), psk.JacobiPreconditionerType)
    assert BiCGStab().makeSolver().name() == "BiCGStab" and psk.BiCGStab is BiCGStab
    # the caller-norm failure text is built from the method's name; GMRES keeps its own
    assert BiCGStabSolver._method == "BiCGStab" and GMRESSolver._method == "GMRES"
