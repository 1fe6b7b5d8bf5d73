"""IDR(s) without a GPU: the shadow-space hash pinned to literal values, the CPU oracle (tests/idrs_oracle.py) on the
BiCGStab tests' systems and on hand-checked cases, and the boundary (header, binding, Python class).

Bars: the oracle's x has a true residual <= tau ||b|| (the solver's own stopping rule; no other bar) wherever the oracle
itself reports success; the step counts are those the recurrence gave when this file was written (they move only if
the recurrence does).
"""
import os
import re

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import bicgstab_oracle as bo
import idrs_oracle as io_
from conftest import GOLDEN, REPO
from oracle import krylov

TAU = 1e-10


def _matrix(name):
    if name == "dh8":
        return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr()
    m = int(name[2:4])
    return bo.cd_matrix(m, {17: 0.3, 33: 0.5}[m])


def _rhs(name, n):
    return np.random.default_rng(len(name) + 17).standard_normal(n)      # tests/test_gpu_bicgstab.py's _rhs


def test_shadow_hash_is_pinned():
    """splitmix64 and shadow(3, 2) against literal values (computed once from the statement in include/psk.h)."""
    assert io_.splitmix64(0) == 0xE220A8397B1DCDAF and io_.splitmix64(1) == 0x910A2DEC89025CC1
    want = [float.fromhex(h) for h in ("0x1.8882a0e5ec772p-1", "0x1.10a2dec890258p-3", "0x1.75835de1c9750p-3",
                                       "-0x1.8bd3ac6c93f9ep-1", "-0x1.18c1c8d1dcc78p-3", "-0x1.cfcc4f35c7640p-3")]
    P = io_.shadow(3, 2)
    assert P.shape == (3, 2) and P.ravel().tolist() == want
    big = io_.shadow(700, 8)
    assert np.all(big >= -1.0) and np.all(big < 1.0) and len(np.unique(big)) == big.size
    assert np.array_equal(big * 2.0 ** 52, np.round(big * 2.0 ** 52))      # multiples of 2^-52: exact in f64


# steps to ||r|| <= 1e-10 ||b|| under Jacobi (np.dot); one step = one SpMV
STEPS = {("cd17", 1): 92, ("cd17", 2): 79, ("cd17", 4): 76, ("cd17", 8): 70,
         ("cd33", 1): 115, ("cd33", 2): 104, ("cd33", 4): 100, ("cd33", 8): 96,
         ("dh8", 1): 86, ("dh8", 2): 71, ("dh8", 4): 66, ("dh8", 8): 60}


@pytest.mark.parametrize("name,s", sorted(STEPS))
def test_oracle_converges_and_its_step_count_is_recorded(name, s):
    A = _matrix(name)
    b = _rhs(name, A.shape[0])
    st = io_.idrs(A, b, s=s, M=krylov.jacobi_form(A), maxiter=1000, tau=TAU)
    nb = np.linalg.norm(b)
    assert st["exit"] == "tolerance" and len(st["hist"]) == st["iters"] == STEPS[name, s]
    assert st["hist"][-1] <= TAU * nb and np.all(st["hist"][:-1] > TAU * nb)
    tr = np.linalg.norm(b - A @ st["soln"])
    assert st["resid"] == tr and st["success"] == (tr <= TAU * nb)
    if (name, s) != ("cd33", 4):         # cd33, s = 4 ends at 0.95 tau ||b|| and its true residual is 1.04: a failure
        assert st["success"]             # the oracle reports as psk_idrs does (PSK_TRUE_RESID_FAIL)


def test_zero_rhs_gives_zero():
    st = io_.idrs(bo.cd_matrix(5, 0.3), np.zeros(25), s=4)
    assert st["success"] and st["iters"] == 1 and st["exit"] == "none" and len(st["hist"]) == 0
    assert np.array_equal(st["soln"], np.zeros(25)) and st["resid"] == 0.0


def test_maxiter_rules():
    A = _matrix("cd17")
    b = _rhs("cd17", A.shape[0])
    M = krylov.jacobi_form(A)
    for mi in (3, 5, 7):                                   # inside a cycle, on the omega step (s + 1 = 5), behind it
        st = io_.idrs(A, b, s=4, M=M, maxiter=mi, tau=TAU, fail_on_maxiter=True)
        assert not st["success"] and st["status"] == "maxiter" and st["iters"] == mi - 1 and len(st["hist"]) == mi
        assert st["msg"] == "failure to converge" and st["resid"] == st["hist"][-1]
        ok = io_.idrs(A, b, s=4, M=M, maxiter=mi, tau=TAU, fail_on_maxiter=False)
        assert ok["success"] and ok["status"] == "converged" and ok["exit"] == "maxiter" and ok["iters"] == mi
        assert np.array_equal(ok["hist"], st["hist"])
    z = io_.idrs(A, b, s=4, M=M, maxiter=30, tau=0.0)
    assert z["status"] == "maxiter" and len(z["hist"]) == 30 and np.all(np.isfinite(z["hist"]))
    assert io_.idrs(A, b, s=4, M=M, maxiter=0)["iters"] == 0


def test_breakdown_on_a_zero_pivot():
    """A b = 0 exactly: g = A u = 0 at step 0, so every q_i and with them Mm[0][0] are zero."""
    A, b = io_.breakdown_system()
    assert not np.any(A @ b)
    for s in (1, 4):
        st = io_.idrs(A, b, s=s, tau=TAU)
        assert not st["success"] and st["status"] == "breakdown" and st["iters"] == 0 and len(st["hist"]) == 0
        assert st["msg"] == "breakdown Mm[k][k]==0" and np.isnan(st["resid"])


def test_bad_s_is_refused():
    for s in (0, 9, -1):
        with pytest.raises(ValueError):
            io_.idrs(bo.cd_matrix(5, 0.3), np.ones(25), s=s)


def test_every_dot_order_converges_and_the_prefix_rule_holds():
    """What tests/test_gpu_idrs.py relies on: the three summation orders agree on >= 10 steps of cd17, s = 4."""
    A = _matrix("cd17")
    res, prefix = io_.spread(A, _rhs("cd17", A.shape[0]), s=4, M=krylov.jacobi_form(A), tau=TAU, maxiter=1000)
    assert all(r["success"] for r in res) and prefix >= 10
    assert io_.counts_comparable is bo.counts_comparable


# ---- the boundary ----------------------------------------------------------------------------------------------------

def test_header_declares_psk_idrs_and_the_binding_holds_it():
    from pysolvers_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "psk.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+psk_idrs\s*\(([^;]*)\)\s*;", text)
    assert decl is not None
    args = " ".join(decl.group(1).split())
    assert args == ("const psk_csr *A, const psk_prec *M, const double *b, double *x, const psk_ctl *ctl, int32_t s, "
                    "psk_result *res, double *hist, int32_t loc")
    assert re.search(r"#define\s+PSK_IDRS_MAX_S\s+8\b", text) and N.PSK_IDRS_MAX_S == io_.MAX_S == 8
    sig = N.SIGNATURES["psk_idrs"]
    bi = N.SIGNATURES["psk_bicgstab"]
    assert sig[0] is bi[0] and sig[1] == bi[1][:5] + [N.I32] + bi[1][5:]      # psk_bicgstab's with s behind ctl
    assert hasattr(N.lib, "psk_idrs") and N.lib.psk_abi_version() == 4


def test_python_class():
    import pysolvers_amd as psk
    from pysolvers_amd.Linear import IDRs, IDRsSolver
    ctl = psk.CommonSolverArgs(maxiter=77, tau=1e-9, showIters=False, showFinal=False)
    s = IDRs(control=ctl, precond=psk.JacobiPreconditionerType(), s=6, name="idr").makeSolver()
    assert isinstance(s, IDRsSolver) and isinstance(s, psk.IterativeLinearSolver)
    assert s._entry == "psk_idrs" and s.name() == "idr" and s.maxiter() == 77 and s.tau() == 1e-9 and s.s() == 6
    assert IDRs().makeSolver().s() == 4 and IDRs().makeSolver().name() == "IDRs"
    assert psk.IDRs is IDRs and psk.IDRsSolver is IDRsSolver and IDRsSolver._method == "IDR(s)"
    for bad in (0, 9, 2.5, True):
        with pytest.raises(ValueError):
            IDRs(s=bad)
        with pytest.raises(ValueError):
            IDRsSolver(s=bad)
