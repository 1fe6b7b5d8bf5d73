"""Multicolour Gauss-Seidel without a GPU: the oracle colouring (tests/mcgs_oracle.py) is proper and gives the colour
counts the ordering promises, psk_color_plan (host code, called through ctypes) reproduces it exactly, the symmetric
operator is symmetric, and as a PCG preconditioner it beats Jacobi; the Python classes import and the header declares
the entry points.

Bars (written here, not inferred):
* symmetry: |u^T M^-1 v - v^T M^-1 u| <= 5e-16 * ||u|| ||v|| ||M^-1||_est with ||M^-1||_est = the larger of
  ||M^-1 u|| / ||u|| and ||M^-1 v|| / ||v|| (a lower bound of the norm, so the stricter choice), over five pairs of
  standard normal u, v (seed 2). In exact arithmetic the difference is zero; each side is a sum of n rounded products
  of an apply that is itself a few roundings per entry. The prototype of this arithmetic measured at most 4.3e-17 on
  -FD 16^2, -FD 33^2, DH-8 and DH-10 with 1 and 2 sweeps; the bar is ten times that, far inside the 1e-12 the operator
  must meet and far below anything a missing backward pass would give (the forward sweep alone measures 1e-2).
* PCG with the oracle operator takes fewer iterations than with Jacobi (oracle.krylov.pcg, tau 1e-8,
  b = A rand(seed 12345)). Recorded counts, Jacobi / 1 symmetric sweep / 2 symmetric sweeps:
  -FD 64^2 177 / 89 / 63, DH-10 103 / 52 / 36 (and -FD 33^2 96 / 49 / 34, DH-8 51 / 25 / 19).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import mcgs_oracle as mo
from conftest import REPO
from mcgs_cases import matrix
from oracle import krylov

COUNTS = {"negfd16": 2, "negfd33": 2, "dh8": 3, "dh10": 3, "diag": 1}
PLAN_CASES = ["negfd16", "negfd33", "dh8", "dh10", "diag", "one", "nonsym", "shuffled", "longrow", "dense70"]


@pytest.mark.parametrize("name", PLAN_CASES)
def test_oracle_coloring_is_proper(name):
    A = matrix(name)
    color, nc = mo.coloring(A)
    coo = A.tocoo()                       # every stored entry, zeros included
    off = coo.row != coo.col
    assert not np.any(color[coo.row[off]] == color[coo.col[off]])
    assert color.min() == 0 and nc == color.max() + 1 and set(color) == set(range(nc))


@pytest.mark.parametrize("name,want", sorted(COUNTS.items()))
def test_color_counts(name, want):
    assert mo.coloring(matrix(name))[1] == want


def test_red_black_on_the_stencil():
    m = 33
    color, nc = mo.coloring(matrix("negfd33"))
    i = np.arange(m * m)
    assert nc == 2 and np.array_equal(color, ((i // m + i % m) & 1).astype(np.int32))


def test_a_stored_zero_counts_as_structure():
    A, B = matrix("negfd16"), matrix("shuffled")
    ca, cb = mo.coloring(A)[0], mo.coloring(B)[0]
    assert ca[0] == ca[34] and cb[0] != cb[34]      # the stored zero at (0, 34) separates the two rows


def _plan(A):
    from pysolvers_amd import _native as N
    A = A.tocsr()
    n = A.shape[0]
    ip, ix = A.indptr.astype(np.int32), np.ascontiguousarray(A.indices, dtype=np.int32)
    color, nc = np.full(n, -7, dtype=np.int32), N.I32(-1)
    rc = N.lib.psk_color_plan(n, N.ptr(ip), N.ptr(ix), N.ptr(color), ctypes.byref(nc))
    return rc, color, nc.value


@pytest.mark.parametrize("name", PLAN_CASES)
def test_color_plan_equals_the_oracle(name):
    from pysolvers_amd import _native as N
    A = matrix(name)
    rc, color, nc = _plan(A)
    want, wnc = mo.coloring(A)
    assert rc == N.PSK_OK and nc == wnc
    assert np.array_equal(color, want)


def test_color_plan_refuses_bad_input():
    from pysolvers_amd import _native as N
    ip = np.array([0, 1, 2], dtype=np.int32)
    color, nc = np.zeros(2, dtype=np.int32), N.I32()
    for ix in ([0, 2], [-1, 1]):                      # a column outside [0, n)
        bad = np.array(ix, dtype=np.int32)
        assert N.lib.psk_color_plan(2, N.ptr(ip), N.ptr(bad), N.ptr(color), ctypes.byref(nc)) == N.PSK_ERR_ARG
    ok = np.array([0, 1], dtype=np.int32)
    assert N.lib.psk_color_plan(0, N.ptr(ip), N.ptr(ok), N.ptr(color), ctypes.byref(nc)) == N.PSK_ERR_ARG
    assert N.lib.psk_color_plan(-3, N.ptr(ip), N.ptr(ok), N.ptr(color), ctypes.byref(nc)) == N.PSK_ERR_ARG


@pytest.mark.parametrize("name", ["negfd16", "dh8", "nonsym", "shuffled", "diag", "one"])
def test_vectorised_oracle_is_the_scalar_definition(name):
    A = matrix(name)
    v = np.random.default_rng(1).standard_normal(A.shape[0])
    v[0] = -0.0
    for sweeps in (1, 2):
        for symmetric in (True, False):
            a = mo.apply_scalar(A, v, sweeps, symmetric)
            b = mo.MCGS(A, sweeps, symmetric)(v)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_one_forward_sweep_is_gauss_seidel_in_the_colour_order():
    """z = (D + L_c)^-1 v with L_c the entries whose column's colour comes first: the classical sweep, here by a dense
    solve in the permuted order (another summation order: a few ulp of cond * ||z||)."""
    A = matrix("dh8")
    color, _ = mo.coloring(A)
    p = np.argsort(color, kind="stable")
    Ap = A.toarray()[np.ix_(p, p)]
    v = np.random.default_rng(4).standard_normal(A.shape[0])
    z = np.linalg.solve(np.tril(Ap), v[p])
    got = mo.MCGS(A, 1, False)(v)[p]
    assert np.linalg.norm(got - z) <= 1e-12 * np.linalg.norm(z)


@pytest.mark.parametrize("name", ["negfd16", "negfd33", "dh8", "dh10"])
@pytest.mark.parametrize("sweeps", [1, 2])
def test_symmetric_operator_is_symmetric(name, sweeps):
    A = matrix(name)
    op = mo.MCGS(A, sweeps, True)
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(5):
        u, v = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
        Mu, Mv = op(u), op(v)
        est = max(np.linalg.norm(Mu) / np.linalg.norm(u), np.linalg.norm(Mv) / np.linalg.norm(v))
        worst = max(worst, abs(np.dot(u, Mv) - np.dot(v, Mu)) / (np.linalg.norm(u) * np.linalg.norm(v) * est))
        assert np.dot(u, Mu) > 0.0 and np.dot(v, Mv) > 0.0      # and positive definite
    print("%s sweeps %d: symmetry defect %.3e" % (name, sweeps, worst))
    assert worst <= 5e-16


@pytest.mark.parametrize("name,want", [("negfd64", (177, 89, 63)), ("dh10", (103, 52, 36))])
def test_oracle_pcg_takes_fewer_iterations_than_jacobi(name, want):
    A = matrix(name)
    b = A @ np.random.default_rng(12345).random(A.shape[0])
    jac = krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=krylov.jacobi_form(A))
    one = krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=mo.MCGS(A, 1, True))
    two = krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=mo.MCGS(A, 2, True))
    print("%s: PCG iterations Jacobi %d, SGS 1 sweep %d, 2 sweeps %d" % (name, jac["iters"], one["iters"], two["iters"]))
    assert jac["success"] and one["success"] and two["success"]
    assert two["iters"] < one["iters"] < jac["iters"]
    assert (jac["iters"], one["iters"], two["iters"]) == want
    assert np.linalg.norm(b - A @ one["soln"]) <= 1e-7 * np.linalg.norm(b)


def test_oracle_refuses_what_the_library_refuses():
    import scipy.sparse as sp
    with pytest.raises(OverflowError):
        mo.MCGS(matrix("dense70"))
    with pytest.raises(ValueError) as e:                # a zero diagonal: the smallest such row is named
        mo.MCGS(sp.csr_matrix(np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])))
    assert "row 1" in str(e.value)
    with pytest.raises(ValueError):
        mo.MCGS(matrix("negfd16"), sweeps=0)


def test_classes_are_importable():
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import (MulticolorGS, MulticolorGSPreconditioner, MulticolorGSPreconditionerType,
                                      MulticolorGaussSeidelSmoother)
    from pysolvers_amd.Linear.Preconditioner import DeviceOperator, GenericPreconditioner
    from pysolvers_amd.Linear.PreconditionerType import PreconditionerType
    assert psk.MulticolorGS is MulticolorGS is MulticolorGSPreconditionerType
    assert psk.MulticolorGSPreconditioner is MulticolorGSPreconditioner
    assert psk.MulticolorGaussSeidelSmoother is MulticolorGaussSeidelSmoother
    t = MulticolorGS()
    assert isinstance(t, PreconditionerType) and t.sweeps == 1 and t.symmetric is True
    assert MulticolorGS(sweeps=2, symmetric=False).sweeps == 2 and not MulticolorGS(2, False).symmetric
    assert issubclass(MulticolorGSPreconditioner, DeviceOperator)
    assert issubclass(MulticolorGSPreconditioner, GenericPreconditioner)
    assert MulticolorGSPreconditioner.device_kind == N.PSK_PREC_MCGS == 7
    assert N.PSK_MCGS_MAX_COLORS == mo.MAX_COLORS == 64 and N.PSK_MCGS_SYMMETRIC == 1
    assert N.lib.psk_abi_version() == 4
    assert hasattr(psk.DeviceCSR, "coloring")
    assert {"psk_color_plan", "psk_prec_create_mcgs", "psk_prec_mcgs_info"} <= set(N.SIGNATURES)
    S = MulticolorGaussSeidelSmoother.of(sweeps=2, symmetric=False)
    assert issubclass(S, MulticolorGaussSeidelSmoother) and S.sweeps == 2 and S.symmetric is False
    assert MulticolorGaussSeidelSmoother.sweeps == 1 and MulticolorGaussSeidelSmoother.symmetric is True


def test_header_declares_the_entry_points():
    raw = open(os.path.join(REPO, "include", "psk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+psk_color_plan\s*\(\s*int64_t\s+n\s*,\s*const\s+int32_t\s*\*\s*rowptr\s*,\s*const\s+int32_t"
                     r"\s*\*\s*colidx\s*,\s*int32_t\s*\*\s*color\s*,\s*int32_t\s*\*\s*ncolors\s*\)\s*;", txt)
    assert re.search(r"\bint\s+psk_prec_create_mcgs\s*\(\s*const\s+psk_csr\s*\*\s*A\s*,\s*int32_t\s+sweeps\s*,\s*int32_t"
                     r"\s+flags\s*,\s*psk_prec\s*\*\*\s*out\s*\)\s*;", txt)
    assert re.search(r"\bint\s+psk_prec_mcgs_info\s*\(\s*const\s+psk_prec\s*\*\s*M\s*,\s*int32_t\s*\*\s*ncolors\s*,"
                     r"\s*int32_t\s*\*\s*sweeps\s*,\s*int32_t\s*\*\s*flags\s*,\s*int64_t\s*\*\s*color_rows\s*\)\s*;", txt)
    for name, value in (("PSK_PREC_MCGS", 7), ("PSK_MCGS_MAX_COLORS", 64), ("PSK_MCGS_SYMMETRIC", 1),
                        ("PSK_ABI_VERSION", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), txt), name
