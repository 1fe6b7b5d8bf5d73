"""FSAI without a GPU: the oracle (tests/fsai_oracle.py) is an approximate inverse Cholesky factor on the prescribed
pattern, refuses a matrix that is not definite, and as a PCG preconditioner beats Jacobi; the Python classes import
and the header declares the entry points.

Bars (written here, not inferred):
* max |diag(G sA G^T) - 1| <= 1e-14. In exact arithmetic row i of G sA G^T has a unit diagonal (g = C^-T e_m scaled so
  that g^T B g = 1). The prototype of this arithmetic measured at most 8.9e-16 on these matrices; the bar is ten times
  that and far below anything a wrong operation order or a dropped term would give.
* PCG with the oracle operator takes fewer iterations than PCG with Jacobi (oracle.krylov.pcg, tau 1e-8,
  b = A rand(seed 12345)).
"""
import functools
import os
import re

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import fsai_oracle as fo
from conftest import GOLDEN, REPO
from oracle import fdlap, krylov


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name.startswith("negfd"):
        return (-fdlap.fd_laplacian_2d(-1.0, 1.0, int(name[5:]))).tocsr()
    if name.startswith("fd"):
        return fdlap.fd_laplacian_2d(-1.0, 1.0, int(name[2:])).tocsr()
    if name == "dh8":
        return scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _operator(name, power):
    return fo.FSAI(_matrix(name), power=power)


def _tril_pattern(P):
    """Sorted (row, column) structure of the lower triangle of P."""
    T = sp.tril(sp.csr_matrix((np.ones(P.nnz), P.indices.copy(), P.indptr.copy()), shape=P.shape)).tocsr()
    T.sort_indices()
    return T.indptr, T.indices


@pytest.mark.parametrize("name,sign", [("negfd16", 1), ("fd16", -1), ("dh8", 1)])
@pytest.mark.parametrize("power", [1, 2])
def test_oracle_is_an_inverse_cholesky_factor_on_the_pattern(name, sign, power):
    A = _matrix(name)
    op = _operator(name, power)
    G = op.G
    assert op.sign == sign
    # lower triangular, on exactly tril(pattern), rows in ascending column order
    pattern = A if power == 1 else (A @ A).tocsr()
    ip, ix = _tril_pattern(pattern)
    assert np.array_equal(G.indptr, ip) and np.array_equal(G.indices, ix)
    assert sp.triu(G, k=1).nnz == 0 and np.all(G.diagonal() > 0.0)
    assert op.max_row == np.max(np.diff(ip)) <= fo.ROW_CAP
    sA = (float(sign) * A).toarray()
    Gd = G.toarray()
    err = np.max(np.abs(np.diag(Gd @ sA @ Gd.T) - 1.0))
    print("%s power %d: max |diag(G sA G^T) - 1| = %.3e, max row %d" % (name, power, err, op.max_row))
    assert err <= 1e-14
    # apply() is the symmetric product (sign G^T) G, definite with A's sign
    v = np.random.default_rng(3).standard_normal(A.shape[0])
    y = op(v)
    assert np.array_equal(y, fo.apply(G, op.sign, v))
    dense = sign * (Gd.T @ (Gd @ v))      # the same sums in another order: a few ulp of ||G||^2 ||v|| per entry
    assert np.linalg.norm(y - dense) <= 1e-13 * np.linalg.norm(dense)
    assert sign * np.dot(v, y) > 0.0


@pytest.mark.parametrize("name", ["negfd32", "dh8"])
@pytest.mark.parametrize("power", [1, 2])
def test_oracle_pcg_takes_fewer_iterations_than_jacobi(name, power):
    A = _matrix(name)
    b = A @ np.random.default_rng(12345).random(A.shape[0])
    jac = krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=krylov.jacobi_form(A))
    ref = krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=_operator(name, power))
    print("%s: PCG iterations Jacobi %d, FSAI(%d) %d" % (name, jac["iters"], power, ref["iters"]))
    assert jac["success"] and ref["success"] and ref["iters"] < jac["iters"]
    assert np.linalg.norm(b - A @ ref["soln"]) <= 1e-7 * np.linalg.norm(b)


def test_powers_order_the_iteration_counts():
    """The richer pattern is the better preconditioner on the model problem."""
    A = _matrix("negfd32")
    b = A @ np.random.default_rng(12345).random(A.shape[0])
    it = [krylov.pcg(A, b, maxiter=1000, tau=1e-8, precond=_operator("negfd32", p))["iters"] for p in (1, 2)]
    assert it[1] < it[0]


def test_oracle_refuses_a_matrix_that_is_not_definite():
    with pytest.raises(fo.PivotError) as e:           # sign +1 from row 0, then a negative pivot in row 1
        fo.fsai(sp.csr_matrix(np.diag([1.0, -1.0])))
    assert e.value.row == 1
    with pytest.raises(fo.PivotError) as e:           # a pivot that fails only inside the small Cholesky
        fo.fsai(sp.csr_matrix(np.array([[1.0, 2.0], [2.0, 1.0]])))
    assert e.value.row == 1
    with pytest.raises(ValueError):                   # no sign without row 0's diagonal
        fo.fsai(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 2.0]])))


def test_oracle_refuses_bad_structure():
    A = _matrix("negfd16")
    n = A.shape[0]
    nodiag = sp.csr_matrix(A - sp.diags(A.diagonal()))
    nodiag.eliminate_zeros()
    with pytest.raises(ValueError):                   # a pattern row without its diagonal
        fo.fsai(A, nodiag)
    with pytest.raises(ValueError):                   # duplicate column in row 0
        fo.fsai(sp.csr_matrix((np.array([2.0, 1.0, 1.0, 3.0]), np.array([0, 0, 0, 1]), np.array([0, 2, 4])),
                              shape=(2, 2)))
    with pytest.raises(ValueError):
        fo.fsai(sp.csr_matrix(np.ones((2, 3))))
    with pytest.raises(OverflowError):                # a pattern row over the cap
        fo.fsai(A, sp.csr_matrix(np.tril(np.ones((n, n)))))


def test_unsorted_rows_and_upper_pattern_entries_do_not_matter():
    A = _matrix("negfd16")
    ip = A.indptr
    assert any(np.any(np.diff(A.indices[ip[i]:ip[i + 1]]) < 0) for i in range(A.shape[0])), "rows are stored sorted"
    S = A.copy()
    S.sort_indices()
    Ga, sa = fo.fsai(A)
    Gs, ss = fo.fsai(S, sp.tril(S).tocsr())
    assert sa == ss == 1
    assert np.array_equal(Ga.indptr, Gs.indptr) and np.array_equal(Ga.indices, Gs.indices)
    assert np.array_equal(Ga.data.view(np.uint64), Gs.data.view(np.uint64))


def test_classes_are_importable():
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import FSAI, FSAIPreconditioner, FSAIPreconditionerType
    from pysolvers_amd.Linear.Preconditioner import DeviceOperator, GenericPreconditioner
    from pysolvers_amd.Linear.PreconditionerType import PreconditionerType
    assert psk.FSAI is FSAI is FSAIPreconditionerType and psk.FSAIPreconditioner is FSAIPreconditioner
    assert isinstance(FSAI(), PreconditionerType) and FSAI().power == 1 and FSAI(power=2).power == 2
    assert issubclass(FSAIPreconditioner, DeviceOperator) and issubclass(FSAIPreconditioner, GenericPreconditioner)
    assert FSAIPreconditioner.device_kind == N.PSK_PREC_FSAI == 6
    assert N.PSK_FSAI_ROW_CAP == fo.ROW_CAP == 64 and N.PSK_FSAI_WAVE_ONLY == 1 and N.lib.psk_abi_version() == 4
    assert hasattr(psk.DeviceCSR, "fsai")
    assert {"psk_csr_fsai", "psk_prec_create_fsai", "psk_prec_fsai_info"} <= set(N.SIGNATURES)
    with pytest.raises(ValueError):                   # before any device work
        FSAIPreconditioner(None, power=3)


def test_header_declares_the_entry_points():
    raw = open(os.path.join(REPO, "include", "psk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+psk_csr_fsai\s*\(\s*const\s+psk_csr\s*\*\s*A\s*,\s*const\s+psk_csr\s*\*\s*pattern\s*,"
                     r"\s*int32_t\s+flags\s*,\s*psk_csr\s*\*\*\s*G\s*,\s*int32_t\s*\*\s*sign\s*\)\s*;", txt)
    assert re.search(r"\bint\s+psk_prec_create_fsai\s*\(\s*const\s+psk_csr\s*\*\s*A\s*,\s*const\s+psk_csr\s*\*\s*pattern"
                     r"\s*,\s*int32_t\s+flags\s*,\s*psk_prec\s*\*\*\s*out\s*\)\s*;", txt)
    assert re.search(r"\bint\s+psk_prec_fsai_info\s*\(\s*const\s+psk_prec\s*\*\s*M\s*,\s*int32_t\s*\*\s*sign\s*,"
                     r"\s*int64_t\s*\*\s*nnz_g\s*,\s*int32_t\s*\*\s*max_row\s*\)\s*;", txt)
    for name, value in (("PSK_PREC_FSAI", 6), ("PSK_FSAI_ROW_CAP", 64), ("PSK_FSAI_WAVE_ONLY", 1), ("PSK_ABI_VERSION", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), txt), name
