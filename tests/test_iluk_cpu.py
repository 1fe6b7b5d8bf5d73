"""CPU tests of the level-of-fill ILU(k) definition (tests/iluk_oracle.py, the rule include/psk.h states for
psk_csr_iluk_pattern) and of the binding's argument checks; no GPU.

Iteration counts of the oracle factor as a right preconditioner, recorded when the feature was written (tau = 1e-8,
b = default_rng(3).standard_normal(n), oracle.krylov; the convection-diffusion operator is cd 64 with c = 0.2, the
operator and c of tools/idrs_vs_bicgstab.py):

    matrix      k   nnz(P)/nnz(A)   GMRES   GMRES(30)   PCG
    -FD 64^2    0   1.00            63      89          65
    -FD 64^2    1   1.39            41      42          42
    -FD 64^2    2   1.78            33      34          34
    -FD 64^2    3   2.55            25      25          25
    cd 64       0   1.00            47      61
    cd 64       1   1.39            29      29
    cd 64       2   1.78            23      23
    cd 64       3   2.55            17      17
"""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import bicgstab_oracle as bo
import ilu0_oracle as io0
import iluk_oracle as ko
from conftest import REPO
from oracle import fdlap, krylov

GMRES_COUNTS = {"negfd64": [63, 41, 33], "cd64": [47, 29, 23]}
PCG_COUNTS = {"negfd64": [65, 42, 34]}


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name.startswith("negfd"):
        return (-fdlap.fd_laplacian_2d(-1.0, 1.0, int(name[5:]))).tocsr()
    if name == "cd64":
        return bo.cd_matrix(64, 0.2)
    if name == "arrow":
        return arrow(40)
    if name in ("skip5", "skip5sym"):
        return skip5(name == "skip5sym")
    if name == "skip11":
        return skip11()
    if name == "skip880":
        return sp.block_diag([skip11()] * 80, format="csr")
    raise KeyError(name)


def arrow(n):
    """Dense last row and column on a diagonal, then the ordering reversed: the dense row and column are stored
    first, so eliminating row 0 fills everything."""
    D = sp.lil_matrix((n, n))
    D.setdiag(4.0 + np.arange(n))
    D[n - 1, :] = -1.0
    D[:, n - 1] = -1.0
    D[n - 1, n - 1] = 4.0 * n
    p = np.arange(n)[::-1]
    return D.tocsr()[p][:, p].tocsr()


def skip5(symmetric):
    """Diagonal plus (3,0), (0,2), (2,1), (1,4) (and their transposes): (3,2) and (2,4) get level 1, (3,4) level 3 from
    that pair, and nothing has level 2 — a round that adds nothing is followed by one that does."""
    e = [(3, 0), (0, 2), (2, 1), (1, 4)]
    if symmetric:
        e += [(b, a) for a, b in e]
    r, c = [a for a, _ in e] + list(range(5)), [b for _, b in e] + list(range(5))
    return sp.csr_matrix((np.array([-1.0] * len(e) + [4.0] * 5), (r, c)), shape=(5, 5))


def skip11():
    """11 x 11, found by a search over random patterns: its levels are {0, 1, 2, 5, 6}, so rounds 3 and 4 add nothing
    and rounds 5 and 6 do."""
    e = [(0, 7), (1, 4), (2, 4), (3, 0), (3, 1), (3, 4), (4, 5), (5, 3), (7, 10), (9, 1)]
    r, c = [a for a, _ in e] + list(range(11)), [b for _, b in e] + list(range(11))
    return sp.csr_matrix((np.array([-1.0] * len(e) + [8.0] * 11), (r, c)), shape=(11, 11))


@functools.lru_cache(maxsize=None)
def _pattern(name, k):
    P, Lev = ko.pattern(_matrix(name), k)
    for M in (P, Lev):
        M.data.setflags(write=False)
    return P, Lev


def _same(A, B):
    return (np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(A.data.view(np.uint64), B.data.view(np.uint64)))


@pytest.mark.parametrize("name", ["negfd16", "cd64", "arrow"])
def test_level_zero_is_the_sorted_copy(name):
    P, Lev = _pattern(name, 0)
    assert _same(P, io0.sorted_copy(_matrix(name)))
    assert not Lev.data.any() and np.array_equal(Lev.indices, P.indices)


def test_level_zero_sorts_shuffled_rows_and_keeps_stored_zeros():
    A = _matrix("negfd16").tocoo()
    rng = np.random.default_rng(5)
    p = rng.permutation(A.nnz)
    vals = A.data.copy()
    vals[0] = 0.0
    B = sp.csr_matrix((vals[p], (A.row[p], A.col[p])), shape=A.shape)
    B.has_sorted_indices = False
    P, _ = ko.pattern(B, 0)
    assert P.nnz == A.nnz and np.count_nonzero(P.data == 0.0) == 1
    assert all(np.all(np.diff(P.indices[P.indptr[i]:P.indptr[i + 1]]) > 0) for i in range(P.shape[0]))
    P1, L1 = ko.pattern(B, 1)          # a stored zero is structure: the same fill as with a nonzero there
    assert np.array_equal(P1.indices, _pattern("negfd16", 1)[0].indices)
    assert np.array_equal(L1.data, _pattern("negfd16", 1)[1].data)


@pytest.mark.parametrize("name", ["negfd16", "arrow"])
def test_patterns_nest_and_levels_are_kept(name):
    prev = None
    for k in range(4):
        P, Lev = _pattern(name, k)
        assert Lev.data.max() <= k and np.array_equal(Lev.data, np.round(Lev.data))
        cur = {(i, int(c)): lv for i in range(P.shape[0])
               for c, lv in zip(P.indices[P.indptr[i]:P.indptr[i + 1]], Lev.data[P.indptr[i]:P.indptr[i + 1]])}
        if prev is not None:
            assert all(e in cur and cur[e] == lv for e, lv in prev.items())     # a level never changes as k grows
            assert all(lv == k for e, lv in cur.items() if e not in prev)       # what k adds has level k
        prev = cur


def test_longest_row_of_negfd16():
    assert [int(np.diff(_pattern("negfd16", k)[0].indptr).max()) for k in range(4)] == [5, 7, 9, 13]


def test_fill_ratio_of_negfd64():
    A = _matrix("negfd64")
    assert ["%.2f" % (_pattern("negfd64", k)[0].nnz / A.nnz) for k in range(4)] == ["1.00", "1.39", "1.78", "2.55"]


def test_padded_values():
    A = io0.sorted_copy(_matrix("cd64"))
    P, Lev = _pattern("cd64", 2)
    stored = Lev.data == 0.0
    assert np.array_equal(P.data[stored].view(np.uint64), A.data.view(np.uint64))
    assert np.array_equal(P.indices[stored], A.indices)
    assert np.all(P.data[~stored].view(np.uint64) == 0)                         # +0.0, not -0.0


def test_a_level_may_be_skipped():
    """Levels 1 + 1 make a level 3 where no level 2 exists: an empty round does not end the fill."""
    for name, nnz in (("skip5", [9, 11, 11, 12, 12]), ("skip5sym", [13, 17, 17, 19, 19])):
        assert [_pattern(name, k)[0].nnz for k in range(5)] == nnz
        assert sorted(set(_pattern(name, 4)[1].data)) == [0.0, 1.0, 3.0]
    for name, blocks in (("skip11", 1), ("skip880", 80)):
        assert sorted(set(_pattern(name, 8)[1].data)) == [0.0, 1.0, 2.0, 5.0, 6.0]
        nnz = [_pattern(name, k)[0].nnz for k in (2, 3, 4, 5, 6, 8)]
        assert nnz[0] == nnz[1] == nnz[2] < nnz[3] < nnz[4] == nnz[5]
        assert _matrix(name).shape[0] == 11 * blocks and nnz[5] == blocks * _pattern("skip11", 8)[0].nnz


def test_arrow_fills_completely_at_level_one():
    A = _matrix("arrow")
    n = A.shape[0]
    assert A.nnz == 3 * n - 2 and A[0].nnz == n and A[:, 0].nnz == n
    assert _pattern("arrow", 0)[0].nnz == A.nnz
    P, Lev = _pattern("arrow", 1)
    assert P.nnz == n * n and Lev.data.max() == 1.0
    assert _pattern("arrow", 2)[0].nnz == n * n


@functools.lru_cache(maxsize=None)
def _counts(name, k):
    A = _matrix(name)
    b = np.random.default_rng(3).standard_normal(A.shape[0])
    M = io0.apply(io0.ilu0(_pattern(name, k)[0]))
    g = krylov.gmres(A, b, maxiter=400, tau=1e-8, precond=M)
    assert g["success"]
    c = None
    if name == "negfd64":
        c = krylov.pcg(A, b, maxiter=400, tau=1e-8, precond=M)
        assert c["success"]
        c = c["iters"]
    return g["iters"], c


@pytest.mark.parametrize("name", ["negfd64", "cd64"])
def test_iteration_counts_fall_with_the_level(name):
    g = [_counts(name, k)[0] for k in range(3)]
    assert g[0] > g[1] > g[2]
    assert g == GMRES_COUNTS[name]
    if name in PCG_COUNTS:
        c = [_counts(name, k)[1] for k in range(3)]
        assert c[0] > c[1] > c[2]
        assert c == PCG_COUNTS[name]


def test_oracle_refuses_bad_input():
    A = _matrix("negfd16")
    for k in (-1, 9, 1.5, True):
        with pytest.raises(ValueError):
            ko.pattern(A, k)
    with pytest.raises(ValueError):     # no stored diagonal in row 1
        ko.pattern(sp.csr_matrix((np.array([2.0, 1.0, 1.0]), np.array([0, 1, 0]), np.array([0, 2, 3])), shape=(2, 2)), 1)
    with pytest.raises(ValueError):     # duplicate column in row 0
        ko.pattern(sp.csr_matrix((np.array([2.0, 1.0, 1.0, 3.0]), np.array([0, 0, 0, 1]), np.array([0, 2, 4])),
                                 shape=(2, 2)), 1)


# ---- the binding ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [True, False, 1.0, 1.5, "1", None, -1, 9])
def test_a_bad_level_is_a_value_error(k):
    import pysolvers_amd as psk
    for make in (psk.RightILUK, psk.LeftILUK):
        with pytest.raises(ValueError):
            make(k)
        with pytest.raises(ValueError):
            make(k=k, sweeps=2)
    with pytest.raises(ValueError):     # checked before the matrix is looked at
        psk.RightILUKPreconditioner(None, k=k)
    with pytest.raises(ValueError):
        psk.DeviceCSR(None, 4, 4).iluk_pattern(k)


def test_good_levels_and_defaults():
    import pysolvers_amd as psk
    assert psk.RightILUK().k == 1 and psk.LeftILUK().k == 1 and psk.RightILUK().sweeps is None
    assert [psk.RightILUK(k).k for k in range(9)] == list(range(9))
    assert psk.RightILUK(np.int32(3)).k == 3 and type(psk.RightILUK(np.int64(3)).k) is int
    assert psk.RightILUK(2, sweeps=(1, 2)).sweeps == (1, 2)


def test_a_sharded_matrix_is_a_value_error():
    import pysolvers_amd as psk
    sharded = psk.DeviceCSR(None, 4, 4, comm=object(), row_begin=0, row_end=4, n_global=8)
    with pytest.raises(ValueError, match="sharded"):
        sharded.iluk_pattern(1)
    with pytest.raises(ValueError, match="sharded"):
        psk.RightILUK(1).form(sharded)
    with pytest.raises(ValueError, match="sharded"):
        psk.LeftILUK(1).form(sharded)


def test_classes_are_importable():
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import (ILUKPreconditioner, LeftILUK, LeftILUKPreconditioner, RightILUK,
                                      RightILUKPreconditioner)
    from pysolvers_amd.Linear.PreconditionerType import PreconditionerType
    from pysolvers_amd.Linear.TriangularSolve import TriangularSolveChain
    assert psk.RightILUK is RightILUK and psk.LeftILUK is LeftILUK
    assert psk.ILUKPreconditioner is ILUKPreconditioner and psk.RightILUKPreconditioner is RightILUKPreconditioner
    assert psk.LeftILUKPreconditioner is LeftILUKPreconditioner
    assert isinstance(RightILUK(), PreconditionerType) and isinstance(LeftILUK(), PreconditionerType)
    assert RightILUKPreconditioner.device_kind == N.PSK_PREC_ILU
    assert LeftILUKPreconditioner.device_kind == N.PSK_PREC_IDENTITY and LeftILUKPreconditioner.device_handle is None
    assert issubclass(RightILUKPreconditioner, ILUKPreconditioner) and hasattr(ILUKPreconditioner, "factors")
    for name in ("schedule", "grid_info", "sweeps"):
        assert getattr(ILUKPreconditioner, name) is getattr(TriangularSolveChain, name)
    assert hasattr(psk.DeviceCSR, "iluk_pattern")
    for name in ("RightILUK", "LeftILUK", "ILUKPreconditioner", "LeftILUKPreconditioner", "RightILUKPreconditioner"):
        assert name in psk.__all__


def test_signatures_cover_the_header():
    from pysolvers_amd import _native as N
    raw = open(os.path.join(REPO, "include", "psk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+psk_csr_iluk_pattern\s*\(\s*const\s+psk_csr\s*\*\s*A\s*,\s*int32_t\s+k\s*,\s*psk_csr\s*\*\*"
                     r"\s*P\s*,\s*psk_csr\s*\*\*\s*Lev\s*\)\s*;", txt)
    assert re.search(r"\bint\s+psk_prec_create_iluk\s*\(\s*const\s+psk_csr\s*\*\s*A\s*,\s*int32_t\s+k\s*,\s*psk_prec\s*\*\*"
                     r"\s*out\s*\)\s*;", txt)
    assert re.search(r"#define\s+PSK_ILUK_MAX_LEVEL\s+8\b", txt) and re.search(r"#define\s+PSK_ILUK_ROW_CAP\s+512\b", txt)
    assert "#define PSK_ABI_VERSION 4" in raw
    declared = sorted(set(re.findall(r"\b(psk_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(N.SIGNATURES) == declared
    assert len(N.SIGNATURES["psk_csr_iluk_pattern"][1]) == 4 and len(N.SIGNATURES["psk_prec_create_iluk"][1]) == 3
    assert "psk_lab_iluk_timing" in N.LAB_SIGNATURES
    lab = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "psk_lab.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+psk_lab_iluk_timing\s*\(\s*double\s*\*\s*out\s*\)\s*;", lab)
    from pysolvers_amd.Linear.ILUKPreconditioner import ILUK_MAX_LEVEL
    assert ILUK_MAX_LEVEL == ko.MAX_LEVEL == 8
