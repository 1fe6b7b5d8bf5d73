"""ILU(0) without a GPU: the oracle (tests/ilu0_oracle.py) is a factorisation of A on A's pattern, refuses a zero
pivot and does not depend on the stored order of a row; the Python classes import and the header declares the
two entry points.

Bar: (L U - A) restricted to A's pattern <= 1e-12 max|A|. ILU(0) makes (L U)_ij = a_ij exactly in exact arithmetic
on the pattern; in floating point an entry is a_ij minus at most (row length) rounded products and differences,
each within 2^-53 of values bounded by a few max|A| on these diagonally dominant matrices: 1e-12 is > 100x that.
"""
import os
import re

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import bicgstab_oracle as bo
import ilu0_oracle as io0
from conftest import GOLDEN, REPO
from oracle import fdlap


def _cases():
    return {
        "fd17": lambda: fdlap.fd_laplacian_2d(-1.0, 1.0, 17).tocsr(),
        "cd33": lambda: bo.cd_matrix(33, 0.5),
        "dh8": lambda: scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr(),
        "dh10": lambda: scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-10.mtx")).tocsr(),
        "rand511": lambda: bo.random_nonsym(511, seed=511),
        "fd300": lambda: fdlap.fd_laplacian_2d(-1.0, 1.0, 300).tocsr(),
    }


@pytest.mark.parametrize("name", list(_cases()))
def test_oracle_factors_a_on_its_pattern(name):
    A = _cases()[name]()
    F = io0.ilu0(A)
    S = io0.sorted_copy(A)
    assert np.array_equal(F.indptr, S.indptr) and np.array_equal(F.indices, S.indices)
    L, U = io0.split(F)
    R = (L @ U - S).tocsr()
    mask = S.copy()
    mask.data[:] = 1.0
    err = abs(R.multiply(mask)).max()
    amax = np.max(np.abs(S.data))
    print("%s: max |L U - A| on the pattern = %.3e max|A|" % (name, err / amax))
    assert err <= 1e-12 * amax


def test_oracle_refuses_a_zero_pivot():
    A = sp.csr_matrix((np.array([0.0, 1.0, 1.0, 0.0]), np.array([0, 1, 0, 1]), np.array([0, 2, 4])), shape=(2, 2))
    with pytest.raises(io0.PivotError) as e:
        io0.ilu0(A)
    assert e.value.row == 0
    # a pivot that only becomes zero during the elimination: [[1, 1], [1, 1]] -> u_11 = 1 - 1 * 1
    with pytest.raises(io0.PivotError) as e:
        io0.ilu0(sp.csr_matrix(np.ones((2, 2))))
    assert e.value.row == 1


def test_oracle_refuses_bad_structure():
    with pytest.raises(ValueError):     # no stored diagonal in row 1
        io0.ilu0(sp.csr_matrix((np.array([2.0, 1.0, 1.0]), np.array([0, 1, 0]), np.array([0, 2, 3])), shape=(2, 2)))
    with pytest.raises(ValueError):     # duplicate column in row 0
        io0.ilu0(sp.csr_matrix((np.array([2.0, 1.0, 1.0, 3.0]), np.array([0, 0, 0, 1]), np.array([0, 2, 4])),
                               shape=(2, 2)))
    with pytest.raises(ValueError):
        io0.ilu0(sp.csr_matrix(np.ones((2, 3))))


@pytest.mark.parametrize("name", ["fd17", "rand511"])
def test_unsorted_rows_give_the_sorted_copys_factors(name):
    A = _cases()[name]()
    ip = A.indptr
    assert any(np.any(np.diff(A.indices[ip[i]:ip[i + 1]]) < 0) for i in range(A.shape[0])), "rows are stored sorted"
    S = A.copy()
    S.sort_indices()
    Fa, Fs = io0.ilu0(A), io0.ilu0(S)
    assert np.array_equal(Fa.indptr, Fs.indptr) and np.array_equal(Fa.indices, Fs.indices)
    assert np.array_equal(Fa.data.view(np.uint64), Fs.data.view(np.uint64))


def test_classes_are_importable():
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import (ILU0Preconditioner, LeftILU0, LeftILU0Preconditioner, RightILU0,
                                      RightILU0Preconditioner)
    from pysolvers_amd.Linear.PreconditionerType import PreconditionerType
    assert psk.RightILU0 is RightILU0 and psk.LeftILU0 is LeftILU0
    assert isinstance(RightILU0(), PreconditionerType) and isinstance(LeftILU0(), PreconditionerType)
    assert RightILU0Preconditioner.device_kind == N.PSK_PREC_ILU
    assert LeftILU0Preconditioner.device_kind == N.PSK_PREC_IDENTITY and LeftILU0Preconditioner.device_handle is None
    assert issubclass(RightILU0Preconditioner, ILU0Preconditioner) and hasattr(ILU0Preconditioner, "factors")
    assert hasattr(psk.DeviceCSR, "ilu0")
    assert "psk_csr_ilu0" in N.SIGNATURES and "psk_prec_create_ilu0" in N.SIGNATURES


def test_header_declares_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "psk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+psk_csr_ilu0\s*\(\s*const\s+psk_csr\s*\*\s*A\s*,\s*psk_csr\s*\*\*\s*F\s*\)\s*;", txt)
    assert re.search(r"\bint\s+psk_prec_create_ilu0\s*\(\s*const\s+psk_csr\s*\*\s*A\s*,\s*psk_prec\s*\*\*\s*out\s*\)\s*;",
                     txt)
    assert "#define PSK_ABI_VERSION 4" in open(os.path.join(REPO, "include", "psk.h")).read()
