"""GPU tests of level-of-fill ILU(k) (psk_csr_iluk_pattern / psk_prec_create_iluk, iluk.hip;
pysolvers_amd.Linear.RightILUK / LeftILUK, DeviceCSR.iluk_pattern).

Bars (written here, not inferred):
* Pattern: indptr, indices and the levels (as integers) EQUAL those of tests/iluk_oracle.py, the sequential rule
  include/psk.h states; the values are bitwise A's where A stores the entry and +0.0 elsewhere.
* Factor: indptr, indices and the uint64 view of the values equal ilu0_oracle.ilu0 of the oracle's padded matrix;
  k = 0 applies are bitwise RightILU0's; two forms, scipy or DeviceCSR input and every lanes-per-row geometry of the
  symbolic kernels (PSK_ILUK_WIDTH = 1, 4, 16, 64) give the same bits.
* Apply: max |psk_prec_apply(v) - apply(F)(v)| <= 1e-12 max |apply(F)(v)|, RTOL_APPLY of tests/test_gpu_ilu0.py
  (imported from there); the swept apply against tests/trisweep_oracle.py at that same bar, the one
  tests/test_gpu_trisweep.py uses.
* Solvers: iteration counts equal the oracle's run with the oracle factor's apply (oracle.krylov for GMRES and PCG;
  tests/bicgstab_oracle.py and tests/idrs_oracle.py, the project's oracles of those two methods, for BiCGStab and
  IDR(4)); histories within RTOL_RESID = 1e-10 of ||b||; counts strictly below RightILU0's on the same system.
  Measured on an MI355X: at most 9.0e-15 ||b|| for GMRES, BiCGStab and PCG; IDR(4) 9.9e-11 at k = 1 and 1.1e-12 at
  k = 2 (IDR(s) amplifies the summation order of the device's dot products; the run is bitwise repeatable).
* Errors are error returns that write no output and leave no sticky state.

Cases (tests/mcgs_cases.py unless stated): negfd16; negfd33 (odd width: tiles end mid-row); dh8, dh10 (block
structure, no fill beyond the blocks); nonsym (nonsymmetric pattern); shuffled (shuffled rows, stored zeros that count
as structure); one, diag (no round adds anything); arrow (test_iluk_cpu.arrow: 4 lanes per row by the
mean, 38 new columns in a row: over the narrow set's 32, so the 64-lane instance takes the row); rand700 (700 rows, 30
entries per row inside a band of half-width 100, shuffled: 16 lanes per row, rows grow to 200 entries — longer than a
wave — and gain up to 136 columns in round 1: over the 128 of the 16-lane set); skip5, skip5sym (test_iluk_cpu.skip5:
levels {0, 1, 3}: round 2 adds nothing and round 3 adds an entry), skip11 and skip880 (80 diagonal blocks of skip11, more
than one workgroup: levels {0, 1, 2, 5, 6}, two empty rounds before two that add).
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import bicgstab_oracle as bo
import idrs_oracle as io_
import ilu0_oracle as io0
import iluk_oracle as ko
import mcgs_cases
import trisweep_oracle as tso
from oracle import krylov
from test_gpu_ilu0 import RTOL_APPLY, RTOL_RESID
from test_iluk_cpu import arrow, skip5, skip11

pytestmark = pytest.mark.gpu

assert (RTOL_APPLY, RTOL_RESID) == (1e-12, 1e-10)
TAU = 1e-10
MAXITER = 400
NAMES = ("negfd16", "negfd33", "dh8", "dh10", "nonsym", "shuffled", "one", "diag", "arrow", "rand700")
SKIPS = [(n, k) for n in ("skip5", "skip5sym") for k in (2, 3, 4)] + [(n, k) for n in ("skip11", "skip880")
                                                                   for k in (2, 4, 5, 6, 8)]
PATTERN_CASES = [(n, k) for n in NAMES for k in range(4)] + [("negfd16", 8)] + SKIPS
FACTOR_CASES = PATTERN_CASES
APPLY_CASES = [(n, k) for n in NAMES for k in (1, 3)]


@pytest.fixture(scope="module")
def psk():
    import pysolvers_amd
    from pysolvers_amd import _native as N
    assert N.device_count() >= 1, "no GPU visible to libpsk"
    return pysolvers_amd


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def rand700(n=700, per_row=30, half=100, seed=700):
    rng = np.random.default_rng(seed)
    cols, vals = [], []
    for i in range(n):
        cand = np.setdiff1d(np.arange(max(0, i - half), min(n, i + half + 1)), [i])
        c = rng.choice(cand, size=per_row - 1, replace=False)
        v = rng.uniform(-1.0, 1.0, c.size)
        order = rng.permutation(per_row)                    # stored unsorted, the diagonal anywhere
        cols.append(np.concatenate([c, [i]])[order])
        vals.append(np.concatenate([v, [np.abs(v).sum() + 1.0]])[order])
    A = sp.csr_matrix((np.concatenate(vals), np.concatenate(cols).astype(np.int32),
                       np.arange(0, n * per_row + 1, per_row, dtype=np.int32)), shape=(n, n))
    A.has_sorted_indices = False
    return A


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name == "arrow":
        A = arrow(40)
    elif name == "rand700":
        A = rand700()
    elif name in ("skip5", "skip5sym"):
        A = skip5(name == "skip5sym")
    elif name == "skip11":
        A = skip11()
    elif name == "skip880":
        A = sp.block_diag([skip11()] * 80, format="csr")
    elif name.startswith("cd"):
        A = bo.cd_matrix(int(name[2:]), 0.2)
    else:
        return mcgs_cases.matrix(name)
    for a in (A.data, A.indices, A.indptr):
        a.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _oracle_pattern(name, k):
    """(P, Lev) of the oracle: computed once, shared, never written to."""
    P, Lev = ko.pattern(_matrix(name), k)
    P.data.setflags(write=False)
    Lev.data.setflags(write=False)
    return P, Lev


@functools.lru_cache(maxsize=None)
def _oracle_factor(name, k):
    F = io0.ilu0(_oracle_pattern(name, k)[0])
    F.data.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def _rhs(name):
    b = np.random.default_rng(3).standard_normal(_matrix(name).shape[0])
    b.setflags(write=False)
    return b


def _same_csr(F, ref):
    assert np.array_equal(F.indptr, ref.indptr)
    assert np.array_equal(F.indices, ref.indices)
    assert np.array_equal(_bits(F.data), _bits(ref.data))


def _ctl(psk, **kw):
    kw.setdefault("showIters", False)
    kw.setdefault("showFinal", False)
    kw.setdefault("maxiter", MAXITER)
    kw.setdefault("tau", TAU)
    return psk.CommonSolverArgs(**kw)


# ---- 1. the pattern ------------------------------------------------------------------------------------------------

def test_cases_have_the_shapes_they_are_chosen_for():
    A = _matrix("rand700")
    assert A.shape == (700, 700) and np.all(np.diff(A.indptr) == 30)
    assert any(np.any(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) < 0) for i in range(700))
    grown = np.diff(_oracle_pattern("rand700", 1)[0].indptr)
    assert grown.max() > 64 and (grown - 30).max() > 128           # over a wave's lanes; over the 16-lane set
    assert np.diff(_oracle_pattern("rand700", 3)[0].indptr).max() <= 512
    arw = np.diff(_oracle_pattern("arrow", 1)[0].indptr) - np.diff(io0.sorted_copy(_matrix("arrow")).indptr)
    assert arw.max() > 32 and _matrix("arrow").nnz / 40 <= 8.0      # over the 4-lane set
    assert np.count_nonzero(_matrix("shuffled").data == 0.0) == 2
    assert sorted(set(_oracle_pattern("skip5", 4)[1].data)) == [0.0, 1.0, 3.0]
    assert sorted(set(_oracle_pattern("skip880", 8)[1].data)) == [0.0, 1.0, 2.0, 5.0, 6.0]
    assert _oracle_pattern("skip880", 4)[0].nnz == _oracle_pattern("skip880", 2)[0].nnz < _oracle_pattern("skip880", 5)[0].nnz
    assert _oracle_pattern("diag", 3)[0].nnz == _matrix("diag").nnz and _oracle_pattern("one", 3)[0].nnz == 1


@pytest.mark.parametrize("name,k", PATTERN_CASES)
def test_pattern_and_levels_equal_the_oracle(psk, name, k):
    A = _matrix(name)
    Pref, Lref = _oracle_pattern(name, k)
    dA = psk.DeviceCSR.from_scipy(A)
    P, Lev = dA.iluk_pattern(k, levels=True)
    assert isinstance(P, psk.DeviceCSR) and isinstance(Lev, psk.DeviceCSR)
    assert P.shape == A.shape and P.nnz == Pref.nnz == Lev.nnz
    P, Lev = P.to_scipy(), Lev.to_scipy()
    print("%s k=%d: nnz %d -> %d, longest row %d" % (name, k, A.nnz, P.nnz, np.diff(P.indptr).max()))
    assert np.array_equal(P.indptr, Pref.indptr) and np.array_equal(P.indices, Pref.indices)
    assert np.array_equal(Lev.indptr, Pref.indptr) and np.array_equal(Lev.indices, Pref.indices)
    assert np.array_equal(Lev.data, np.round(Lev.data))
    assert np.array_equal(Lev.data.astype(np.int64), Lref.data.astype(np.int64))
    assert np.array_equal(_bits(P.data), _bits(Pref.data))          # A's bits or +0.0
    alone = dA.iluk_pattern(k)                                        # levels not asked for: P alone, the same
    assert isinstance(alone, psk.DeviceCSR)
    _same_csr(alone.to_scipy(), Pref)


# ---- 2. the factor, bitwise ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k", FACTOR_CASES)
def test_factor_bitwise_vs_oracle(psk, name, k):
    A, ref = _matrix(name), _oracle_factor(name, k)
    M = psk.RightILUK(k).form(A)
    assert M.level == k and M.n == A.shape[0]
    _same_csr(M.factors(), ref)
    assert M.fill_ratio == ref.nnz / A.nnz
    info = M.device_info()
    assert info["kind"] == psk._native.PSK_PREC_ILU and info["n"] == A.shape[0]
    assert info["nnz_l"] + info["nnz_u"] + A.shape[0] == ref.nnz
    dA = psk.DeviceCSR.from_scipy(A)
    _same_csr(psk.RightILUK(k).form(dA).factors(), ref)              # a second form, DeviceCSR input
    _same_csr(dA.iluk_pattern(k).ilu0().to_scipy(), ref)


@pytest.mark.parametrize("name", ["negfd33", "shuffled", "nonsym", "rand700"])
def test_level_zero_is_ilu0_to_the_bit(psk, name):
    A, v = _matrix(name), np.array(_rhs(name))
    Mk, M0 = psk.RightILUK(0).form(A), psk.RightILU0().form(A)
    _same_csr(Mk.factors(), M0.factors())
    assert Mk.fill_ratio == 1.0
    assert np.array_equal(_bits(Mk.applyRight(v)), _bits(M0.applyRight(v)))
    left = psk.LeftILUK(0).form(A)
    assert left.applyRight(v) is v
    assert np.array_equal(_bits(left.applyLeft(v)), _bits(M0.applyRight(v)))


@pytest.mark.parametrize("name,k", [("negfd33", 3), ("arrow", 1), ("rand700", 2), ("nonsym", 2), ("diag", 1),
                                    ("skip880", 6)])
@pytest.mark.parametrize("width", [1, 4, 16, 64])
def test_pattern_does_not_depend_on_the_launch_geometry(psk, name, k, width, monkeypatch):
    """1, 4, 16 or 64 lanes per row in every symbolic kernel (the library picks by the mean row length; 64 is the
    widest group and never hands a row on): the same pattern, levels and factor bits."""
    monkeypatch.setenv("PSK_ILUK_WIDTH", str(width))
    dA = psk.DeviceCSR.from_scipy(_matrix(name))
    P, Lev = dA.iluk_pattern(k, levels=True)
    _same_csr(P.to_scipy(), _oracle_pattern(name, k)[0])
    _same_csr(Lev.to_scipy(), _oracle_pattern(name, k)[1])
    _same_csr(psk.RightILUK(k).form(dA).factors(), _oracle_factor(name, k))


# ---- 3. the apply --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k", APPLY_CASES)
def test_apply_vs_oracle(psk, name, k):
    v = np.array(_rhs(name))
    ref = io0.apply(_oracle_factor(name, k))(v)
    M = psk.RightILUK(k).form(_matrix(name))
    y = M.applyRight(v)
    dev = np.max(np.abs(y - ref)) / np.max(np.abs(ref))
    print("%s k=%d: schedules L=%s U=%s, apply deviation %.3e max|oracle apply|"
          % (name, k, M.schedule("L")["schedule"], M.schedule("U")["schedule"], dev))
    assert np.all(np.isfinite(y)) and dev <= RTOL_APPLY, (name, k, dev)
    assert np.array_equal(_bits(M.applyRight(v)), _bits(y))                                     # run to run
    yd = M.applyRight(psk.DeviceVector.from_numpy(v)).numpy()
    assert np.array_equal(_bits(yd), _bits(y))
    left = psk.LeftILUK(k).form(_matrix(name))
    assert left.applyRight(v) is v and np.array_equal(_bits(left.applyLeft(v)), _bits(y))


@pytest.mark.parametrize("name", ["negfd33", "cd32", "rand700"])
def test_swept_apply_vs_oracle(psk, name):
    """RightILUK(1, sweeps=4) against the sweep oracle on the oracle factor."""
    v = np.array(_rhs(name))
    M = psk.RightILUK(1, sweeps=4).form(_matrix(name))
    assert (M.sweeps("L"), M.sweeps("U")) == (4, 4)
    ref = tso.ilu0_chain(_oracle_factor(name, 1), 4, 4)(v)
    y = M.applyRight(v)
    dev = np.max(np.abs(y - ref)) / np.max(np.abs(ref))
    print("%s: ILU(1) with 4 sweeps, deviation %.3e max|oracle|" % (name, dev))
    assert np.all(np.isfinite(y)) and dev <= RTOL_APPLY, (name, dev)
    mixed = psk.RightILUK(1, sweeps=(0, 2)).form(_matrix(name))
    assert (mixed.sweeps("L"), mixed.sweeps("U")) == (0, 2)


def test_gmres_converges_with_swept_ilu1_on_cd32(psk):
    A, b = _matrix("cd32"), np.array(_rhs("cd32"))
    st = psk.GMRES(control=_ctl(psk), precond=psk.RightILUK(1, sweeps=4)).makeSolver().solve(A, b)
    print("cd32: GMRES + ILU(1) with 4 sweeps: %d iterations" % st.iters())
    assert st.success(), st.msg()
    assert np.linalg.norm(b - A @ st.soln()) <= TAU * np.linalg.norm(b)


# ---- 4. the solvers ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(method, name, k):
    A, b = _matrix(name), _rhs(name)
    M = io0.apply(_oracle_factor(name, k))
    if method == "gmres":
        r = krylov.gmres(A, b, maxiter=MAXITER, tau=TAU, precond=M)
    elif method == "pcg":
        r = krylov.pcg(A, b, maxiter=MAXITER, tau=TAU, precond=M)
    elif method == "bicgstab":
        r = bo.bicgstab(A, b, M=M, maxiter=MAXITER, tau=TAU)
    else:
        r = io_.idrs(A, b, s=4, M=M, maxiter=MAXITER, tau=TAU)
    r["hist"].setflags(write=False)
    return r


def _device_solve(psk, method, name, prec):
    make = {"gmres": psk.GMRES, "pcg": psk.PCG, "bicgstab": psk.BiCGStab}.get(method)
    solver = (psk.IDRs(control=_ctl(psk), precond=prec, s=4) if make is None
              else make(control=_ctl(psk), precond=prec)).makeSolver()
    return solver.solve(_matrix(name), np.array(_rhs(name)))


@functools.lru_cache(maxsize=None)
def _ilu0_iters(method, name):
    import pysolvers_amd
    st = _device_solve(pysolvers_amd, method, name, pysolvers_amd.RightILU0())
    assert st.iters() > 1
    return st.iters()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("method,name", [("gmres", "cd64"), ("bicgstab", "cd64"), ("idrs4", "cd64"), ("pcg", "negfd33")])
def test_solvers_match_the_oracle_and_beat_ilu0(psk, method, name, k):
    """cd64: the convection-diffusion operator cd 64 with c = 0.2. PCG may use the factor of the symmetric negfd33:
    its L U is symmetric."""
    ref = _reference(method, name, k)
    st = _device_solve(psk, method, name, psk.RightILUK(k))
    nb = np.linalg.norm(_rhs(name))
    h, ho = st.info["hist"], ref["hist"]
    m = min(len(h), len(ho))
    dev = np.max(np.abs(h[:m] - ho[:m])) / nb
    base = _ilu0_iters(method, name)
    print("%s %s ILU(%d): iters %d (oracle %d, ILU(0) %d), history deviation %.3e ||b||"
          % (method, name, k, st.iters(), ref["iters"], base, dev))
    assert st.iters() == ref["iters"] and len(h) == len(ho), (st.iters(), ref["iters"])
    assert dev <= RTOL_RESID, (method, name, k, dev)
    assert bool(st.success()) == bool(ref["success"]), st.msg()
    if method in ("gmres", "pcg"):
        assert st.success(), st.msg()
    assert st.iters() < base


# ---- 5. errors -----------------------------------------------------------------------------------------------------

def _csr(data, indices, indptr, shape):
    A = sp.csr_matrix((np.array(data, dtype=np.float64), np.array(indices, dtype=np.int32),
                       np.array(indptr, dtype=np.int32)), shape=shape)
    A.has_sorted_indices = False
    return A


BAD = {
    # name: (matrix, k, code, text in the message)
    "longrow": (lambda: mcgs_cases.matrix("longrow"), 1, -5, "row 7 "),
    "no_diagonal": (lambda: _csr([2.0, 1.0, 1.0], [0, 1, 0], [0, 2, 3], (2, 2)), 1, -1, "diagonal"),
    "duplicate": (lambda: _csr([2.0, 1.0, 1.0, 3.0], [0, 0, 0, 1], [0, 2, 4], (2, 2)), 1, -5, "duplicate"),
    "rectangular": (lambda: _csr([2.0, 1.0, 1.0, 3.0], [0, 2, 0, 1], [0, 2, 4], (2, 3)), 1, -1, "square"),
}


@pytest.mark.parametrize("kind", list(BAD))
def test_errors_are_returned_write_nothing_and_leave_no_state(psk, kind):
    from pysolvers_amd import _native as N
    assert (N.PSK_ERR_ARG, N.PSK_ERR_UNSUPPORTED) == (-1, -5)
    make, k, code, text = BAD[kind]
    dA = psk.DeviceCSR.from_scipy(make(), rectangular=True)
    with pytest.raises(N.PskError) as e:
        dA.iluk_pattern(k)
    assert e.value.code == code and text in str(e.value) + " ", str(e.value)
    with pytest.raises(N.PskError) as e:
        psk.RightILUK(k).form(dA)
    assert e.value.code == code and text in str(e.value) + " ", str(e.value)
    hp, hl, hm = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert N.lib.psk_csr_iluk_pattern(dA.handle, k, ctypes.byref(hp), ctypes.byref(hl)) == code
    assert N.lib.psk_prec_create_iluk(dA.handle, k, ctypes.byref(hm)) == code
    assert hp.value is None and hl.value is None and hm.value is None      # no output written
    # a valid form right after the error: nothing sticky is left behind
    _same_csr(psk.RightILUK(1).form(_matrix("negfd16")).factors(), _oracle_factor("negfd16", 1))


def test_longrow_names_the_smallest_row_over_the_cap(psk):
    """Row 7 of `longrow` stores 1500 entries, over PSK_ILUK_ROW_CAP = 512; no other row comes near. k = 0 runs no
    round, so the cap does not apply: the sorted copy, and RightILU0's bits."""
    from pysolvers_amd import _native as N
    A = mcgs_cases.matrix("longrow")
    assert np.diff(A.indptr)[7] == 1500
    dA = psk.DeviceCSR.from_scipy(A)
    _same_csr(dA.iluk_pattern(0).to_scipy(), io0.sorted_copy(A))
    _same_csr(psk.RightILUK(0).form(dA).factors(), psk.RightILU0().form(dA).factors())
    for k in (1, 3):
        with pytest.raises(N.PskError) as e:
            dA.iluk_pattern(k)
        assert e.value.code == N.PSK_ERR_UNSUPPORTED and "row 7 " in str(e.value) and "512" in str(e.value)


def test_a_level_out_of_range(psk):
    from pysolvers_amd import _native as N
    dA = psk.DeviceCSR.from_scipy(_matrix("negfd16"))
    for k in (9, -1):
        with pytest.raises(ValueError):
            dA.iluk_pattern(k)
        with pytest.raises(ValueError):
            psk.RightILUK(k)
        hp, hm = ctypes.c_void_p(), ctypes.c_void_p()
        assert N.lib.psk_csr_iluk_pattern(dA.handle, k, ctypes.byref(hp), None) == N.PSK_ERR_ARG
        assert b"level" in N.lib.psk_last_error()
        assert N.lib.psk_prec_create_iluk(dA.handle, k, ctypes.byref(hm)) == N.PSK_ERR_ARG
        assert hp.value is None and hm.value is None


def test_a_sharded_matrix_is_refused(psk):
    from pysolvers_amd import _native as N
    one = psk.Linear.Communicator(1, 0, dry=True)
    try:
        dS = psk.Linear.fd_laplacian_2d_sharded(-1.0, 1.0, 17, one)
        with pytest.raises(ValueError, match="sharded"):
            dS.iluk_pattern(1)
        with pytest.raises(ValueError, match="sharded"):
            psk.RightILUK(1).form(dS)
        hp, hm = ctypes.c_void_p(), ctypes.c_void_p()
        assert N.lib.psk_csr_iluk_pattern(dS.handle, 1, ctypes.byref(hp), None) == N.PSK_ERR_UNSUPPORTED
        assert b"sharded" in N.lib.psk_last_error()
        assert N.lib.psk_prec_create_iluk(dS.handle, 1, ctypes.byref(hm)) == N.PSK_ERR_UNSUPPORTED
        assert hp.value is None and hm.value is None
        del dS
    finally:
        one.destroy()


def test_a_zero_pivot_made_by_the_fill_reports_as_ilu0_does(psk):
    """ILU(0) of this matrix has the pivots 1, 1, 1. Level 1 adds (1,2) and (2,1), both -1 after row 0 is eliminated,
    and their product cancels row 2's pivot: the error of psk_csr_ilu0 on the padded matrix, in its words."""
    from pysolvers_amd import _native as N
    A = _csr([1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 2.0], [0, 1, 2, 0, 1, 0, 2], [0, 3, 5, 7], (3, 3))
    assert np.array_equal(io0.ilu0(A).diagonal(), [1.0, 1.0, 1.0])
    with pytest.raises(io0.PivotError) as oe:
        ko.iluk(A, 1)
    assert oe.value.row == 2
    dA = psk.DeviceCSR.from_scipy(A)
    _same_csr(psk.RightILUK(0).form(dA).factors(), io0.ilu0(A))
    P = dA.iluk_pattern(1)
    _same_csr(P.to_scipy(), ko.pattern(A, 1)[0])
    with pytest.raises(N.PskError) as e0:
        P.ilu0()
    with pytest.raises(N.PskError) as ek:
        psk.RightILUK(1).form(dA)
    assert ek.value.code == e0.value.code == N.PSK_ERR_ARG
    assert "pivot in row 2" in str(ek.value) and "psk_csr_ilu0" in str(ek.value)
    assert str(ek.value).split(":", 1)[1] == str(e0.value).split(":", 1)[1]


# ---- 6. Newton -----------------------------------------------------------------------------------------------------

def test_newton_bratu_with_gmres_ilu1_steps(psk):
    """FD-Bratu 32^2 (the case of test_gpu_ilu0.py's Newton test) with GMRES + RightILUK(1) steps and the
    preconditioner frozen: Newton succeeds in the iteration count it takes with RightILU0 and meets its own stopping
    rule ||F|| <= tau ||F_0|| + tau."""
    from pysolvers_amd.Nonlinear import NewtonSolver
    from oracle import newton
    func = newton.Bratu2D(m=32)
    tau = 1.0e-12
    out = {}
    for tag, prec in (("ilu0", psk.RightILU0()), ("ilu1", psk.RightILUK(1))):
        lin = psk.GMRES(control=psk.CommonSolverArgs(showIters=False, showFinal=False), precond=prec)
        ns = NewtonSolver(control=psk.CommonSolverArgs(tau=tau, maxiter=10, showIters=False, showFinal=False),
                          solver=lin, fixLinTol=False, minLinTol=1.0e-6, freezePrec=True)
        st = ns.solve(func, func.initialU())
        assert st.success(), st.msg()
        normF0 = np.linalg.norm(func.evalF(func.initialU()))
        assert np.linalg.norm(func.evalF(st.soln())) <= tau * normF0 + tau
        assert len(ns.linear_iters) == st.iters() - 1 and all(q >= 1 for q in ns.linear_iters)
        out[tag] = (st.iters(), list(ns.linear_iters))
    print("Newton Bratu 32^2: ILU(0) %s, ILU(1) %s" % (out["ilu0"], out["ilu1"]))
    assert out["ilu1"][0] == out["ilu0"][0]
