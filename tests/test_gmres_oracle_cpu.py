"""tests/gmres_oracle.py pinned to oracle/krylov.py (no GPU): with np.dot as its dot product the restated cycle is
krylov.gmres / krylov.gmres_cycle bit for bit, and its measures say what they should on arrays built by hand."""
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

import bicgstab_oracle as bo
import gmres_oracle as go
from conftest import GOLDEN
from oracle import krylov

TAU = 1e-10


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _case(name):
    if name == "dh8":
        A = scipy.io.mmread(os.path.join(GOLDEN, "mtx", "DH-Matrix-8.mtx")).tocsr()
    else:
        A = bo.cd_matrix(17, 0.3)
    return A, np.random.default_rng(len(name)).standard_normal(A.shape[0])


@pytest.mark.parametrize("name", ["dh8", "cd17"])
@pytest.mark.parametrize("prec", ["identity", "jacobi"])
def test_cycle_is_krylov_gmres_bit_for_bit(name, prec):
    A, b = _case(name)
    M = krylov.jacobi_form(A) if prec == "jacobi" else krylov.identity_apply
    ref = krylov.gmres(A, b, maxiter=200, tau=TAU, precond=M, return_internals=True)
    c = go.cycle(A, b, 200, TAU * np.linalg.norm(b), M, dot=bo.dot_numpy)
    k = c["k"]
    assert ref["success"] and c["conv"] and not c["brk"] and ref["iters"] == k + 1 and k >= 5
    assert np.array_equal(_bits(c["hist"]), _bits(ref["hist"]))
    assert np.array_equal(_bits(c["R"][:k + 2, :k + 1]), _bits(ref["HBar"]))
    assert np.array_equal(_bits(c["g"][:k + 2]), _bits(ref["g"]))
    assert np.array_equal(_bits(c["y"]), _bits(ref["y"]))
    assert np.array_equal(_bits(c["dx"]), _bits(ref["soln"]))
    # and krylov.gmres_cycle itself
    k2, conv2, hist2, dx2 = krylov.gmres_cycle(A, b, 200, TAU * np.linalg.norm(b), M)
    assert (k2, conv2) == (k, True)
    assert np.array_equal(_bits(hist2), _bits(c["hist"])) and np.array_equal(_bits(dx2), _bits(c["dx"]))
    # the unrotated columns give the rotated ones back
    R, CS, g, hist = go.givens_replay(c["H"], float(np.linalg.norm(b)), k + 1)
    assert np.array_equal(_bits(R), _bits(c["R"])) and np.array_equal(_bits(CS), _bits(c["CS"]))
    assert np.array_equal(_bits(g), _bits(c["g"])) and np.array_equal(_bits(hist), _bits(c["hist"]))


@pytest.mark.parametrize("name", ["dh8", "cd17"])
def test_restarted_solve_is_krylov_gmres_restarted_bit_for_bit(name):
    A, b = _case(name)
    M = krylov.jacobi_form(A)
    ref = krylov.gmres_restarted(A, b, 5, maxiter=200, tau=TAU, precond=M)
    s = go.solve(A, b, restart=5, maxiter=200, tau=TAU, precond=M)
    assert len(s["cycles"]) >= 3 and s["iters"] == ref["iters"] and s["conv"] == ref["success"]
    assert np.array_equal(_bits(s["hist"]), _bits(ref["hist"])) and np.array_equal(_bits(s["x"]), _bits(ref["soln"]))


@pytest.mark.parametrize("name", ["dh8", "cd17"])
def test_measures_on_the_oracle_and_on_damaged_copies(name):
    """The oracle's own arrays sit at rounding level under every dot order; one element dropped from one dot, a
    stale h and a wrong divisor each move the measure that is meant to see them by orders of magnitude."""
    A, b = _case(name)
    M = krylov.jacobi_form(A)
    n = A.shape[0]
    for dot in bo.DOTS:
        c = go.cycle(A, b, 200, TAU * np.linalg.norm(b), M, dot=dot)
        m = c["k"] + 1
        assert np.max(go.arnoldi_residuals(A, M, c["Q"], c["H"], m)) < 50 * go.EPS
        assert go.orthogonality(c["Q"], 10) < 1e-12         # (eps kappa later on: 7e-6 over DH-8's 56 columns)
        wh, wn = go.mgs_dot_errors(A, M, c["Q"], c["H"], m)
        assert wh <= 1 and wn <= 1
        assert go.triangular_error(c["R"], c["y"], c["g"], m) <= 1
        dinv = np.reciprocal(A.diagonal())
        assert go.update_x_error(c["Q"], c["y"], c["dx"], m, dinv) <= 1

    def drop_last(u, v):                       # a dot that forgets the tail element
        return bo.dot_numpy(u[:-1], v[:-1])
    d = go.cycle(A, b, 40, 0.0, M, dot=drop_last)
    md = d["k"] + 1
    assert go.orthogonality(d["Q"], 10) > 1e4 * go.orthogonality(c["Q"], 10)
    assert max(go.mgs_dot_errors(A, M, d["Q"], d["H"], md)) > 1
    H = c["H"].copy()
    H[1, 3] = H[1, 2]                          # a stale h written to the column
    assert np.max(go.arnoldi_residuals(A, M, c["Q"], H, m)) > 1e-6
    Q = c["Q"].copy()
    Q[n - 1, 4] *= 1.0 + 1e-9                  # a tail element normalised by another divisor
    assert np.max(go.arnoldi_residuals(A, M, Q, c["H"], m)) > 1e3 * np.max(go.arnoldi_residuals(A, M, c["Q"], c["H"], m))
    x = c["dx"].copy()
    x[n // 2] *= 1.0 + 1e-12
    assert go.update_x_error(c["Q"], c["y"], x, m, dinv) > 1


def test_exact_breakdown_cases_on_the_oracle():
    """The cases tests/test_gpu_gmres_arnoldi.py holds the device to bit for bit: every intermediate is 0, +-1 or a
    power of two and every sum has one nonzero term."""
    n, idx = 1025, [0, 511, 512, 1024]
    d = np.full(n, 2.0)
    d[idx] = 0.0
    A = (sp.diags(d) + sp.coo_matrix((np.ones(4), ([idx[(i + 1) % 4] for i in range(4)], idx)), shape=(n, n))).tocsr()
    A.eliminate_zeros()
    b = np.zeros(n)
    b[0] = 4.0
    ref = krylov.gmres(A, b, maxiter=50, tau=1e-12)
    assert ref["success"] and ref["iters"] == 4 and ref["resid"] == 0.0
    assert np.array_equal(ref["hist"], [4.0, 4.0, 4.0, 0.0])
    want = np.zeros(n)
    want[1024] = 4.0
    assert np.array_equal(_bits(ref["soln"]), _bits(want))
    c = go.cycle(A, b, 50, 1e-12 * 4.0)
    assert c["brk"] and c["k"] == 3 and not c["Q"][:, 4:].any()
    # GMRES(2) cannot leave b on a cyclic shift of order 4: it stagnates to maxiter, every entry exactly 4
    r2 = krylov.gmres_restarted(A, b, 2, maxiter=50, tau=1e-12)
    assert not r2["success"] and r2["iters"] == 49 and np.array_equal(r2["hist"], np.full(50, 4.0))
    assert not r2["soln"].any()
    A = sp.diags(2.0 ** np.arange(-3, 4)).tocsr()
    b = np.zeros(7)
    b[5] = 3.0
    ref = krylov.gmres(A, b, maxiter=50, tau=1e-12, precond=krylov.jacobi_form(A))
    assert ref["iters"] == 1 and np.array_equal(ref["hist"], [0.0]) and ref["soln"][5] == 0.75
    assert np.count_nonzero(ref["soln"]) == 1
