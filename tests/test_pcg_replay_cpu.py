"""tests/pcg_replay.py pinned on the CPU: the replay fed with the oracle's own scalars reproduces the oracle bit for
bit, and the oracle's own np.dot values stay inside dot_bound of the exact sums on every case the GPU file runs (the
reference alone stays inside the bar the device is held to)."""
import fractions
import functools
import math

import numpy as np
import numpy.linalg as npla
import pytest

import cheby_oracle
import ilu0_oracle
import pcg_replay as pr
from conftest import golden_matrix, load_golden
from oracle import krylov


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def pcg_trace(A, b, maxiter, tau, precond, fail_on_maxiter=True):
    """oracle.krylov.pcg line for line, keeping what it throws away: alphas, udr (udr[k] = u_k.r_k), pTAp, hist, x, and
    the operands of every np.dot with its value."""
    dots = []

    def dot(tag, a, c):
        v = np.dot(a, c)
        dots.append((tag, np.copy(a), np.copy(c), v))
        return v
    normB = npla.norm(b)
    r = np.copy(b)
    p = precond(r)
    u = np.copy(p)
    x = np.zeros_like(b)
    uDotR = dot("u.r 0", u, r)
    t = dict(alphas=[], udr=[uDotR], pTAp=[], hist=[], dots=dots, x=x, normB=normB)
    for k in range(maxiter):
        Ap = krylov.mvmult(A, p)
        pTAp = dot("p.Ap %d" % k, p, Ap)
        if pTAp == 0.0:
            break
        alpha = uDotR / pTAp
        x = x + alpha * p
        r = r - alpha * Ap
        u = precond(r)
        normR = npla.norm(r)
        t["alphas"].append(alpha)
        t["pTAp"].append(pTAp)
        t["hist"].append(normR)
        t["x"] = x
        if (normR <= tau * normB) or ((not fail_on_maxiter) and k == maxiter - 1):
            break
        newUDotR = dot("u.r %d" % (k + 1), u, r)
        beta = newUDotR / uDotR
        uDotR = newUDotR
        t["udr"].append(uDotR)
        p = u + beta * p
    return t


@pytest.mark.parametrize("golden, jacobi", [("pcg_fd16_jacobi.npz", True), ("pcg_dh8_identity.npz", False)])
def test_replay_reproduces_the_oracle_bitwise(golden, jacobi):
    d = load_golden(golden)
    A, b = golden_matrix(d), d["b"]
    maxiter, tau = int(d["maxiter"]), float(d["tau"])
    M = krylov.jacobi_form(A) if jacobi else krylov.identity_apply
    ref = krylov.pcg(A, b, maxiter=maxiter, tau=tau, precond=M)
    t = pcg_trace(A, b, maxiter, tau, M)
    # the restatement is the oracle
    assert np.array_equal(_bits(t["hist"]), _bits(ref["hist"])) and np.array_equal(_bits(t["x"]), _bits(ref["soln"]))
    K = len(t["hist"])
    assert K >= 10 and len(t["udr"]) == K and len(t["alphas"]) == K
    rp = pr.replay(A, b, np.reciprocal(A.diagonal()) if jacobi else None, t["alphas"], t["udr"], K)
    assert np.array_equal(_bits(rp["x"][K]), _bits(ref["soln"]))
    assert np.array_equal(_bits([npla.norm(r) for r in rp["r"][1:]]), _bits(ref["hist"]))
    assert len(rp["p"]) == K and len(rp["Ap"]) == K and len(rp["r"]) == K + 1
    # and a callable apply is the array's
    rc = pr.replay(A, b, M, t["alphas"], t["udr"], K)
    assert all(np.array_equal(_bits(a), _bits(c)) for key in rp for a, c in zip(rp[key], rc[key]))


def test_exact_sums_against_rational_arithmetic():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 257):
        a = rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)
        c = rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)
        hi, lo = pr.two_product(a, c)
        F = fractions.Fraction
        assert all(F(float(h)) + F(float(l)) == F(float(x)) * F(float(y)) for h, l, x, y in zip(hi, lo, a, c))
        assert pr.exact_dot_fma(a, c) == float(sum(F(float(x)) * F(float(y)) for x, y in zip(a, c)))
        assert pr.exact_dot(a, c) == float(sum(F(float(x * y)) for x, y in zip(a, c)))
        assert pr.dot_bound(a, c) == (n - 1) * 2.0 ** -53 * math.fsum(np.abs(a * c))
    assert pr.dot_bound([3.0], [4.0]) == 0.0 and pr.exact_dot([3.0], [4.0]) == 12.0


def test_random_spd_has_the_shape_the_cases_need():
    for n in (2, 513):
        A = pr.random_spd(n, seed=n)
        assert np.array_equal(_bits(pr.random_spd(n, seed=n).data), _bits(A.data))      # a function of (n, seed)
        ip, ind = A.indptr, A.indices
        unsorted = any(np.any(np.diff(ind[ip[i]:ip[i + 1]]) < 0) for i in range(n))
        d = A.diagonal()
        off = np.asarray(abs(A.copy()).sum(axis=1)).ravel() - np.abs(d)                 # (abs sorts its operand in place)
        assert (abs(A - A.T)).nnz == 0 and np.all(d > off) and np.ptp(d) > 0
    assert unsorted and 4 <= A.nnz / 513 <= 6


@functools.lru_cache(maxsize=None)
def _ring():
    """(S, ring depth) of the build (psk_lab_pcg_stagger touches no GPU)."""
    import ctypes
    from pysolvers_amd import _native as N
    s, ring = N.I32(), N.I32()
    N.check(N.load_lab().psk_lab_pcg_stagger(ctypes.byref(s), ctypes.byref(ring)), "psk_lab_pcg_stagger")
    return s.value, ring.value


def host_apply(A, prec):
    return {"identity": lambda: krylov.identity_apply, "jacobi": lambda: krylov.jacobi_form(A),
            "cheb3": lambda: cheby_oracle.Chebyshev(A, degree=3),
            "ilu0": lambda: ilu0_oracle.apply(ilu0_oracle.ilu0(A))}[prec]()


@pytest.mark.parametrize("name, prec", pr.ELEMENTWISE + pr.GENERAL)
def test_the_oracles_own_dots_stay_inside_the_bound(name, prec):
    A, b = pr.matrix(name), pr.rhs(name)
    K = max(pr.depths(A.shape[0], *_ring()))
    t = pcg_trace(A, b, K, 0.0, host_apply(A, prec), fail_on_maxiter=False)
    worst = 0.0
    for tag, a, c, v in t["dots"]:
        ok, ratio = pr.check_sum(v, pr.exact_dot(a, c), a, c)
        assert ok, (name, prec, tag, v, ratio)
        worst = max(worst, ratio)
    print("%s %s: %d dots over %d iterations, worst |np.dot - exact| / bound %.3e" % (name, prec, len(t["dots"]),
                                                                                     len(t["hist"]), worst))
    assert len(t["dots"]) >= 2
