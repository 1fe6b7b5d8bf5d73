"""bench.py as a command: a plain run times exactly --steps iterations, reports ms_per_step, measures nothing
beside the headline, and --dump-outputs writes what the timed solve returned (checked against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

SIDE, STEPS, WARMUP = 96, 7, 3
FULL_ONLY = ("regions_without_kernel_events", "spmv_plain_batch50", "fixed_overhead", "general_path",
             "spmv_csr_layout_batch50", "csr_layout_in_loop", "strong_scaling_16384", "configs1_pcg_jacobi_4096",
             "gmres30_jacobi_4096", "configs2_gmres30_ilut", "configs4_pcg_amg_8192")


def _bench(outdir):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--side", str(SIDE), "--dump-outputs", str(outdir)]
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_line_and_dump(tmp_path):
    from oracle import fdlap, krylov
    out = _bench(tmp_path / "a")
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["full"] is False
    assert out["unit"] == "CG iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["repeats"]["regions"] == 1
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-12)
    assert not [k for k in FULL_ONLY if k in out] and out["cpu_baseline"] is None
    n = SIDE * SIDE
    x = np.load(tmp_path / "a" / "x.npy")
    res = np.load(tmp_path / "a" / "result.npy")
    assert x.dtype == np.float64 and x.shape == (n,) and res.dtype == np.float64
    assert not (tmp_path / "a" / "x_index.npy").exists()      # the whole vector fits: no sample
    A = fdlap.fd_laplacian_2d(-1.0, 1.0, SIDE)
    b = A @ np.random.default_rng(12345).random(n)
    ref = krylov.pcg(A, b, maxiter=STEPS, tau=0.0, fail_on_maxiter=False, precond=krylov.jacobi_form(A))
    assert int(res[0]) == STEPS == ref["iters"]
    # the solvers' parity bar (DESIGN.md "Parity"): solution within 1e-9 relative of the oracle's
    assert np.linalg.norm(x - ref["soln"]) <= 1e-9 * np.linalg.norm(ref["soln"])
    assert res[3] == np.linalg.norm(b) or abs(res[3] - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
    # the same arguments give the same inputs and the same outputs, bit for bit
    _bench(tmp_path / "b")
    assert np.array_equal(np.load(tmp_path / "b" / "x.npy"), x)
    assert np.array_equal(np.load(tmp_path / "b" / "result.npy"), res)
