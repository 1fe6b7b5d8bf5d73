#!/usr/bin/env python3
"""AMG setup on the host against setup on the device, same box, same process (DESIGN.md "Device-side AMG setup").

    python tools/amg_setup_ab.py --sides 2048,8192 --levels 5 --rounds 2 --commit $(git rev-parse --short HEAD) \
        [--out profiles/amg_device_setup_ab.txt]

For every side m, -FDLaplacian2D(m) is built once and kept in HBM; then `rounds` alternating rounds of
AMGPreconditioner(dA, numLevels=levels, setup="host") and (..., setup="device") — what AMG(...).form(A) runs — each
timed on the host clock to a device synchronise, with the phases the classes record themselves:
  fine        the caller's matrix: its host copy (both paths run psk_sa_aggregate and the smoother planner on it)
  aggregate   psk_sa_aggregate, every level (host code in both paths)
  prolong     the smoothing arithmetic and S Phat                     host: numpy + scipy, device: psk_sa_prolongator
  transpose   R = P^T                                                  host: scipy,         device: psk_csr_transpose
  galerkin    A P and R (A P)                                          host: scipy,         device: psk_csr_matmat x 2
  transfer    device: the downloads of the coarse operators (for the aggregation, the smoothers, the coarse solve)
  upload      host: the upload of every operator
  smoothers   the smoother setup of every level (the triangular-solve planner for Gauss-Seidel)
  coarse      the coarse solve (dense inverse or LU)
"operators" = prolong + transpose + galerkin + transfer + upload: what the device path replaces and what it adds.
The two preconditioners' apply of one random vector is compared bit for bit in every round.
"""
import argparse
import hashlib
import os
import socket
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PHASES = ("fine", "aggregate", "prolong", "transpose", "galerkin", "transfer", "upload", "smoothers", "coarse")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="2048,8192")
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pysolvers_amd as psk
    from pysolvers_amd import _native as N
    from pysolvers_amd.Linear import AMGPreconditioner
    assert N.device_count() >= 1, "no GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:
        dev = "gpu"
    with open(N.LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    say("AMG setup, host against device: same-box alternating rounds in one process, tools/amg_setup_ab.py --sides %s "
        "--levels %d --rounds %d" % (args.sides, args.levels, args.rounds))
    say("box: %s, %s; commit: %s; libpsk.so sha256: %s" % (socket.gethostname(), dev, args.commit, sha))
    say("variants: host   = AMGPreconditioner(dA, numLevels=%d, setup=\"host\"): scipy/numpy operators, uploaded"
        % args.levels)
    say("          device = the same with setup=\"device\": psk_sa_prolongator, psk_csr_transpose, psk_csr_matmat")
    say("columns: round variant side: form seconds | the phases in seconds | operators = prolong + transpose + galerkin"
        " + transfer + upload | products on the device / on the host | sha256 of one apply's bits")
    for m in [int(v) for v in args.sides.split(",")]:
        A = -psk.DeviceCSR.fd_laplacian_2d(-1.0, 1.0, m).to_scipy()
        dA = psk.DeviceCSR.from_scipy(A)
        n = A.shape[0]
        del A
        v = psk.DeviceVector.from_numpy(np.random.default_rng(m).standard_normal(n))
        first = True
        for r in range(args.rounds):
            bits = {}
            for setup in ("host", "device"):
                N.check(N.lib.psk_synchronize(), "sync")
                t0 = time.perf_counter()
                M = AMGPreconditioner(dA, numIters=2, numLevels=args.levels, setup=setup)
                N.check(N.lib.psk_synchronize(), "sync")
                total = time.perf_counter() - t0
                st, sec = M.mlh.setup_stats, dict(M.mlh.setup_stats["seconds"])
                ph = dict(fine=M.setup_seconds["fine"], aggregate=sec["aggregate"], prolong=sec["prolongator"],
                          transpose=sec["transpose"], galerkin=sec["galerkin"], transfer=sec["transfer"],
                          upload=M.setup_seconds["upload"], smoothers=M.setup_seconds["smoothers"],
                          coarse=M.setup_seconds["coarse"])
                ops = ph["prolong"] + ph["transpose"] + ph["galerkin"] + ph["transfer"] + ph["upload"]
                if first:
                    say("== side %d: n = %d, levels %s, coarse %s" % (m, n, M.levels(), M.coarse_kind))
                    first = False
                bits[setup] = hashlib.sha256(M.apply(v).numpy().tobytes()).hexdigest()[:12]
                say("%d %-6s %5d: form %8.3f s | %s | operators %8.3f | products %d/%d | apply %s"
                    % (r, setup, m, total, "  ".join("%s %.3f" % (k, ph[k]) for k in PHASES), ops,
                       st["device_products"], st["host_products"], bits[setup]))
                del M
            assert bits["host"] == bits["device"], "the two setups' applies differ"
        del dA, v
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
