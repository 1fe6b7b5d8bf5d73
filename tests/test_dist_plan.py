"""Host-only checks of the general shard planner (dist_plan and dist_peers through psk_lab_dist_plan; no GPU)
against the CPU oracle's plan (oracle.dist_pcg.shard_plan), rank by rank and exactly: the local columns, the
halo, the peer list, what is sent to and received from every peer, and which peers gather their rows through the
pack list. The shards on the device are checked in tests/test_gpu_shards.py."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from pysolvers_amd import _native as N
from pysolvers_amd.Linear.Distributed import even_row_starts
from oracle import dist_pcg, fdlap

PEER = ("rank", "send_count", "send_begin", "packed", "pack_off", "recv_count", "recv_offset")


def _tridiag(n):
    return sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()


def _matrix(name):
    from conftest import golden_matrix, load_golden
    if name == "fd6_permuted":   # rows and columns renumbered alike (still symmetric): a peer's rows lie anywhere
        A = fdlap.fd_laplacian_2d(-1.0, 1.0, 6).tocsr()
        perm = np.random.default_rng(0).permutation(36)
        return A[perm][:, perm].tocsr()
    if name.startswith("fd"):
        return fdlap.fd_laplacian_2d(-1.0, 1.0, int(name[2:]))
    if name.startswith("tri"):
        return _tridiag(int(name[3:]))
    return golden_matrix(load_golden("pcg_%s_identity.npz" % name))


# case -> (matrix, ranks, row_starts; None: even_row_starts by stored entries, as tests/test_gpu_shards.py)
CASES = {
    "dh8-P2": ("dh8", 2, None), "dh12-P3": ("dh12", 3, None), "dh12-P5": ("dh12", 5, None),
    "fd50-P4": ("fd50", 4, None),
    "fd8-P1": ("fd8", 1, None),                      # no peers, empty halo
    "tri3-P3": ("tri3", 3, [0, 1, 2, 3]),            # one row per rank; the middle rank has two contiguous peers
    "tri6-empty-rank": ("tri6", 3, [0, 3, 3, 6]),    # rank 1 owns nothing; ranks 0 and 2 exchange past it
    "fd6-permuted-P2": ("fd6_permuted", 2, [0, 18, 36]),   # non-contiguous send rows: the pack path
}


def lab_plan(n_global, rs, P, r, rowptr, colidx):
    """psk_lab_dist_plan of one rank: (rc, dict of outputs)."""
    rs = np.ascontiguousarray(rs, dtype=np.int64)
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    nnz = int(rowptr[-1] - rowptr[0])
    cap = max(nnz, 1)
    lcol, pack = np.full(cap, -1, np.int32), np.full(cap, -1, np.int32)
    halo, peers = np.full(cap, -1, np.int64), np.full(7 * P, -1, np.int64)
    nhalo, npack, npeers = N.I64(-1), N.I64(-1), N.I32(-1)
    rc = N.load_lab().psk_lab_dist_plan(n_global, N.ptr(rs), P, r, N.ptr(rowptr), N.ptr(colidx), N.ptr(lcol),
                                        N.ptr(halo), ctypes.byref(nhalo), N.ptr(pack), ctypes.byref(npack),
                                        N.ptr(peers), ctypes.byref(npeers))
    if rc != N.PSK_OK:
        return rc, None
    k = npeers.value
    return rc, dict(lcol=lcol[:nnz], halo=halo[:nhalo.value], pack=pack[:npack.value],
                    peers=[dict(zip(PEER, (int(v) for v in peers[7 * j:7 * j + 7]))) for j in range(k)])


@functools.lru_cache(maxsize=None)
def _planned(case):
    name, P, rs = CASES[case]
    A = _matrix(name).tocsr()
    n = A.shape[0]
    rs = even_row_starts(n, P, A.indptr) if rs is None else np.array(rs, dtype=np.int64)
    out = []
    for r in range(P):
        rb, re = int(rs[r]), int(rs[r + 1])
        e0, e1 = int(A.indptr[rb]), int(A.indptr[re])
        rc, got = lab_plan(n, rs, P, r, A.indptr[rb:re + 1], A.indices[e0:e1])
        assert rc == N.PSK_OK, (case, r, rc)
        out.append((got, dist_pcg.shard_plan(A, rs, r)))
    return tuple(out)


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_matches_oracle(case):
    for r, (got, pl) in enumerate(_planned(case)):
        assert np.array_equal(got["lcol"], pl["Aloc"].indices), (case, r)
        assert np.array_equal(got["halo"], pl["halo"]), (case, r)
        want_peers = sorted(set(pl["send"]) | set(pl["recv"]))
        assert [p["rank"] for p in got["peers"]] == want_peers, (case, r)
        pack_off = 0
        for p in got["peers"]:
            q = p["rank"]
            send = pl["send"].get(q, np.zeros(0, np.int64))
            roff, rcnt = pl["recv"].get(q, (0, 0))
            assert p["send_count"] == len(send), (case, r, q)
            assert (p["recv_offset"], p["recv_count"]) == (roff, rcnt), (case, r, q)
            contiguous = len(send) == 0 or bool(np.all(np.diff(send) == 1))
            assert bool(p["packed"]) == (not contiguous), (case, r, q)
            if p["packed"]:
                assert p["pack_off"] == pack_off, (case, r, q)
                rows = got["pack"][p["pack_off"]:p["pack_off"] + p["send_count"]]
                pack_off += p["send_count"]
            else:
                rows = p["send_begin"] + np.arange(p["send_count"])
            assert np.array_equal(rows, send), (case, r, q)
        assert len(got["pack"]) == pack_off, (case, r)


def test_cases_reach_their_paths():
    """The cases are what their comments say, by the oracle's plan and the planner's alike."""
    (got, pl), = _planned("fd8-P1")
    assert got["peers"] == [] and len(got["halo"]) == 0 and not pl["send"] and not pl["recv"]
    mid = _planned("tri3-P3")[1][0]
    assert [p["rank"] for p in mid["peers"]] == [0, 2] and not any(p["packed"] for p in mid["peers"])
    lo, empty, hi = (g for g, _ in _planned("tri6-empty-rank"))
    assert empty["peers"] == [] and len(empty["lcol"]) == 0
    assert [p["rank"] for p in lo["peers"]] == [2] and [p["rank"] for p in hi["peers"]] == [0]
    assert any(p["packed"] for g, _ in _planned("fd6-permuted-P2") for p in g["peers"])


@pytest.mark.parametrize("bad", [6, 7, -1, -2 ** 31])
def test_column_out_of_range_is_refused(bad):
    A = _tridiag(6)
    rs = np.array([0, 3, 6], dtype=np.int64)
    for r in range(2):
        rb, re = int(rs[r]), int(rs[r + 1])
        e0, e1 = int(A.indptr[rb]), int(A.indptr[re])
        cols = A.indices[e0:e1].astype(np.int64)
        assert lab_plan(6, rs, 2, r, A.indptr[rb:re + 1], cols)[0] == N.PSK_OK
        for j in (0, len(cols) - 1):
            c = cols.copy()
            c[j] = bad
            assert lab_plan(6, rs, 2, r, A.indptr[rb:re + 1], c)[0] == N.PSK_ERR_ARG
