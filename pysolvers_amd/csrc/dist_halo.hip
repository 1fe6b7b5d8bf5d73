// dist_halo.hip — what the ranks of a sharded solve send each other: the halo exchange of a vector and the
// all-gather of the ranks' scalars, over RCCL or the shared-memory transport (shmcomm.hip), and the synchronous
// host-buffer forms of both that matrix creation checks its plan with.
//
// No reference counterpart: PySolvers is single-process. The sharded PCG is the same loop as
// pcg.hip; per iteration it adds (1) a halo exchange of the search direction p with the two
// neighbouring ranks (grouped ncclSend/ncclRecv of one grid line each way for the 5-point FD
// matrix: m doubles per side), and (2) two ncclAllGather of the ranks' dot products (p.Ap; then
// r.r and u.r fused). Every rank then sums the gathered values in rank order itself, so all ranks
// hold bit-identical scalars and stop on the same iteration without further communication (an
// all-reduce would leave the order of the rank sum to RCCL's algorithm choice).
#include "dist.hpp"

#include <algorithm>

namespace psk {

// sendbuf[k] = x[idx[k]]: the owned entries the peers need, packed peer by peer
__global__ void halo_pack_kernel(int64_t count, const int32_t *__restrict__ idx, const double *__restrict__ x,
                                 double *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) out[k] = x[idx[k]];
}

int halo_pack(psk_csr *A, const double *x, hipStream_t s) {
    if (A->pack_count == 0) return PSK_OK;
    hipLaunchKernelGGL(halo_pack_kernel, dim3((unsigned)((A->pack_count + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       A->pack_count, A->pack_idx, x, A->sendbuf.as<double>());
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

const double *halo_send_ptr(const psk_csr *A, const HaloPeer &p, const double *x) {
    return p.packed ? A->sendbuf.as<double>() + p.pack_off : x + p.send_begin;
}

int halo_exchange(psk_csr *A, double *x, hipStream_t s) {
    if (!A->comm || A->peers.empty()) return PSK_OK;
    if (A->comm->dry) return PSK_OK;   // the caller supplied the halo entries
    ncclComm_t nc = A->comm->nccl;
    PSK_TRY(halo_pack(A, x, s));
    if (A->comm->shm) {
        std::vector<int> pr;
        std::vector<const double *> sd;
        std::vector<double *> rv;
        std::vector<int64_t> sc, rc;
        for (const HaloPeer &p : A->peers) {
            pr.push_back(p.rank);
            sd.push_back(halo_send_ptr(A, p, x));
            sc.push_back(p.send_count);
            rv.push_back(x + A->n + p.recv_offset);
            rc.push_back(p.recv_count);
        }
        return shm_exchange(A->comm, (int)pr.size(), pr.data(), sd.data(), sc.data(), rv.data(), rc.data(), s);
    }
    PSK_RCCL(ncclGroupStart());
    for (const HaloPeer &p : A->peers) {
        if (p.send_count > 0)
            PSK_RCCL(ncclSend(halo_send_ptr(A, p, x), (size_t)p.send_count, ncclDouble, p.rank, nc, s));
        if (p.recv_count > 0)
            PSK_RCCL(ncclRecv(x + A->n + p.recv_offset, (size_t)p.recv_count, ncclDouble, p.rank, nc, s));
    }
    PSK_RCCL(ncclGroupEnd());
    return PSK_OK;
}

// The halo exchange on the second stream `cs`, after the work already enqueued on `s` (event ev_a);
// ev_b marks its completion for the consumer (the next SpMV waits on it).
// t0 / t1 (optional, timing): recorded on `cs` around the exchange itself
int halo_exchange_async(psk_csr *A, double *x, hipStream_t s, hipStream_t cs, hipEvent_t ev_a, hipEvent_t ev_b,
                        hipEvent_t t0, hipEvent_t t1) {
    PSK_HIP(hipEventRecord(ev_a, s));
    PSK_HIP(hipStreamWaitEvent(cs, ev_a, 0));
    if (t0) PSK_HIP(hipEventRecord(t0, cs));
    PSK_TRY(halo_exchange(A, x, cs));
    if (t1) PSK_HIP(hipEventRecord(t1, cs));
    PSK_HIP(hipEventRecord(ev_b, cs));
    return PSK_OK;
}

// Overlap plan: true when every row sent to a peer lies in a prefix [0, lo*tile) or a suffix
// [hi*tile, n) of the owned rows (contiguous sends: row blocks of banded matrices) and the middle
// [lo, hi) is at least a quarter of the `nv` tiles, so that K3 can run the send tiles first.
bool halo_split(const psk_csr *A, int64_t tile, int64_t nv, int64_t &lo, int64_t &hi) {
    if (!A->comm || A->peers.empty() || A->comm->dry) return false;
    int64_t pre = 0, suf = A->n;
    for (const HaloPeer &p : A->peers) {
        if (p.send_count == 0) continue;
        if (p.packed) return false;
        const int64_t b = p.send_begin, e = p.send_begin + p.send_count;
        if (b == 0) pre = std::max(pre, e);
        else if (e == A->n) suf = std::min(suf, b);
        else return false;
    }
    lo = (pre + tile - 1) / tile;
    hi = suf / tile;
    return hi > lo && (hi - lo) * 4 >= nv;
}

int allgather(psk_csr *A, const double *send, double *recv, int64_t count, hipStream_t s) {
    if (!A->comm) return fail(PSK_ERR_ARG, "allgather on an unsharded matrix");
    if (A->comm->dry) return fail(PSK_ERR_UNSUPPORTED, "collective on a dry (RCCL-less) communicator");
    if (A->comm->shm) return shm_allgather(A->comm, send, recv, count, s);
    PSK_RCCL(ncclAllGather(send, recv, (size_t)count, ncclDouble, A->comm->nccl, s));
    return PSK_OK;
}

// Synchronous host-buffer collectives for creation-time checks, over the communicator's transport
// (RCCL: staged through device memory on libpsk's stream; shared memory: shmcomm.hip).
int host_allgather(psk_comm *cm, const void *mine, void *all, size_t bytes) {
    if (cm->shm) return shm_allgather_host(cm, mine, all, bytes);
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    DevBuf d;
    DevBufRelease rel{d};
    PSK_TRY(d.ensure(bytes * (size_t)(cm->nranks + 1) + 64));
    char *dm = d.as<char>(), *da = dm + bytes;
    PSK_HIP(hipMemcpy(dm, mine, bytes, hipMemcpyHostToDevice));
    PSK_RCCL(ncclAllGather(dm, da, bytes, ncclUint8, cm->nccl, s));
    PSK_HIP(hipMemcpyAsync(all, da, bytes * (size_t)cm->nranks, hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    return PSK_OK;
}

int host_exchange(psk_comm *cm, const std::vector<int> &peers, const std::vector<const void *> &sends,
                  const std::vector<size_t> &sb, const std::vector<void *> &recvs, const std::vector<size_t> &rb) {
    const int np = (int)peers.size();
    if (cm->shm) return shm_exchange_host(cm, np, peers.data(), sends.data(), sb.data(), recvs.data(), rb.data());
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    size_t tot = 0;
    for (int k = 0; k < np; ++k) tot += sb[(size_t)k] + rb[(size_t)k];
    DevBuf d;
    DevBufRelease rel{d};
    PSK_TRY(d.ensure(tot + 64));
    char *p = d.as<char>();
    std::vector<char *> dr((size_t)np);
    PSK_RCCL(ncclGroupStart());
    for (int k = 0; k < np; ++k) {
        if (sb[(size_t)k]) {
            PSK_HIP(hipMemcpy(p, sends[(size_t)k], sb[(size_t)k], hipMemcpyHostToDevice));
            PSK_RCCL(ncclSend(p, sb[(size_t)k], ncclUint8, peers[(size_t)k], cm->nccl, s));
            p += sb[(size_t)k];
        }
        dr[(size_t)k] = p;
        if (rb[(size_t)k]) {
            PSK_RCCL(ncclRecv(p, rb[(size_t)k], ncclUint8, peers[(size_t)k], cm->nccl, s));
            p += rb[(size_t)k];
        }
    }
    PSK_RCCL(ncclGroupEnd());
    for (int k = 0; k < np; ++k)
        if (rb[(size_t)k]) PSK_HIP(hipMemcpyAsync(recvs[(size_t)k], dr[(size_t)k], rb[(size_t)k], hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    return PSK_OK;
}

}  // namespace psk
