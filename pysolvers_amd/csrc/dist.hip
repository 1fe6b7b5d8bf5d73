// dist.hip — row-block sharding across the GPUs of one node (one process per GPU, RCCL over xGMI): the
// communicator's lifecycle and the creation of a rank's shard of a matrix. Creation is validate -> plan
// (dist_plan.hip, host only) -> allocate and upload -> attach the plan -> SpMV layout; what the ranks exchange
// during a solve is dist_halo.hip and dist_mailbox.hip.
#include "dist.hpp"

#include <algorithm>
#include <climits>

namespace psk {

// Creation-time check (collective over all ranks, same verdict everywhere): the send and receive
// counts agree pairwise, then each rank's send list equals what its peer expects to receive.
static int dist_verify(psk_comm *cm, const DistPlan &pl) {
    const int P = cm->nranks;
    std::vector<int64_t> mine((size_t)2 * P), all((size_t)2 * P * P);
    for (int q = 0; q < P; ++q) {
        mine[(size_t)q] = (int64_t)pl.send_rows[(size_t)q].size();
        mine[(size_t)(P + q)] = pl.recv_cnt[(size_t)q];
    }
    PSK_TRY(host_allgather(cm, mine.data(), all.data(), mine.size() * 8));
    for (int a = 0; a < P; ++a)
        for (int b = 0; b < P; ++b)
            if (a != b && all[(size_t)(2 * P * a + b)] != all[(size_t)(2 * P * b + P + a)])
                return fail(PSK_ERR_ARG, "psk_csr_create_dist: halo counts disagree across ranks (pattern not "
                                         "structurally symmetric)");
    // send each owner the global ids we receive from it; receive the ids each peer receives from us
    std::vector<int> peers;
    std::vector<const void *> sends;
    std::vector<void *> recvs;
    std::vector<size_t> sb, rb;
    std::vector<std::vector<int64_t>> got((size_t)P);
    for (int q = 0; q < P; ++q) {
        const size_t ns = pl.send_rows[(size_t)q].size(), nr = (size_t)pl.recv_cnt[(size_t)q];
        if (ns == 0 && nr == 0) continue;
        got[(size_t)q].resize(ns);
        peers.push_back(q);
        sends.push_back(pl.halo.data() + (nr ? pl.recv_off[(size_t)q] : 0));
        sb.push_back(nr * 8);
        recvs.push_back(got[(size_t)q].data());
        rb.push_back(ns * 8);
    }
    PSK_TRY(host_exchange(cm, peers, sends, sb, recvs, rb));
    int32_t ok = 1;
    for (int q = 0; q < P && ok; ++q)
        for (size_t k = 0; k < pl.send_rows[(size_t)q].size(); ++k)
            if (got[(size_t)q][k] != pl.rb + pl.send_rows[(size_t)q][k]) {
                ok = 0;
                break;
            }
    std::vector<int32_t> oks((size_t)P);
    PSK_TRY(host_allgather(cm, &ok, oks.data(), 4));
    for (int q = 0; q < P; ++q)
        if (!oks[(size_t)q])
            return fail(PSK_ERR_ARG, "psk_csr_create_dist: halo lists disagree across ranks (pattern not "
                                     "structurally symmetric)");
    return PSK_OK;
}

// the planned shard onto the device: rowptr rebased to 0 in int32, the local columns, the values and the pack list
static int dist_upload(psk_csr *A, const int64_t *rowptr, const std::vector<int32_t> &lcol, const double *vals,
                       const std::vector<int32_t> &pack) {
    std::vector<int32_t> rp32((size_t)A->n + 1);
    for (int64_t i = 0; i <= A->n; ++i) rp32[(size_t)i] = (int32_t)(rowptr[i] - rowptr[0]);
    if (hipMemcpy(A->rowptr, rp32.data(), rp32.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (A->nnz > 0 && (hipMemcpy(A->colidx, lcol.data(), (size_t)A->nnz * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(A->vals, vals, (size_t)A->nnz * 8, hipMemcpyHostToDevice) != hipSuccess)))
        return fail(PSK_ERR_HIP, "psk_csr_create_dist: upload");
    if (pack.empty()) return PSK_OK;
    if (hipMalloc(&A->pack_idx, pack.size() * 4) != hipSuccess) return fail(PSK_ERR_ALLOC, "halo pack alloc");
    A->pack_count = (int64_t)pack.size();
    if (hipMemcpy(A->pack_idx, pack.data(), pack.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(PSK_ERR_HIP, "halo pack upload");
    return A->sendbuf.ensure(pack.size() * 8);
}

}  // namespace psk

using namespace psk;

extern "C" {

int psk_comm_unique_id(uint8_t *id) {
    if (!id) return fail(PSK_ERR_ARG, "NULL id");
    static_assert(sizeof(ncclUniqueId) <= PSK_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId uid;
    PSK_RCCL(ncclGetUniqueId(&uid));
    std::memset(id, 0, PSK_UNIQUE_ID_BYTES);
    std::memcpy(id, &uid, sizeof(uid));
    return PSK_OK;
}

int psk_comm_init(int32_t nranks, int32_t rank, const uint8_t *id, psk_comm **out) {
    if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(PSK_ERR_ARG, "psk_comm_init: bad arguments");
    psk_comm *c = new psk_comm();
    c->nranks = nranks;
    c->rank = rank;
    hipError_t e = hipGetDevice(&c->device);
    if (e != hipSuccess) {
        delete c;
        return fail(PSK_ERR_HIP, "hipGetDevice");
    }
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    ncclResult_t r = ncclCommInitRank(&c->nccl, nranks, uid, rank);
    if (r != ncclSuccess) {
        delete c;
        return fail(PSK_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    }
    rccl_comm_count(1);
    *out = c;
    return PSK_OK;
}

int psk_comm_init_dry(int32_t nranks, int32_t rank, psk_comm **out) {
    if (!out || nranks < 1 || rank < 0 || rank >= nranks) return fail(PSK_ERR_ARG, "psk_comm_init_dry: bad arguments");
    psk_comm *c = new psk_comm();
    c->nranks = nranks;
    c->rank = rank;
    c->dry = true;
    if (hipGetDevice(&c->device) != hipSuccess) c->device = 0;
    *out = c;
    return PSK_OK;
}

int psk_comm_destroy(psk_comm *c) {
    if (!c) return PSK_OK;
    mbox_close(c);
    if (c->nccl) {
        (void)ncclCommDestroy(c->nccl);
        rccl_comm_count(-1);
    }
    shm_close(c);
    delete c;
    return PSK_OK;
}

int psk_csr_create_fd2d_dist(double a, double b, int64_t m, psk_comm *cm, psk_csr **out,
                             int64_t *row_begin, int64_t *row_end) {
    if (!cm || !out || m < 1) return fail(PSK_ERR_ARG, "psk_csr_create_fd2d_dist: bad arguments");
    if ((m == 1 ? 1 : 5 * m * m - 4 * m) > kMaxNnz) return fail(PSK_ERR_UNSUPPORTED, "nnz > int32");
    FdPlan plan;
    PSK_TRY(fd2d_plan(m, cm->nranks, cm->rank, plan));
    Context *c;
    PSK_TRY(ctx(&c));
    // nnz of the local rows from the closed-form rowptr
    auto fdrp = [m](int64_t k) -> int64_t {
        int64_t mk = k < m ? k : m, top = k - m * (m - 1);
        if (top < 0) top = 0;
        return 5 * k - mk - top - (k + m - 1) / m - k / m;
    };
    psk_csr *A = nullptr;
    PSK_TRY(csr_new_device(plan.nloc, plan.ncols, fdrp(plan.re) - fdrp(plan.rb), &A));
    A->n_global = m * m;
    A->row_begin = plan.rb;
    A->row_end = plan.re;
    A->comm = cm;
    fd2d_peers(m, cm->rank, plan, A->peers, A->halo_cols);
    int rc = fd2d_fill(A, m, a, b, plan.rb, plan.re, plan.rb - plan.halo_lo, c->stream);
    if (rc == PSK_OK) rc = csr_finish_device(A, c->stream);
    if (rc != PSK_OK) {
        csr_discard(A);
        return rc;
    }
    *out = A;
    if (row_begin) *row_begin = plan.rb;
    if (row_end) *row_end = plan.re;
    return PSK_OK;
}

int psk_csr_create_dist(int64_t n_global, const int64_t *row_starts, const int64_t *rowptr, const int32_t *colidx,
                        const double *vals, psk_comm *cm, psk_csr **out) {
    if (!cm || !out || !row_starts || !rowptr || n_global < 0)
        return fail(PSK_ERR_ARG, "psk_csr_create_dist: bad arguments");
    const int P = cm->nranks, r = cm->rank;
    if (row_starts[0] != 0 || row_starts[P] != n_global)
        return fail(PSK_ERR_ARG, "psk_csr_create_dist: row_starts must run from 0 to n_global");
    for (int q = 0; q < P; ++q)
        if (row_starts[q + 1] < row_starts[q]) return fail(PSK_ERR_ARG, "psk_csr_create_dist: row_starts not monotone");
    if (n_global >= INT32_MAX) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_create_dist: int32 columns required");
    const int64_t nloc = row_starts[r + 1] - row_starts[r];
    for (int64_t i = 0; i < nloc; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(PSK_ERR_ARG, "psk_csr_create_dist: rowptr not monotone");
    const int64_t nnz = rowptr[nloc] - rowptr[0];
    if (nnz > kMaxNnz) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_create_dist: local nnz exceeds int32");
    if (nnz > 0 && (!colidx || !vals)) return fail(PSK_ERR_ARG, "psk_csr_create_dist: NULL entries");
    DistPlan pl;
    PSK_TRY(dist_plan(n_global, row_starts, P, r, rowptr, colidx, pl));
    if (!cm->dry) PSK_TRY(dist_verify(cm, pl));
    Context *c;
    PSK_TRY(ctx(&c));
    psk_csr *A = nullptr;
    PSK_TRY(csr_new_device(nloc, nloc + (int64_t)pl.halo.size(), nnz, &A));
    A->n_global = n_global;
    A->row_begin = pl.rb;
    A->row_end = pl.re;
    A->comm = cm;
    A->halo_cols = pl.halo;
    std::vector<int32_t> pack;
    dist_peers(pl, A->peers, pack);
    int rc = dist_upload(A, rowptr, pl.lcol, vals, pack);
    if (rc == PSK_OK) rc = csr_choose_layout(A, c->stream);
    if (rc != PSK_OK) {
        csr_discard(A);
        return rc;
    }
    *out = A;
    return PSK_OK;
}

int psk_csr_halo_peers(const psk_csr *A, int32_t *ranks, int64_t *send_counts, int64_t *recv_counts,
                       int64_t *recv_offsets, int32_t *npeers) {
    if (!A || !npeers) return fail(PSK_ERR_ARG, "psk_csr_halo_peers: bad arguments");
    *npeers = (int32_t)A->peers.size();
    for (size_t k = 0; k < A->peers.size(); ++k) {
        if (ranks) ranks[k] = A->peers[k].rank;
        if (send_counts) send_counts[k] = A->peers[k].send_count;
        if (recv_counts) recv_counts[k] = A->peers[k].recv_count;
        if (recv_offsets) recv_offsets[k] = A->peers[k].recv_offset;
    }
    return PSK_OK;
}

int psk_csr_halo_pack(const psk_csr *Ac, const double *x, double *out) {
    if (!Ac || !x || !out) return fail(PSK_ERR_ARG, "psk_csr_halo_pack: NULL argument");
    psk_csr *A = const_cast<psk_csr *>(Ac);
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    PSK_TRY(halo_pack(A, x, s));   // halo_exchange's own send side
    int64_t o = 0;
    for (const HaloPeer &p : A->peers) {
        if (p.send_count > 0)
            PSK_HIP(hipMemcpyAsync(out + o, halo_send_ptr(A, p, x), (size_t)p.send_count * 8, hipMemcpyDeviceToDevice, s));
        o += p.send_count;
    }
    PSK_HIP(hipStreamSynchronize(s));
    return PSK_OK;
}

int psk_csr_halo_cols(const psk_csr *A, int64_t *cols, int64_t *count) {
    if (!A || !count) return fail(PSK_ERR_ARG, "psk_csr_halo_cols: bad arguments");
    *count = (int64_t)A->halo_cols.size();
    if (cols) std::copy(A->halo_cols.begin(), A->halo_cols.end(), cols);
    return PSK_OK;
}

}  // extern "C"
