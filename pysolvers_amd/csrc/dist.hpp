// dist.hpp — the distributed layer's internal header: communicators, the shared-memory segment they map, the
// device mailbox, the host shard planner and the halo transport. Included only by the translation units that use
// a communicator; everything else sees a psk_csr's `comm` as an opaque pointer (psk_internal.hpp).
//   dist.hip          communicator lifecycle, creation of sharded matrices, halo queries
//   dist_plan.hip     host shard planning (no HIP, no RCCL, no Context)
//   dist_halo.hip     halo exchange and the collectives, over RCCL or the shared-memory transport
//   dist_mailbox.hip  device-side exchange of the ranks' scalars through host-shared memory
//   shmcomm.hip       the shared-memory transport and the shared segment both it and the mailbox map
#pragma once

#include "psk_internal.hpp"

#include <rccl/rccl.h>

#include <atomic>

#define PSK_RCCL(call)                                                                           \
    do {                                                                                         \
        ncclResult_t _r = (call);                                                                \
        if (_r != ncclSuccess)                                                                   \
            return ::psk::fail(PSK_ERR_RCCL, std::string(#call) + ": " + ncclGetErrorString(_r)); \
    } while (0)

namespace psk {

void rccl_comm_count(int delta);   // live RCCL communicators (psk_shutdown_ex resets the device only at 0)

// ---------------------------------------------------------------------------------------------
// A named POSIX shared-memory segment every rank of the node maps and registers with HIP (shmcomm.hip). A new
// segment is zero-filled, so a counter in its header starts at 0. shm_segment_open leaves nothing behind when it
// fails; shm_segment_close undoes it (unregister, unmap, and `owner` — rank 0 — unlinks the name) and may be
// called on a segment that was never opened. `who` prefixes the error messages (the entry point's name).
struct ShmSegment {
    std::string name;
    char *base = nullptr;
    size_t bytes = 0;
    bool registered = false, owner = false;
};
int shm_segment_open(ShmSegment &g, const char *who, const char *name, size_t bytes, unsigned register_flags,
                     bool owner);
// counts this rank in and waits (60 s) until all P ranks of the communicator have attached
int shm_segment_attach(const char *who, std::atomic<int32_t> *attached, int P);
void shm_segment_close(ShmSegment &g);

// Device-side exchange of the solvers' per-rank scalars through a host-shared mailbox (dist_mailbox.hip,
// psk_comm_mailbox; round 5): the kernel that finishes a rank's grid sums stores them straight into
// every rank's slot of the exchange (system-scope stores to pinned host memory mapped by all ranks of
// the node), and a one-wave kernel on each rank waits for the P values of its own slot, copies them to
// the gathered array the solver sums in rank order and re-arms the slot. Slot index (reader q, ring
// position e mod kMbRing of exchange e, writer r, component c): ((q*kMbRing + e%kMbRing)*P + r)*kMbW + c.
constexpr int kMbRing = 4;
constexpr int kMbW = 2;
struct Mailbox {
    ShmSegment seg;           // the mapped segment (4 KiB header, then the slots)
    uint64_t *dev = nullptr;  // device address of the slots
    int P = 1, rank = 0;
    uint64_t seq = 0;         // exchanges issued on this communicator (identical on every rank)
};
}  // namespace psk

struct psk_comm {
    int nranks = 1;
    int rank = 0;
    int device = 0;
    ncclComm_t nccl = nullptr;
    bool dry = false;     // psk_comm_init_dry: builds shards, no collectives (single-GPU validation)
    psk::ShmComm *shm = nullptr;   // psk_comm_init_host: shared-memory transport (shmcomm.hip)
    psk::Mailbox *mb = nullptr;    // psk_comm_mailbox: device-side scalar exchange (dist_mailbox.hip)
};

namespace psk {
// shared-memory transport (shmcomm.hip): stream-ordered like the RCCL calls they stand in for
int shm_allgather(psk_comm *c, const double *send, double *recv, int64_t count, hipStream_t s);
int shm_exchange(psk_comm *c, int npeers, const int *peers, const double *const *sends, const int64_t *send_counts,
                 double *const *recvs, const int64_t *recv_counts, hipStream_t s);
int shm_allgather_host(psk_comm *c, const void *mine, void *all, size_t bytes);
int shm_exchange_host(psk_comm *c, int npeers, const int *peers, const void *const *sends, const size_t *send_bytes,
                      void *const *recvs, const size_t *recv_bytes);
int shm_error(const psk_comm *c);
void shm_close(psk_comm *c);

// ---------------------------------------------------------------------------------------------
// host shard planning (dist_plan.hip): index arithmetic only

// Row-block plan of the m x m 5-point matrix over P ranks: whole grid lines per rank; local column
// layout [owned | halo_lo (previous rank's last line) | halo_hi (next rank's first line)].
struct FdPlan {
    int64_t rb, re, nloc, ncols, halo_lo, halo_hi;
};
int fd2d_plan(int64_t m, int P, int r, FdPlan &p);
// its halo peers (ranks r - 1 and r + 1, one grid line each way, contiguous) and the halo columns' global ids
void fd2d_peers(int64_t m, int r, const FdPlan &p, std::vector<HaloPeer> &peers, std::vector<int64_t> &halo_cols);

// Plan of rank r's block of a general global CSR, rows [rs[r], rs[r+1]) (dist_plan.hip has the rules)
struct DistPlan {
    int64_t rb = 0, re = 0, nloc = 0;
    std::vector<int32_t> lcol;                    // local column of every local entry
    std::vector<int64_t> halo;                    // global ids of the halo columns (ascending)
    std::vector<int64_t> recv_off, recv_cnt;      // per rank: halo segment it owns
    std::vector<std::vector<int32_t>> send_rows;  // per rank: owned local rows it needs
};
int dist_plan(int64_t n_global, const int64_t *rs, int P, int r, const int64_t *rowptr, const int32_t *colidx,
              DistPlan &pl);
// its halo peers in rank order, and the send rows of the packed ones concatenated (HaloPeer::pack_off)
void dist_peers(const DistPlan &pl, std::vector<HaloPeer> &peers, std::vector<int32_t> &pack);

// ---------------------------------------------------------------------------------------------
// halo transport and collectives (dist_halo.hip)
int halo_exchange(psk_csr *A, double *x_local, hipStream_t s);
// the exchange on stream cs after the work enqueued on s (ev_a), completion recorded in ev_b
int halo_exchange_async(psk_csr *A, double *x, hipStream_t s, hipStream_t cs, hipEvent_t ev_a, hipEvent_t ev_b,
                        hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
// rows sent to peers confined to the first lo / the tiles from hi on (of nv tiles of `tile` rows)
bool halo_split(const psk_csr *A, int64_t tile, int64_t nv, int64_t &lo, int64_t &hi);
// the two steps of an exchange's send side: gather the packed peers' rows of x into A->sendbuf on s, and where
// peer p's send data then starts (its segment of the send buffer, or its contiguous owned range of x)
int halo_pack(psk_csr *A, const double *x, hipStream_t s);
const double *halo_send_ptr(const psk_csr *A, const HaloPeer &p, const double *x);
// recv[q*count + i] = rank q's send[i]: no arithmetic, so every rank holds the same bits and
// reduces them in rank order itself (RCCL's reduction order is algorithm- and rank-dependent)
int allgather(psk_csr *A, const double *send, double *recv, int64_t count, hipStream_t s);
// synchronous host-buffer collectives for creation-time checks, over the communicator's transport
int host_allgather(psk_comm *cm, const void *mine, void *all, size_t bytes);
int host_exchange(psk_comm *cm, const std::vector<int> &peers, const std::vector<const void *> &sends,
                  const std::vector<size_t> &sb, const std::vector<void *> &recvs, const std::vector<size_t> &rb);

// ---------------------------------------------------------------------------------------------
// mailbox exchanges (dist_mailbox.hip; psk_comm::mb): the next exchange's writer slots into gs (producer launch),
// and the gather of that exchange into recv[q*W + c] on s (skipped on the device when *done is set: the producer
// did not run either); returns the exchange number
uint64_t mbox_next(psk_comm *c, GridSum *gs);
int mbox_gather(psk_comm *c, uint64_t seq, int W, double *recv, const int32_t *done, hipStream_t s,
                hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
void mbox_close(psk_comm *c);   // detaches the communicator's mailbox, if any (psk_comm_destroy)

}  // namespace psk
