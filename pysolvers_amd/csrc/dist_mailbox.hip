// dist_mailbox.hip — device-side scalar exchange through a host-shared mailbox (round 5; dist.hpp Mailbox).
// An RCCL all-gather of a few bytes costs a collective kernel launch and its protocol on the solver's
// stream (tens of us at P = 8 by DESIGN.md's budget), twice per PCG iteration, on the critical path. Here
// the kernel that finishes a rank's grid sums (gridsum_mail) stores them directly into every rank's slot,
// and each rank's one-wave gather kernel polls its own slot: one posted system-scope store per value and
// one host-memory round trip per poll. Value-is-flag: a slot holds a signalling-NaN sentinel until its
// value lands; the reader re-arms it after copying. Ring of kMbRing exchanges: exchange e + kMbRing is
// written by a rank only after it consumed exchange e + kMbRing - 1 from every rank, and every rank
// consumed e before producing e + 1 (each exchange's values come from a kernel that follows the gather
// of the previous one), so a slot is never overwritten before its reader re-armed it.
#include "dist.hpp"

#include <hip/hip_ext.h>

namespace psk {

constexpr size_t kMbHeader = 4096;
constexpr uint64_t kMbSentinel = 0x7FF0DEAD5EED0001ull;   // sNaN payload: never an arithmetic result
constexpr uint64_t kMbWaitTicks = (uint64_t)2 << 27;       // s_memrealtime (100 MHz): ~2.7 s

static inline size_t mb_index(const Mailbox &m, int q, int64_t slot, int r, int c) {
    return (((size_t)q * kMbRing + (size_t)slot) * (size_t)m.P + (size_t)r) * kMbW + (size_t)c;
}

uint64_t mbox_next(psk_comm *c, GridSum *gs) {
    Mailbox &m = *c->mb;
    const uint64_t e = m.seq++;
    gs->mb = m.dev + mb_index(m, 0, (int64_t)(e % kMbRing), m.rank, 0);
    gs->mb_q = (int64_t)kMbRing * m.P * kMbW;
    gs->mb_P = m.P;
    return e;
}

// lane q < P: writer q's W values of this rank's slot -> recv[q*W + c], then re-armed
__global__ void mbox_gather_kernel(uint64_t *mine, int P, int W, double *__restrict__ recv, const int32_t *done,
                                   int32_t *err) {
    if (done && __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;   // uniform
    const int q = threadIdx.x;
    if (q >= P) return;
    for (int c = 0; c < W; ++c) {
        uint64_t *p = mine + (size_t)q * kMbW + c;
        uint64_t v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (v == kMbSentinel) {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            while ((v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) == kMbSentinel) {
                if (__builtin_amdgcn_s_memrealtime() - t0 > kMbWaitTicks) {
                    atomicOr(err, 8);
                    v = 0x7FF8000000000000ull;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        recv[q * W + c] = __longlong_as_double((long long)v);
        __hip_atomic_store(p, kMbSentinel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // the re-arms are visible system-wide before this rank's next mailbox stores (a later kernel's), whatever the
    // other ranks' progress: exchange e + 4 reuses this slot
    __threadfence_system();
}

int mbox_gather(psk_comm *c, uint64_t seq, int W, double *recv, const int32_t *done, hipStream_t s, hipEvent_t ev0,
                hipEvent_t ev1) {
    Context *cx;
    PSK_TRY(ctx(&cx));
    if (!cx->gs_err) {   // the error word gridsum_check reports (allocated with the first grid sum)
        GridSum tmp;
        PSK_TRY(gridsum_prepare(cx, 1, 1, recv, &tmp));
    }
    Mailbox &m = *c->mb;
    if (W < 1 || W > kMbW) return fail(PSK_ERR_ARG, "mbox_gather: bad width");
    // ev0 / ev1 (optional, timing): recorded by the dispatch itself around the kernel (its wait for the ranks)
    hipExtLaunchKernelGGL(mbox_gather_kernel, dim3(1), dim3(64), 0, s, ev0, ev1, 0,
                          m.dev + mb_index(m, m.rank, (int64_t)(seq % kMbRing), 0, 0), m.P, W, recv, done, cx->gs_err);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// Maps the segment for the kernels, arms this rank's reader slots, then waits until all P ranks have attached.
static int mbox_open(Mailbox &m, const char *name) {
    const char *who = "psk_comm_mailbox";
    // mapped for the kernels (fine-grained: system-scope stores and loads are coherent across devices)
    PSK_TRY(shm_segment_open(m.seg, who, name, kMbHeader + (size_t)m.P * kMbRing * m.P * kMbW * sizeof(uint64_t),
                             hipHostRegisterMapped | hipHostRegisterPortable, m.rank == 0));
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, m.seg.base, 0) != hipSuccess)
        return fail(PSK_ERR_HIP, std::string(who) + ": hipHostGetDevicePointer");
    m.dev = reinterpret_cast<uint64_t *>(static_cast<char *>(dp) + kMbHeader);
    uint64_t *slots = reinterpret_cast<uint64_t *>(m.seg.base + kMbHeader);
    for (int64_t e = 0; e < kMbRing; ++e)   // this rank's reader slots: only it reads and re-arms them
        for (int r = 0; r < m.P; ++r)
            for (int k = 0; k < kMbW; ++k) slots[mb_index(m, m.rank, e, r, k)] = kMbSentinel;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    return shm_segment_attach(who, reinterpret_cast<std::atomic<int32_t> *>(m.seg.base), m.P);
}

void mbox_close(psk_comm *c) {
    if (!c->mb) return;
    shm_segment_close(c->mb->seg);
    delete c->mb;
    c->mb = nullptr;
}

// mailbox self-check: each rank stores (rank*4096 + r, -(rank*4096 + r)) into exchange r the way a
// solver's grid-sum finisher does, gathers the P pairs and verifies them (bounded waits: a value that
// never arrives is reported, not waited for). Collective: every rank of c, the same rounds.
__global__ void mbox_check_put_kernel(GridSum gs, double v) {
    if (threadIdx.x == 0) {
        const double r[2] = {v, -v};
        gridsum_mail<2>(gs, r);
    }
}

}  // namespace psk

using namespace psk;

extern "C" {

// Attach the host-shared mailbox `name` to the communicator (collective: every rank of c, one node).
int psk_comm_mailbox(psk_comm *c, const char *name) {
    if (!c || !name || name[0] != '/' || std::strlen(name) > 200)
        return fail(PSK_ERR_ARG, "psk_comm_mailbox: bad arguments (name must start with '/')");
    if (c->dry) return fail(PSK_ERR_UNSUPPORTED, "psk_comm_mailbox: dry communicator");
    if (c->mb) return fail(PSK_ERR_ARG, "psk_comm_mailbox: already attached");
    c->mb = new Mailbox();
    c->mb->P = c->nranks;
    c->mb->rank = c->rank;
    const int rc = mbox_open(*c->mb, name);
    if (rc != PSK_OK) mbox_close(c);
    return rc;
}

int psk_comm_mailbox_check(psk_comm *c, int32_t rounds) {
    if (!c || !c->mb || rounds < 1) return fail(PSK_ERR_ARG, "psk_comm_mailbox_check: no mailbox attached");
    Context *cx;
    PSK_TRY(ctx(&cx));
    const int P = c->nranks;
    DevBuf rb;
    DevBufRelease rel{rb};
    PSK_TRY(rb.ensure((size_t)P * 2 * sizeof(double)));
    std::vector<double> h((size_t)P * 2);
    for (int r = 0; r < rounds; ++r) {
        GridSum gs{};
        const uint64_t seq = mbox_next(c, &gs);
        hipLaunchKernelGGL(mbox_check_put_kernel, dim3(1), dim3(64), 0, cx->stream, gs, (double)(c->rank * 4096 + r));
        PSK_HIP(hipGetLastError());
        PSK_TRY(mbox_gather(c, seq, 2, rb.as<double>(), nullptr, cx->stream));
        PSK_HIP(hipMemcpyAsync(h.data(), rb.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, cx->stream));
        PSK_HIP(hipStreamSynchronize(cx->stream));
        PSK_TRY(gridsum_check(cx));   // a wait that expired (bit 8)
        for (int q = 0; q < P; ++q)
            if (h[2 * q] != (double)(q * 4096 + r) || h[2 * q + 1] != -(double)(q * 4096 + r))
                return fail(PSK_ERR_RCCL, "psk_comm_mailbox_check: rank " + std::to_string(q) + "'s value of exchange " +
                                              std::to_string(r) + " is wrong");
    }
    return PSK_OK;
}

}  // extern "C"
