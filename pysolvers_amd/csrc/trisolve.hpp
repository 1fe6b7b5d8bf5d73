// trisolve.hpp — what the triangular-solve files (trisolve*.hip) share: the publication protocol, the
// forward-progress words, the layout constants the host planner and the kernels agree on, the planner's
// types and one launch function per schedule. TriFactor itself is in psk_internal.hpp (psk_prec holds two).
#pragma once
#include "psk_internal.hpp"

#include <vector>

namespace psk {

// Publication protocol (every spin-waiting schedule): the output is pre-filled with a signalling-NaN sentinel
// that arithmetic never produces; each x[i] is written by ONE 8-byte agent-scope store (sc1) and read by
// agent-scope relaxed loads that bypass the non-coherent L1 (MI355X_MICROARCH.md, hand-off granule
// R2: "the data IS the flag"). Every spin is bounded and reports PSK_ERR instead of hanging.
constexpr uint64_t kSentinel = 0x7FF4DEAD0000BEEFull;   // sNaN payload: never an arithmetic result
constexpr int64_t kMaxSpins = 1ll << 24;

__device__ __forceinline__ double load_pub(const double *p) {
    const uint64_t b = __hip_atomic_load(reinterpret_cast<const uint64_t *>(p), __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ void store_pub(double *p, double v) {
    __hip_atomic_store(reinterpret_cast<uint64_t *>(p), (uint64_t)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool is_sentinel(double v) { return (uint64_t)__double_as_longlong(v) == kSentinel; }

__device__ __forceinline__ double wait_pub(const double *p, int32_t *err) {
    double xv = load_pub(p);
    int64_t spins = 0;
    while (is_sentinel(xv)) {
        if (++spins > kMaxSpins) {
            atomicExch(err, 1);
            return 0.0;
        }
        __builtin_amdgcn_s_sleep(4);   // sleep 1 / 4 / 12 between polls: AMG 8192^2 2.90 / 2.92 / 2.90 it/s
        xv = load_pub(p);
    }
    return xv;
}

// ---- forward progress without co-residency (round 5) ---------------------
// The spin-waiting schedules no longer assume that every workgroup of their grid is resident at once (a
// plain launch promises nothing: a caller's kernels on other streams, a second process on the device or
// the halo exchange's kernels may hold CUs). Each takes its work from counters in TriFactor::sched (words
// on separate 256-B lines, zero between launches):
//  * band / narrow band / grid: a workgroup draws its next block (band) from a ticket counter instead of
//    deriving it from blockIdx.x. A block waits only on earlier blocks, and every earlier block was drawn
//    by a workgroup that has started and runs to completion, so the lowest unfinished block can always
//    proceed. The drawer of the launch's last ticket re-arms the counter.
//  * sync-free: a row may wait on ANY earlier position, so rows are dealt round-robin over the waves that
//    ENROLLED: the first workgroup to start waits until all gridDim.x have enrolled or kEnrollWaitTicks
//    have passed, closes the enrolment and publishes the count R; positions are dealt over those 4R waves,
//    and workgroups that arrive later leave at once. Every row is then held by a running wave. The last
//    workgroup to leave re-arms the words.
// The grid is unchanged when the device is free (all workgroups enrol within a few us); under contention
// the solve runs on fewer waves instead of waiting on workgroups that cannot start.
// kSchedTicket / kSchedPub / kSchedExit / kSchedLast / kSchedWords: psk_internal.hpp (the lab library reads kSchedLast)
constexpr uint32_t kEnrollClosed = 0x80000000u;
constexpr uint64_t kEnrollWaitTicks = 2000;   // s_memrealtime (100 MHz): 20 us

__device__ __forceinline__ uint32_t sched_add(uint32_t *w, uint32_t v) {
    return __hip_atomic_fetch_add(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t sched_load(const uint32_t *w) {
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sched_store(uint32_t *w, uint32_t v) {
    __hip_atomic_store(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// thread 0: the next block of a ticket-dealt launch (every workgroup draws until it gets one >= nblocks,
// so the launch draws exactly nblocks + gridDim.x tickets; the last drawer re-arms the counter)
__device__ __forceinline__ int64_t sched_next_block(uint32_t *sched, int64_t nblocks) {
    const uint32_t t = sched_add(sched + kSchedTicket, 1u);
    if ((int64_t)t == nblocks + (int64_t)gridDim.x - 1) sched_store(sched + kSchedTicket, 0u);
    return t;
}

// thread 0: the block of a launch in which every workgroup draws exactly one (the grid schedule's bands);
// the drawer of ticket gridDim.x - 1 re-arms the counter
__device__ __forceinline__ int64_t sched_one_block(uint32_t *sched) {
    const uint32_t t = sched_add(sched + kSchedTicket, 1u);
    if (t == gridDim.x - 1) sched_store(sched + kSchedTicket, 0u);
    return t;
}

// every thread: enrol this workgroup (see above); returns its worker rank (-1: arrived after the close) and
// the worker count R in *R. Bounded: the decider waits at most kEnrollWaitTicks.
__device__ __forceinline__ int sched_enroll(uint32_t *sched, uint32_t *R, int32_t *err) {
    __shared__ int s_rank;
    __shared__ uint32_t s_R;
    if (threadIdx.x == 0) {
        const uint32_t G = gridDim.x;
        const uint32_t old = sched_add(sched + kSchedTicket, 1u);
        if (old & kEnrollClosed) {
            s_rank = -1;
            s_R = 0;
        } else if (old == 0) {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            while ((sched_load(sched + kSchedTicket) & ~kEnrollClosed) < G &&
                   __builtin_amdgcn_s_memrealtime() - t0 < kEnrollWaitTicks)
                __builtin_amdgcn_s_sleep(2);
            const uint32_t r = __hip_atomic_fetch_or(sched + kSchedTicket, kEnrollClosed, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT) & ~kEnrollClosed;
            sched_store(sched + kSchedPub, r);
            sched_store(sched + kSchedLast, r);   // kept after the launch (psk_lab_trisolve_workers)
            s_rank = 0;
            s_R = r;
        } else {
            uint32_t r;
            int64_t spins = 0;
            while ((r = sched_load(sched + kSchedPub)) == 0) {
                if (++spins > kMaxSpins) {
                    atomicExch(err, 4 << 24);
                    r = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            s_rank = (int)old;
            s_R = r;
        }
    }
    __syncthreads();
    *R = s_R;
    return s_rank;
}

// every thread, at the very end of an enrolled launch (after the workgroup's last use of the words)
__device__ __forceinline__ void sched_leave(uint32_t *sched) {
    __syncthreads();
    if (threadIdx.x == 0 && sched_add(sched + kSchedExit, 1u) == gridDim.x - 1) {
        sched_store(sched + kSchedTicket, 0u);
        sched_store(sched + kSchedPub, 0u);
        sched_store(sched + kSchedExit, 0u);
    }
}

__device__ __forceinline__ void drain_vm() { __builtin_amdgcn_s_waitcnt(0x0F70); }   // vmcnt(0) only
__device__ __forceinline__ int32_t opaque_zero() {
    int32_t z;
    __asm__ volatile("v_mov_b32 %0, 0" : "=v"(z));
    return z;
}

// ---- what more than one kernel file uses, and the layout constants the host planner shares with them ------
// sync-free family (sync-free, LDS, partitioned kernels): row header, tail chunks, row total
struct SfHead {
    int32_t row, s, e;
};
constexpr int kSfTail = 4;
// Row total of the sync-free family (sync-free, LDS, partitioned kernels: the same function, so the
// three give identical bits): the DPP wave total (psk_internal.hpp), ~130 cycles on the dependency
// chain where a butterfly of ds_bpermute shuffles took ~700 (tools/part_micro.py trace, FD chain).
__device__ __forceinline__ double row_total(double v) { return wave_total(v); }
// LDS: the largest factor whose x one workgroup holds
constexpr int64_t kLdsMaxRows = 18432;   // 144 KiB of x
// partitioned: one workgroup of 16 waves per strip, an LDS cache of kPartSlots results, entry arrays padded
constexpr int kPartThreads = 1024;
constexpr int kPartWaves = kPartThreads / 64;
constexpr int kPartSlots = 8192;                // 64 KiB of values + 32 KiB of tags
constexpr int kPtChunks = 2;   // 64-entry chunks of a row held in registers (4 rows in flight per wave)
constexpr int kPartPadEntries = 64 * kPtChunks;
// band / narrow band: LDS ring, staged chunks, the LDS a launch asks for (trisolve_band.hip)
constexpr int kRingMaxWords = 16384;                     // 128 KiB LDS ring (then 1 workgroup / CU)
constexpr int kBandChunk = kBlock;   // records per staged chunk = widest level = threads
constexpr int kNarrowBufs = 3;
constexpr int kNarrowChunk = 128;   // records per buffer
constexpr int kNarrowWidth = 64;    // widest local level (one wave)
size_t band_lds_bytes(int ring_words, int K);
size_t narrow_lds_bytes(int ring_words, int K);
// grid: one wave per band of kGridLanes lines; the levels kernel uses the buffer accessors too
constexpr int kGridLanes = 64;
constexpr int kGridMaxRing = 128;   // ring rows the plan may ask for (the kernel's mirrored kGridRing)
// Records of one step of a band: three contiguous 64-lane fields — K 16-bit pattern codes per lane,
// K values per lane (stored entry order), the diagonal — so each field load is one contiguous access
// (one 32-B record per lane, loaded as two 16-B halves, touched twice the cache lines and ran the
// 5-point sweep 1.6x slower).
template <int K>
struct GridStep {
    static constexpr int64_t kCode = 0;                                   // uint16 [64][K]
    static constexpr int64_t kCoef = kGridLanes * 2 * K;                  // double [64][K]
    static constexpr int64_t kDiag = kCoef + kGridLanes * 8 * K;          // double [64]
    static constexpr int64_t kBytes = kDiag + kGridLanes * 8;
};
// the skewed step of line y's first position: g(y) = (sigma2 * y + phase) >> 1 (sigma2 = twice the skew)
__host__ __device__ __forceinline__ int64_t grid_g(int64_t sigma2, int64_t phase, int64_t y) {
    return (sigma2 * y + phase) >> 1;
}
// Buffer (bounds-checked) access for the solver wave's rhs loads and x stores: an out-of-range
// offset loads 0 / drops the store in hardware, so every lane issues every load and store with no
// branch around it. The compiler's vmcnt waits count only memory operations it knows were issued:
// with the rhs load and the two x stores under divergent branches it assumed one operation per step
// (the record index) and waited with vmcnt(10) — i.e. for stores and loads issued ~3 steps before,
// write-through stores included — where the prefetch runs D steps ahead. Byte offsets are 32-bit:
// the grid schedule takes factors of at most kGridMaxRows rows (host check).
constexpr uint32_t kBufOOB = 0xFFFFFFFFu;
constexpr int64_t kGridMaxRows = (int64_t)1 << 29;
typedef unsigned int grid_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t grid_rsrc(const double *p, int64_t n) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(p), (short)0, (int)(uint32_t)(n * 8), 0x00020000);
}
__device__ __forceinline__ double grid_bload(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
}
template <int CPOL>   // 0x10: sc1 (agent-scope write-through, the publication store), 0: plain
__device__ __forceinline__ void grid_bstore(__amdgpu_buffer_rsrc_t r, uint32_t off, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(grid_u2, v), r, off, 0, CPOL);
}
// levels: record fields and the limits of a plan
constexpr uint32_t kLevelIdle = 0xFFFFFFFFu;   // row field of an idle lane
constexpr int kLevelMaxK = 16, kLevelMaxW = 256, kLevelD = 4, kLevelPad = 8;   // D: steps loaded ahead (PSK_LEVELS_D=8: lab)
constexpr int64_t kLevelMaxSlots = 18432;     // live values + the zero and trash slots: <= 144 KiB of LDS

// ---- host planner (trisolve_plan.hip): pure host code, no HIP call, no Context --------------------------
struct HostFactor {
    int64_t n = 0;
    bool upper = false;
    std::vector<int32_t> rp, ci;   // off-diagonal entries
    int64_t pos(int64_t i) const { return upper ? n - 1 - i : i; }
    int64_t row(int64_t p) const { return upper ? n - 1 - p : p; }
};

// Split one host CSR factor into off-diagonal entries + diagonal. lower: entries must have c <= i.
int split_factor(int64_t n, const int32_t *rp, const int32_t *ci, const double *va, bool lower, bool unit,
                 std::vector<int32_t> &orp, std::vector<int32_t> &oci, std::vector<double> &ova, std::vector<double> &dg);

// Global dependency levels of F: lev[i] = the level of row i, order = the rows sorted by level (solve order inside
// one), nlev = the number of levels.
void level_order(const HostFactor &F, std::vector<int32_t> &order, std::vector<int32_t> &lev, int64_t &nlev);

struct GridPlan {
    bool ok = false;
    int64_t w = 0, H = 0, sigma2 = 0, phase = 0, off = 0;   // g(y) = (sigma2 * y + phase) >> 1
    int K = 0, pe = 0, maxyd = 0, ring = 0;
    GridExt ext{};
    double est = -1.0;
};
void plan_grid(const HostFactor &F, GridPlan &g);

// What make_factor uploads: T holds the chosen schedule, the estimates and the scalars of every layout built
// (its device pointers stay null), the vectors the arrays those pointers will hold.
struct FactorPlan {
    TriFactor T;
    std::vector<int32_t> krp, kci, order;   // the sync-free kernel's copy, in solve order
    std::vector<double> kva, dg;
    std::vector<int32_t> rec_row, rec_end, rec_c;   // band
    std::vector<double> rec_v, rec_d;
    std::vector<double> gcoef, gdict;   // grid
    std::vector<uint32_t> gidx;
    std::vector<int64_t> pseg;   // partitioned
    std::vector<int32_t> prp, pcode, prow;
    std::vector<double> pva;
    std::vector<uint64_t> lrc, lsl;   // levels
    std::vector<double> lcf, ldg;
};
// Plan one factor (CSR with its diagonal unless `unit`; nat: natural index of every row, or empty) for a
// device of num_cus CUs whose sync-free launch runs syncfree_waves waves.
int plan_factor(int64_t n, const int32_t *rp, const int32_t *ci, const double *va, bool upper, bool unit,
                const std::vector<int32_t> &nat, int num_cus, int64_t syncfree_waves, FactorPlan &out);

// ---- x = T^-1 rhs[rhs_idx] with one schedule's kernel (trisolve_<schedule>.hip) ---------------------------
using TriLaunch = int(const Context *c, int64_t n, const TriFactor &T, const double *rhs, const int32_t *rhs_idx,
                      double *x, int32_t *err, hipStream_t s);
TriLaunch launch_syncfree, launch_lds, launch_part, launch_band, launch_grid, launch_levels;
// T.sweeps Jacobi sweeps in place of the factor's schedule (trisolve_sweep.hip; psk_prec_trisolve_sweeps): plain
// launches, no sentinel, no scheduling words, err never written
TriLaunch launch_sweeps;
constexpr int32_t kMaxSweeps = 65536;
// the sentinel on the rows the grid schedule publishes (gate != nullptr: only when *gate is set)
int launch_grid_fill(const TriFactor &T, int64_t n, double *x, const int32_t *gate, hipStream_t s);

}  // namespace psk
