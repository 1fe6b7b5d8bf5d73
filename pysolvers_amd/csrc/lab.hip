// lab.hip — libpsk_lab.so: test / lab entry points kept OUT of the product library (round 6).
// A separate shared library linked against libpsk.so (one instance of its state): a co-running kernel that holds
// CUs while a solve runs (the forward-progress tests, tests/test_gpu_progress.py), a dispatch probe and the
// enrolment count of the last sync-free triangular-solve launch. Declared in include/psk_lab.h; nothing in the
// product path calls them.
#include "amg.hpp"
#include "dist.hpp"
#include "trisolve.hpp"
#include "pcg_state.hpp"
#include "solve_loop.hpp"
#include "../../include/psk_lab.h"

#include <algorithm>
#include <chrono>
#include <string>

namespace psk {

// ---- lab: a co-running kernel that holds CUs while a solve runs (tests of the forward-progress rule) ----
// occupy_kernel: `wgs` workgroups of 1024 threads (16 waves each) with `lds` bytes of LDS each, on a
// stream of their own, every wave spinning until the flag is set on the solver's stream (occupy_end) or
// the time limit passes. A solve enqueued between begin and end can only use what the occupiers leave.
__global__ __launch_bounds__(1024) void occupy_kernel(uint32_t *flag, int64_t *started, uint64_t ticks,
                                                      int32_t *timed_out) {
    extern __shared__ unsigned char occ_lds[];
    if (threadIdx.x == 0) {
        occ_lds[0] = 1;
        __hip_atomic_fetch_add(started, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // which XCD holds this occupier (HW_REG_XCC_ID, bits 3:0): psk_lab_occupy_xcc
        const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;
        __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(timed_out) + 32 + xcc, 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > ticks) {
            if (threadIdx.x == 0) atomicOr(timed_out, 1);
            break;
        }
        __builtin_amdgcn_s_sleep(8);
    }
}
__global__ void occupy_release_kernel(uint32_t *flag) {
    __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

namespace {
struct Occupier {
    hipStream_t s = nullptr;
    uint32_t *dw = nullptr;       // [0] release flag, [64] timed-out word
    int64_t *started = nullptr;   // host-mapped count of started occupier workgroups
    bool active = false;
};
Occupier g_occ;
}  // namespace

}  // namespace psk

extern "C" int psk_lab_occupy_begin(int32_t wgs, int32_t lds_bytes, double seconds) {
    using namespace psk;
    Context *c;
    PSK_TRY(ctx(&c));
    if (g_occ.active) return fail(PSK_ERR_ARG, "psk_lab_occupy_begin: already active");
    if (wgs < 1 || lds_bytes < 16 || lds_bytes > 160 * 1024 || seconds <= 0)
        return fail(PSK_ERR_ARG, "psk_lab_occupy_begin: bad arguments");
    if (!g_occ.s) {
        PSK_HIP(hipStreamCreateWithFlags(&g_occ.s, hipStreamNonBlocking));
        PSK_HIP(hipMalloc(&g_occ.dw, 128 * sizeof(uint32_t)));
        PSK_HIP(hipHostMalloc(&g_occ.started, 64, hipHostMallocCoherent));
    }
    PSK_HIP(hipMemsetAsync(g_occ.dw, 0, 128 * sizeof(uint32_t), g_occ.s));
    PSK_HIP(hipStreamSynchronize(g_occ.s));
    *reinterpret_cast<volatile int64_t *>(g_occ.started) = 0;
    const uint64_t ticks = (uint64_t)(seconds * 1e8);
    hipLaunchKernelGGL(occupy_kernel, dim3((unsigned)wgs), dim3(1024), (size_t)lds_bytes, g_occ.s, g_occ.dw,
                       g_occ.started, ticks, reinterpret_cast<int32_t *>(g_occ.dw + 64));
    PSK_HIP(hipGetLastError());
    g_occ.active = true;
    // every occupier resident before the caller enqueues its solve (bounded: 5 s)
    const auto t0 = std::chrono::steady_clock::now();
    while (*reinterpret_cast<volatile int64_t *>(g_occ.started) < wgs &&
           std::chrono::steady_clock::now() - t0 < std::chrono::seconds(5)) {
    }
    const int64_t got = *reinterpret_cast<volatile int64_t *>(g_occ.started);
    return got >= wgs ? PSK_OK : fail(PSK_ERR_HIP, "psk_lab_occupy_begin: only " + std::to_string(got) + " of " +
                                                       std::to_string(wgs) + " occupiers started");
}

// releases the occupiers behind everything enqueued on the solver's stream so far, waits for them;
// *timed_out = 1 when they hit their time limit first (the solve could not finish while they held CUs)
extern "C" int psk_lab_occupy_end(int32_t *timed_out) {
    using namespace psk;
    Context *c;
    PSK_TRY(ctx(&c));
    if (!g_occ.active) return fail(PSK_ERR_ARG, "psk_lab_occupy_end: not active");
    hipLaunchKernelGGL(occupy_release_kernel, dim3(1), dim3(1), 0, c->stream, g_occ.dw);
    PSK_HIP(hipGetLastError());
    PSK_HIP(hipStreamSynchronize(g_occ.s));
    int32_t h = 0;
    PSK_HIP(hipMemcpy(&h, g_occ.dw + 64, sizeof(int32_t), hipMemcpyDeviceToHost));
    g_occ.active = false;
    if (timed_out) *timed_out = h;
    return PSK_OK;
}

// lab: `nwg` workgroups of 128 threads holding `lds_bytes` of LDS each, each spinning `usec` and recording
// (start, end, XCD) in s_memrealtime ticks — is a launch that needs its workgroups recycled dispatched
// beside the occupiers? (the grid schedule's progress test)
__global__ void dispatch_probe_kernel(uint64_t ticks, int64_t *rec) {
    extern __shared__ unsigned char dp_lds[];
    if (threadIdx.x == 0) {
        dp_lds[0] = 1;
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        uint64_t t = t0;
        while (t - t0 < ticks) {
            __builtin_amdgcn_s_sleep(4);
            t = __builtin_amdgcn_s_memrealtime();
        }
        rec[3 * blockIdx.x + 0] = (int64_t)t0;
        rec[3 * blockIdx.x + 1] = (int64_t)t;
        rec[3 * blockIdx.x + 2] = (int64_t)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u);
    }
}

extern "C" int psk_lab_dispatch_probe(int32_t nwg, int32_t lds_bytes, double usec, int64_t *rec_out) {
    using namespace psk;
    if (nwg < 1 || lds_bytes < 16 || lds_bytes > 160 * 1024 || usec < 0 || !rec_out)
        return fail(PSK_ERR_ARG, "psk_lab_dispatch_probe: bad arguments");
    Context *c;
    PSK_TRY(ctx(&c));
    int64_t *rec = nullptr;
    PSK_HIP(hipMalloc(&rec, (size_t)nwg * 3 * sizeof(int64_t)));
    hipLaunchKernelGGL(dispatch_probe_kernel, dim3((unsigned)nwg), dim3(128), (size_t)lds_bytes, c->stream,
                       (uint64_t)(usec * 100.0), rec);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(rec_out, rec, (size_t)nwg * 3 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(rec);   // (after the launch completed: the caller releases the occupiers afterwards)
    return e == hipSuccess ? PSK_OK : fail(PSK_ERR_HIP, hipGetErrorString(e));
}

// occupiers per XCD of the last psk_lab_occupy_begin (counts[8]; after psk_lab_occupy_end)
extern "C" int psk_lab_occupy_xcc(int32_t *counts) {
    using namespace psk;
    if (!counts || !g_occ.dw) return fail(PSK_ERR_ARG, "psk_lab_occupy_xcc: no occupiers yet");
    PSK_HIP(hipMemcpy(counts, g_occ.dw + 96, 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PSK_OK;
}

// workers (waves / 4) the last sync-free launch of a factor enrolled, and the grid it was launched with
extern "C" int psk_lab_trisolve_workers(const psk_prec *M, int32_t which, int32_t *enrolled, int32_t *grid) {
    using namespace psk;
    if (!M || M->kind != PSK_PREC_ILU) return fail(PSK_ERR_ARG, "psk_lab_trisolve_workers: not a triangular-solve chain");
    const TriFactor &T = which == 0 ? M->lo : M->up;
    if (!T.present || !T.sched) return fail(PSK_ERR_ARG, "psk_lab_trisolve_workers: factor absent");
    Context *c;
    PSK_TRY(ctx(&c));
    uint32_t v = 0;
    PSK_HIP(hipStreamSynchronize(c->stream));
    PSK_HIP(hipMemcpy(&v, T.sched + kSchedLast, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (enrolled) *enrolled = (int32_t)v;
    if (grid) *grid = syncfree_grid(c);
    return PSK_OK;
}

// the host planner's view of one factor (no GPU, no Context)
extern "C" int psk_lab_trisolve_plan(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                                     int32_t upper, int32_t unit, const int32_t *nat, int32_t num_cus,
                                     int64_t syncfree_waves, int32_t *schedule, double *est, int64_t *info) {
    using namespace psk;
    if (n < 0 || !rowptr || (rowptr[n] > 0 && (!colidx || !vals)) || num_cus < 1 || syncfree_waves < 1 || !schedule || !est || !info)
        return fail(PSK_ERR_ARG, "psk_lab_trisolve_plan: bad arguments");
    FactorPlan P;
    PSK_TRY(plan_factor(n, rowptr, colidx, vals, upper != 0, unit != 0,
                        nat ? std::vector<int32_t>(nat, nat + n) : std::vector<int32_t>(), num_cus, syncfree_waves, P));
    const TriFactor &T = P.T;
    *schedule = T.schedule;
    for (int i = 0; i < 6; ++i) est[i] = T.est_us[i];
    const int64_t v[8] = {T.levels, T.band.K, T.band.nblocks, T.band.ring_words, T.band.narrow ? 1 : 0,
                          T.grid.K, T.grid.dict_n, T.lv.steps};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    return PSK_OK;
}

// the host shard planner's view of one rank's block (no GPU, no Context): what psk_csr_create_dist plans and uploads
extern "C" int psk_lab_dist_plan(int64_t n_global, const int64_t *row_starts, int32_t P, int32_t rank,
                                 const int64_t *rowptr, const int32_t *colidx, int32_t *lcol, int64_t *halo,
                                 int64_t *nhalo, int32_t *pack, int64_t *npack, int64_t *peers, int32_t *npeers) {
    using namespace psk;
    if (!row_starts || !rowptr || P < 1 || rank < 0 || rank >= P || !lcol || !halo || !nhalo || !pack || !npack || !peers ||
        !npeers)
        return fail(PSK_ERR_ARG, "psk_lab_dist_plan: bad arguments");
    if (rowptr[row_starts[rank + 1] - row_starts[rank]] > rowptr[0] && !colidx)
        return fail(PSK_ERR_ARG, "psk_lab_dist_plan: NULL entries");
    DistPlan pl;
    PSK_TRY(dist_plan(n_global, row_starts, P, rank, rowptr, colidx, pl));
    std::vector<HaloPeer> hp;
    std::vector<int32_t> pk;
    dist_peers(pl, hp, pk);
    std::copy(pl.lcol.begin(), pl.lcol.end(), lcol);
    std::copy(pl.halo.begin(), pl.halo.end(), halo);
    std::copy(pk.begin(), pk.end(), pack);
    *nhalo = (int64_t)pl.halo.size();
    *npack = (int64_t)pk.size();
    *npeers = (int32_t)hp.size();
    for (size_t k = 0; k < hp.size(); ++k) {
        const HaloPeer &p = hp[k];
        const int64_t v[7] = {p.rank, p.send_count, p.send_begin, p.packed ? 1 : 0, p.pack_off, p.recv_count, p.recv_offset};
        std::copy(v, v + 7, peers + 7 * k);
    }
    return PSK_OK;
}

extern "C" int psk_lab_cheby_ab(const psk_prec *M, const double *v, int32_t reps, double *fused_ms, double *pieces_ms) {
    return psk::cheby_ab(M, v, reps, fused_ms, pieces_ms);
}

extern "C" int psk_lab_iluk_timing(double *out) {
    if (!out) return psk::fail(PSK_ERR_ARG, "psk_lab_iluk_timing: NULL argument");
    const psk::IlukTiming &t = psk::iluk_last_timing();
    const double v[7] = {t.symbolic_ms, (double)t.level, (double)t.rounds, (double)t.wide_rounds, (double)t.width,
                         (double)t.nnz_a, (double)t.nnz_p};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    return PSK_OK;
}

extern "C" int psk_lab_ilu0_timing(double *out) {
    if (!out) return psk::fail(PSK_ERR_ARG, "psk_lab_ilu0_timing: NULL argument");
    const psk::Ilu0Timing &t = psk::ilu0_last_timing();
    const double v[7] = {t.sort_ms, t.levels_ms, t.numeric_ms, t.split_ms, t.plan_ms, (double)t.levels, (double)t.width};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    return PSK_OK;
}

extern "C" int psk_lab_amg_gs_pair(psk_prec *M, int32_t set, int32_t *levels_on, int32_t *levels_eligible) {
    using namespace psk;
    if (set < -1 || set > 1) return fail(PSK_ERR_ARG, "psk_lab_amg_gs_pair: set must be -1, 0 or 1");
    Context *c;
    PSK_TRY(ctx(&c));
    PSK_HIP(hipStreamSynchronize(c->stream));   // queued applies keep the setting they were enqueued with
    int on = 0, el = 0;
    PSK_TRY(amg_gs_pair(M, set, &on, &el));
    if (levels_on) *levels_on = on;
    if (levels_eligible) *levels_eligible = el;
    return PSK_OK;
}

// the probe's writer: dst = src with 16-B accesses (the shape of K3 writing p_{k+1}, which the next SpMV gathers)
__global__ __launch_bounds__(256) void lab_copy_kernel(int64_t n, const double *__restrict__ src, double *__restrict__ dst) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i + 1 < n) {
        const double2 v = *reinterpret_cast<const double2 *>(src + i);
        *reinterpret_cast<double2 *>(dst + i) = v;
    } else if (i < n) {
        dst[i] = src[i];
    }
}

extern "C" int psk_lab_spmv_rotate(const psk_csr *A, const double *const *xs, double *const *ys, int32_t nbuf,
                                   int32_t reps, int32_t dot, double *avg_ms) {
    using namespace psk;
    if (!A || !xs || !ys || nbuf < 1 || reps < 1 || !avg_ms) return fail(PSK_ERR_ARG, "psk_lab_spmv_rotate: bad arguments");
    if (A->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_lab_spmv_rotate: sharded matrix");
    for (int32_t i = 0; i < nbuf; ++i)
        if (!xs[i] || !ys[i]) return fail(PSK_ERR_ARG, "psk_lab_spmv_rotate: NULL buffer");
    Context *c;
    PSK_TRY(ctx(&c));
    hipEvent_t e0, e1;
    PSK_HIP(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));
    PSK_HIP(hipEventCreateWithFlags(&e1, hipEventDisableSystemFence));
    const int mode = dot ? kSpmvDot : kSpmvPlain;
    DevBuf part;
    int rc = part.ensure(64);
    double *pp = dot ? part.as<double>() : nullptr;
    for (int32_t i = 0; i < nbuf && rc == PSK_OK; ++i)   // warm: every pair once
        rc = launch_spmv(A, mode, xs[i], ys[i], nullptr, nullptr, pp, nullptr, c->stream);
    if (rc == PSK_OK && hipEventRecord(e0, c->stream) != hipSuccess) rc = fail(PSK_ERR_HIP, "event record");
    for (int32_t r = 0; r < reps && rc == PSK_OK; ++r)
        rc = launch_spmv(A, mode, xs[r % nbuf], ys[r % nbuf], nullptr, nullptr, pp, nullptr, c->stream);
    if (rc == PSK_OK && hipEventRecord(e1, c->stream) != hipSuccess) rc = fail(PSK_ERR_HIP, "event record");
    float ms = 0.f;
    if (rc == PSK_OK && hipEventSynchronize(e1) != hipSuccess) rc = fail(PSK_ERR_HIP, "event sync");
    if (rc == PSK_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = fail(PSK_ERR_HIP, "event time");
    (void)hipStreamSynchronize(c->stream);   // before `part` is freed
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    part.release();
    if (rc == PSK_OK) *avg_ms = (double)ms / reps;
    return rc;
}

extern "C" int psk_lab_spmv_after_write(const psk_csr *A, double *x, double *y, const double *src, double *scratch,
                                        int32_t target, int32_t reps, int32_t dot, double *avg_ms) {
    using namespace psk;
    if (!A || !x || !y || !src || !scratch || reps < 1 || reps > 256 || !avg_ms)
        return fail(PSK_ERR_ARG, "psk_lab_spmv_after_write: bad arguments");
    if (A->comm || A->ncols != A->n) return fail(PSK_ERR_UNSUPPORTED, "psk_lab_spmv_after_write: square unsharded only");
    Context *c;
    PSK_TRY(ctx(&c));
    std::vector<hipEvent_t> ea((size_t)reps), eb((size_t)reps);
    for (int32_t r = 0; r < reps; ++r) {
        PSK_HIP(hipEventCreateWithFlags(&ea[(size_t)r], hipEventDisableSystemFence));
        PSK_HIP(hipEventCreateWithFlags(&eb[(size_t)r], hipEventDisableSystemFence));
    }
    const int mode = dot ? kSpmvDot : kSpmvPlain;
    DevBuf part;
    int rc = part.ensure(64);
    double *pp = dot ? part.as<double>() : nullptr;
    const int64_t n = A->n;
    const unsigned g = (unsigned)((n + 511) / 512);
    double *dst = target == 1 ? x : scratch;   // 1: the writer writes the SpMV's x (as K3 writes p); 2: another buffer
    rc = launch_spmv(A, mode, x, y, nullptr, nullptr, pp, nullptr, c->stream);   // warm
    for (int32_t r = 0; r < reps && rc == PSK_OK; ++r) {
        if (target > 0) {
            hipLaunchKernelGGL(lab_copy_kernel, dim3(g), dim3(256), 0, c->stream, n, src, dst);
            if (hipGetLastError() != hipSuccess) rc = fail(PSK_ERR_HIP, "lab copy");
        }
        if (rc == PSK_OK)
            rc = launch_spmv(A, mode, x, y, nullptr, nullptr, pp, nullptr, c->stream, ea[(size_t)r], eb[(size_t)r]);
    }
    double tot = 0.0;
    if (rc == PSK_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(PSK_ERR_HIP, "sync");
    for (int32_t r = 0; r < reps && rc == PSK_OK; ++r) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ea[(size_t)r], eb[(size_t)r]) != hipSuccess) rc = fail(PSK_ERR_HIP, "event time");
        tot += ms;
    }
    (void)hipStreamSynchronize(c->stream);
    for (int32_t r = 0; r < reps; ++r) {
        (void)hipEventDestroy(ea[(size_t)r]);
        (void)hipEventDestroy(eb[(size_t)r]);
    }
    part.release();
    if (rc == PSK_OK) *avg_ms = tot / reps;
    return rc;
}

// ---- the PCG loop's staggered x flush (pcg_state.hpp): its schedule as the kernels and the host read it (no GPU,
// no Context), and pcg_flush_kernel on caller-supplied vectors ----
extern "C" int psk_lab_pcg_stagger(int32_t *blocks, int32_t *ring) {
    if (blocks) *blocks = psk::kPcgStagger;
    if (ring) *ring = psk::kPcgDefer;
    return PSK_OK;
}

extern "C" int psk_lab_pcg_staggers(const psk_csr *A, const psk_prec *M, int32_t *on) {
    if (!A || !on) return psk::fail(PSK_ERR_ARG, "psk_lab_pcg_staggers: NULL argument");
    *on = psk::pcg_staggers(A, M) ? 1 : 0;
    return PSK_OK;
}

extern "C" int psk_lab_pcg_flush_schedule(int32_t S, int64_t nv, int64_t tile, int64_t k, int32_t in_spmv,
                                          int32_t *blk, int64_t *first_last) {
    using namespace psk;
    if (S < 1 || nv < 1 || tile < 0 || tile >= nv || k < 0 || !blk || !first_last)
        return fail(PSK_ERR_ARG, "psk_lab_pcg_flush_schedule: bad arguments");
    *blk = pcg_block_of_tile(tile, nv, S);
    const PcgPend pd = pcg_flush_pending(S, *blk, k, in_spmv != 0);
    first_last[0] = pd.first;
    first_last[1] = pd.last;
    return PSK_OK;
}

extern "C" int psk_lab_pcg_flush(int64_t n, int64_t k, int32_t stag, double *x, const double *ring,
                                 const double *alphas) {
    using namespace psk;
    if (n < 1 || k < 1 || !x || !ring || !alphas) return fail(PSK_ERR_ARG, "psk_lab_pcg_flush: bad arguments");
    if (stag && kPcgStagger == 0) return fail(PSK_ERR_UNSUPPORTED, "psk_lab_pcg_flush: built without the staggered flush");
    Context *c;
    PSK_TRY(ctx(&c));
    const size_t vec = ((size_t)n * 8 + 255) / 256 * 256, al = ((size_t)k * 8 + 255) / 256 * 256;
    DevBuf buf;
    PSK_TRY(buf.ensure((kPcgDefer + 1) * vec + al));
    char *d = buf.as<char>();
    double *dx = reinterpret_cast<double *>(d), *da = reinterpret_cast<double *>(d + (kPcgDefer + 1) * vec);
    PRing pr;
    for (int t = 0; t < kPcgDefer; ++t) pr.b[t] = reinterpret_cast<double *>(d + (size_t)(t + 1) * vec);
    int rc = PSK_OK;
    if (hipMemcpyAsync(dx, x, (size_t)n * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(da, alphas, (size_t)k * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        rc = fail(PSK_ERR_HIP, "psk_lab_pcg_flush: copy");
    for (int t = 0; t < kPcgDefer && rc == PSK_OK; ++t)
        if (hipMemcpyAsync(pr.b[t], ring + (size_t)t * (size_t)n, (size_t)n * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            rc = fail(PSK_ERR_HIP, "psk_lab_pcg_flush: copy");
    if (rc == PSK_OK) rc = launch_pcg_flush(n, dx, pr, da, k, stag != 0, c->stream);
    if (rc == PSK_OK && hipMemcpyAsync(x, dx, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = fail(PSK_ERR_HIP, "psk_lab_pcg_flush: copy back");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == PSK_OK) rc = fail(PSK_ERR_HIP, "psk_lab_pcg_flush: sync");
    buf.release();
    return rc;
}

// ---- psk_pcg's workspace after a solve (pcg.hip pcg_work_view): what K0 .. K3 and the flush left in HBM ----
extern "C" int psk_lab_pcg_internals(const psk_csr *A, int64_t maxiter, int32_t gen, int32_t own_x, double *r,
                                     double *ring, double *Ap, double *u, double *x, double *alphas, double *udr,
                                     double *hist, double *sums, double *state) {
    using namespace psk;
    if (!A) return fail(PSK_ERR_ARG, "psk_lab_pcg_internals: bad arguments");
    PcgView v;
    PSK_TRY(pcg_work_view(const_cast<psk_csr *>(A), maxiter, gen != 0, own_x != 0, false, &v));
    Context *c;
    PSK_TRY(ctx(&c));
    PSK_HIP(hipStreamSynchronize(c->stream));
    const size_t vec = (size_t)v.n * 8, vecc = (size_t)v.ncols * 8, it = (size_t)(maxiter + 1) * 8;
    if (r && vec) PSK_HIP(hipMemcpy(r, v.r, vec, hipMemcpyDeviceToHost));
    if (Ap && vec) PSK_HIP(hipMemcpy(Ap, v.Ap, vec, hipMemcpyDeviceToHost));
    if (u && v.u && vec) PSK_HIP(hipMemcpy(u, v.u, vec, hipMemcpyDeviceToHost));
    if (x && v.x && vec) PSK_HIP(hipMemcpy(x, v.x, vec, hipMemcpyDeviceToHost));
    for (int t = 0; t < kPcgDefer; ++t)
        if (ring && v.ring[t] && vecc)
            PSK_HIP(hipMemcpy(ring + (size_t)t * (size_t)v.ncols, v.ring[t], vecc, hipMemcpyDeviceToHost));
    if (alphas) PSK_HIP(hipMemcpy(alphas, v.alphas, it, hipMemcpyDeviceToHost));
    if (udr) PSK_HIP(hipMemcpy(udr, v.udr, it, hipMemcpyDeviceToHost));
    if (hist) PSK_HIP(hipMemcpy(hist, v.hist, it, hipMemcpyDeviceToHost));
    if (sums) {
        PSK_HIP(hipMemcpy(&sums[0], v.part1, 8, hipMemcpyDeviceToHost));
        PSK_HIP(hipMemcpy(&sums[1], v.part2, 8, hipMemcpyDeviceToHost));
        // u.r: K2 fuses it on the Jacobi / identity paths; the general path's is pcg_dot_kernel's (part3)
        PSK_HIP(hipMemcpy(&sums[2], gen ? v.part3 : v.part2 + 1, 8, hipMemcpyDeviceToHost));
    }
    if (state) {
        PcgState hs;
        PSK_HIP(hipMemcpy(&hs, v.st, sizeof(hs), hipMemcpyDeviceToHost));
        state[0] = (double)hs.done;
        state[1] = (double)hs.brk_kind;
        state[2] = (double)hs.iters;
        state[3] = hs.resid;
        state[4] = hs.normB;
        state[5] = hs.tauNormB;
        state[6] = (double)hs.live;
        state[7] = (double)hs.x_written;
    }
    return PSK_OK;
}

// psk_pcg clears none of its vectors or scalar arrays (each entry is written before it is read): a test of what the
// kernels leave untouched sets both buffers to a known byte first, sized as the solve will size them, so the solve
// keeps them
extern "C" int psk_lab_pcg_prefill(psk_csr *A, int64_t maxiter, int32_t gen, int32_t own_x, int32_t byte) {
    using namespace psk;
    if (!A || byte < 0 || byte > 255) return fail(PSK_ERR_ARG, "psk_lab_pcg_prefill: bad arguments");
    Context *c;
    PSK_TRY(ctx(&c));
    PSK_HIP(hipStreamSynchronize(c->stream));   // a solve still queued on this matrix keeps its workspace
    PcgView v;
    PSK_TRY(pcg_work_view(A, maxiter, gen != 0, own_x != 0, true, &v));
    PSK_HIP(hipMemsetAsync(v.big, byte, v.big_bytes, c->stream));
    PSK_HIP(hipMemsetAsync(v.small, byte, v.small_bytes, c->stream));
    PSK_HIP(hipStreamSynchronize(c->stream));
    return PSK_OK;
}

// ---- the solvers' workspace layouts (solve_loop.hpp Carve) on null-based carvers: no GPU, no Context ----
extern "C" int psk_lab_solver_layout(int32_t solver, int64_t n, int64_t ncols, int64_t maxiter, int64_t restart,
                                     int32_t flags, int32_t P, int64_t *offsets, int32_t *count, int64_t *bytes) {
    using namespace psk;
    if (n < 0 || ncols < 0 || maxiter < 0 || restart < 0 || P < 1 || !offsets || !count || !bytes)
        return fail(PSK_ERR_ARG, "psk_lab_solver_layout: bad arguments");
    std::vector<int64_t> log;
    const bool gen = (flags & PSK_LAB_LAYOUT_GEN) != 0;
    if (solver == PSK_LAB_SOLVER_PCG) pcg_layout_probe(n, ncols, maxiter, gen, (flags & PSK_LAB_LAYOUT_OWN_X) != 0, P, &log, bytes);
    else if (solver == PSK_LAB_SOLVER_GMRES) gmres_layout_probe(n, maxiter, restart, gen, &log, bytes);
    else if (solver == PSK_LAB_SOLVER_BICGSTAB) bicgstab_layout_probe(n, maxiter, gen, &log, bytes);
    else if (solver == PSK_LAB_SOLVER_MINRES) minres_layout_probe(n, maxiter, gen, &log, bytes);
    else if (solver == PSK_LAB_SOLVER_PCG_MULTI && P <= PSK_PCG_MULTI_MAX) pcg_multi_layout_probe(n, maxiter, P, &log, bytes);
    else if (solver == PSK_LAB_SOLVER_VCYCLE) vcycle_layout_probe(n, maxiter, (flags & PSK_LAB_LAYOUT_DEV_IO) != 0, &log, bytes);
    else return fail(PSK_ERR_ARG, "psk_lab_solver_layout: unknown solver");
    if ((size_t)*count < log.size()) return fail(PSK_ERR_ARG, "psk_lab_solver_layout: offsets too short");
    *count = (int32_t)log.size();
    for (size_t i = 0; i < log.size(); ++i) offsets[i] = log[i];
    return PSK_OK;
}

// ---- psk_pcg_multi's workspace after a solve (pcg_multi.hip pcg_multi_work_view) ----
extern "C" int psk_lab_pcg_multi_internals(const psk_csr *A, int64_t maxiter, int32_t nrhs, double *alphas, double *udr,
                                           double *pap, double *r, double *p, double *Ap, double *x, double *state) {
    using namespace psk;
    if (!A || A->comm) return fail(PSK_ERR_ARG, "psk_lab_pcg_multi_internals: bad arguments");
    PcgMultiView v;
    PSK_TRY(pcg_multi_work_view(const_cast<psk_csr *>(A), maxiter, nrhs, &v));
    Context *c;
    PSK_TRY(ctx(&c));
    PSK_HIP(hipStreamSynchronize(c->stream));
    const size_t vec = (size_t)v.n * (size_t)v.kp * 8, it = (size_t)v.ld * 8;
    const struct {
        double *dst;
        const double *src;
    } vecs[4] = {{r, v.r}, {p, v.p}, {Ap, v.Ap}, {x, v.x}}, its[3] = {{alphas, v.alphas}, {udr, v.udrs}, {pap, v.paps}};
    for (const auto &q : vecs)
        if (q.dst && vec) PSK_HIP(hipMemcpy(q.dst, q.src, vec, hipMemcpyDeviceToHost));
    for (const auto &q : its)
        for (int j = 0; q.dst && j < nrhs; ++j)
            PSK_HIP(hipMemcpy(q.dst + (size_t)j * (size_t)v.ld, q.src + (size_t)j * (size_t)v.ld, it, hipMemcpyDeviceToHost));
    if (state) {
        std::vector<char> hs(pcg_multi_state_bytes());
        PSK_HIP(hipMemcpy(hs.data(), v.state, hs.size(), hipMemcpyDeviceToHost));
        for (int j = 0; j < nrhs; ++j) pcg_multi_col_state(hs.data(), j, state + (size_t)j * kMultiStateWords);
    }
    return PSK_OK;
}

// ---- psk_gmres's workspace after a solve (gmres.hip gmres_work_view): what the Arnoldi kernels left in HBM ----
extern "C" int psk_lab_gmres_internals(const psk_csr *A, int64_t maxiter, int32_t restart, int32_t gen, int32_t cols,
                                       double *Q, double *H, double *R, double *CS, double *g, double *y,
                                       double *state) {
    using namespace psk;
    if (!A || cols < 0) return fail(PSK_ERR_ARG, "psk_lab_gmres_internals: bad arguments");
    GmresView v;
    PSK_TRY(gmres_work_view(const_cast<psk_csr *>(A), maxiter, restart, gen != 0, false, &v));
    if (cols > v.K + 1) return fail(PSK_ERR_ARG, "psk_lab_gmres_internals: more columns than the basis holds");
    Context *c;
    PSK_TRY(ctx(&c));
    PSK_HIP(hipStreamSynchronize(c->stream));
    const size_t K = (size_t)v.K, ld = K + 1;
    if (Q && cols > 0 && v.n > 0)   // n x cols, the padded column stride removed
        PSK_HIP(hipMemcpy2D(Q, (size_t)v.n * 8, v.Q, (size_t)v.ldq * 8, (size_t)v.n * 8, (size_t)cols,
                            hipMemcpyDeviceToHost));
    if (H) PSK_HIP(hipMemcpy(H, v.H, ld * K * 8, hipMemcpyDeviceToHost));
    if (R) PSK_HIP(hipMemcpy(R, v.R, ld * K * 8, hipMemcpyDeviceToHost));
    if (CS) PSK_HIP(hipMemcpy(CS, v.CS, 2 * K * 8, hipMemcpyDeviceToHost));
    if (g) PSK_HIP(hipMemcpy(g, v.g, ld * 8, hipMemcpyDeviceToHost));
    if (y) PSK_HIP(hipMemcpy(y, v.dy, ld * 8, hipMemcpyDeviceToHost));
    if (state) {
        int32_t iv[3];
        PSK_HIP(hipMemcpy(&iv[0], v.done, 4, hipMemcpyDeviceToHost));
        PSK_HIP(hipMemcpy(&iv[1], v.brk, 4, hipMemcpyDeviceToHost));
        PSK_HIP(hipMemcpy(&iv[2], v.kconv, 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < 3; ++i) state[i] = (double)iv[i];
        PSK_HIP(hipMemcpy(&state[3], v.normB, 8, hipMemcpyDeviceToHost));
        PSK_HIP(hipMemcpy(&state[4], v.tauNormB, 8, hipMemcpyDeviceToHost));
        PSK_HIP(hipMemcpy(&state[5], v.rec, 8, hipMemcpyDeviceToHost));
    }
    return PSK_OK;
}

// psk_gmres does not clear its basis or its rotations (each is written before it is read): a test of what the kernels
// leave untouched sets both buffers to a known byte first, sized as the solve will size them, so the solve keeps them
extern "C" int psk_lab_gmres_prefill(psk_csr *A, int64_t maxiter, int32_t restart, int32_t gen, int32_t byte) {
    using namespace psk;
    if (!A || byte < 0 || byte > 255) return fail(PSK_ERR_ARG, "psk_lab_gmres_prefill: bad arguments");
    Context *c;
    PSK_TRY(ctx(&c));
    PSK_HIP(hipStreamSynchronize(c->stream));   // a solve still queued on this matrix keeps its workspace
    GmresView v;
    PSK_TRY(gmres_work_view(A, maxiter, restart, gen != 0, true, &v));
    PSK_HIP(hipMemsetAsync(v.big, byte, v.big_bytes, c->stream));
    PSK_HIP(hipMemsetAsync(v.small, byte, v.small_bytes, c->stream));
    PSK_HIP(hipStreamSynchronize(c->stream));
    return PSK_OK;
}
