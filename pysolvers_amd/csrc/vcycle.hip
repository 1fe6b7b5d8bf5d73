// vcycle.hip — the standalone AMG V-cycle solver, AMGVCycleSolver.solve (VCycleSolver.py:52-95), as a device loop:
//     normB = ||b||;  if normB == 0: return x = 0 (iters 1)
//     x = copy(b)                                      (:69; PSK_VCYCLE_X0_GIVEN: the caller's x instead)
//     for k < maxiter:  x = runCycle(b, x);  r = b - A x;  normR = ||r||;  reportIter(k, normR)
//                       if normR < tau normB: return handleConvergence(k, x)        (strict, :90)
//     return handleMaxiter(maxiter - 1, x)
// The cycle is the preconditioner's (amg.hip amg_cycle: the same launches amg_apply enqueues), and so are the
// residual SpMV with its in-launch sum and the ||b||^2 pass. Per cycle the solver adds that SpMV and ONE launch,
// vc_check_kernel: the test, the snapshot of x when this cycle is the first to converge (or the last of
// maxiter), the history entry and the host-mapped done word.
//
// The host never drains the queue: it enqueues cycle after cycle, records an event every `check_every` cycles
// and reads the done word behind an event kVcLag chunks back (solve_loop.hpp StampPoll). By default (check_every 1,
// kVcLag 1) at most one cycle past the converging one is enqueued; cycles that run after it find conv_iter >= 0
// and change neither the output, the history nor the state, so the results do not depend on the lag.
#include "amg.hpp"
#include "pcg_state.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

namespace psk {

// the loop state (device; copied to the host once, after the loop)
struct VcState {
    int64_t conv_iter;   // -1 while running; k of the first cycle whose test held
    int64_t nhist;       // history entries written
    double resid;        // the latest reported ||b - A x||
    double normB;
    int64_t pad[4];
};
constexpr int kVcStateWords = (int)(sizeof(VcState) / 8);
static_assert(sizeof(VcState) == 64, "VcState");

// vc_check_kernel's tickets (the project's pattern: psk_internal.hpp gridsum, one counter per 256-B line): block
// b draws on counter b % kVcGroups, the block holding a group's last ticket draws on the final counter, and the
// holder of ITS last ticket is the last block of the launch. One word takes ~88 atomics/us; 16,384 blocks (n =
// 4.2M) on one word would cost more than the three small launches this kernel replaces.
constexpr int kVcGroups = 64, kVcTickStride = 64;
constexpr size_t kVcTickBytes = (size_t)(kVcGroups + 1) * kVcTickStride * sizeof(uint32_t);
constexpr int kVcLag = 1;

__device__ __forceinline__ int64_t vc_load(const void *p) {
    return (int64_t)__hip_atomic_load(reinterpret_cast<const uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// after ||b||^2 (amg_loop_start): the state, and the done stamp 1 when b = 0 (no cycle runs, :64-65)
__global__ void vc_init_kernel(const double *bb, VcState *st, int64_t *hdone, int64_t hgen) {
    const double normB = sqrt(bb[0]);   // self.norm(b)  :63
    st->conv_iter = -1;
    st->nhist = 0;
    st->resid = 0.0;
    st->normB = normB;
    if (normB == 0.0) done_stamp_store(hdone, hgen, 1);
}

// After cycle k and r = b - A x (sum = ||r||^2, published by the SpMV's launch). Every block reads the same words
// — the sum and the state as the PREVIOUS launch left it — and evaluates the same predicate; nothing a block of
// this launch writes is read by another: the state is read before the block's ticket is drawn and written only by
// the holder of the launch's last ticket, which every other block's reads precede.
__global__ __launch_bounds__(kBlock) void vc_check_kernel(int64_t n, const double *__restrict__ x,
                                                          double *__restrict__ out, const double *sum, double tau,
                                                          VcState *st, uint32_t *tick, double *hist, int64_t k,
                                                          int64_t maxiter, int64_t *hdone, int64_t hgen) {
    const bool running = vc_load(&st->conv_iter) < 0;
    const double normB = __longlong_as_double(vc_load(&st->normB));
    const double normR = sqrt(__longlong_as_double(vc_load(sum)));   // self.norm(r)  :87
    const bool hit = running && normR < tau * normB;                // :90 (strict)
    // the returned x: the first converging cycle's (:91), else the last iterate (handleMaxiter, :95)
    if (running && (hit || k == maxiter - 1)) {
        const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (i < n) out[i] = x[i];
    }
    __syncthreads();   // every thread's state reads have returned (their values chose the branch above)
    if (threadIdx.x != 0) return;
    __builtin_amdgcn_s_waitcnt(0);   // ... before the ticket is issued
    const uint32_t nb = gridDim.x, g = blockIdx.x % kVcGroups;
    const uint32_t members = (nb - g + kVcGroups - 1) / kVcGroups, ngroups = nb < kVcGroups ? nb : kVcGroups;
    uint32_t *cg = tick + (size_t)g * kVcTickStride, *cf = tick + (size_t)kVcGroups * kVcTickStride;
    if (__hip_atomic_fetch_add(cg, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != members - 1) return;
    __hip_atomic_store(cg, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_fetch_add(cf, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ngroups - 1) return;
    __hip_atomic_store(cf, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!running) return;   // a cycle enqueued past the converging one: nothing changes
    hist[k] = normR;        // reportIter(k, normR, normB)  :89
    st->nhist = k + 1;
    st->resid = normR;
    if (hit) {
        st->conv_iter = k;
        done_stamp_store(hdone, hgen, k + 2);
    }
}

// the loop's device words: [state][hist maxiter][tickets], then b and the output when they are the host's. The
// history follows the state unaligned: the final host copy reads both as one contiguous range.
struct VcWork {
    VcState *st;
    double *hist, *b, *out;
    uint32_t *tick;
};
static void vc_layout(Carve &cv, int64_t n, int64_t maxiter, bool dev_io, VcWork &w) {
    w.st = cv.take<VcState>(sizeof(VcState), 8);
    w.hist = cv.take<double>((size_t)maxiter * 8, 8);
    w.tick = cv.take<uint32_t>(kVcTickBytes);
    w.b = dev_io ? nullptr : cv.take<double>((size_t)n * 8);
    w.out = dev_io ? nullptr : cv.take<double>((size_t)n * 8);
}
void vcycle_layout_probe(int64_t n, int64_t maxiter, bool dev_io, std::vector<int64_t> *log, int64_t *bytes) {
    Carve cv;
    cv.log = log;
    VcWork w;
    vc_layout(cv, n, maxiter, dev_io, w);
    bytes[0] = (int64_t)cv.off;
    bytes[1] = 0;
}

// what the phases of one solve share
struct VcRun {
    const psk_prec *M;
    const psk_ctl *ctl;
    Context *c;
    hipStream_t s;
    int64_t n, maxiter;
    bool dev_io;        // b and x are the caller's device vectors
    int32_t flags;
    AmgLoop lp;
    VcWork w;
    SolveKit *kit;
    double *out;        // where vc_check_kernel snapshots x: the caller's device vector, or w.out
    const double *bd;   // b on the device
};

static int vc_workspace(VcRun &r, double *xout) {
    PSK_TRY(amg_loop_view(r.M, &r.lp));
    int64_t need[2];
    vcycle_layout_probe(r.n, r.maxiter, r.dev_io, nullptr, need);
    PSK_TRY(r.lp.work->ensure((size_t)need[0]));
    Carve cv{r.lp.work->as<char>()};
    vc_layout(cv, r.n, r.maxiter, r.dev_io, r.w);
    r.out = r.dev_io ? xout : r.w.out;
    return PSK_OK;
}

// in front of the loop: b, ||b||^2 and x = copy(b) (or the caller's x), the state; the one wait, which tells
// whether b = 0 (*zero_b: no cycle runs, :64-65)
static int vc_init(VcRun &r, StampPoll &poll, const double *b, const double *xout, int32_t loc, bool *zero_b) {
    hipStream_t s = r.s;
    r.bd = b;
    if (!r.dev_io) {
        PSK_TRY(to_device_vec(b, loc, r.n, r.w.b, s));
        r.bd = r.w.b;
    }
    PSK_HIP(hipEventRecord(r.kit->ev0, s));
    PSK_TRY(amg_loop_start(r.M, r.c, r.bd, s));                                              // ||b||^2, x = copy(b)  :63, :69
    if (r.flags & PSK_VCYCLE_X0_GIVEN) PSK_TRY(to_device_vec(xout, loc, r.n, r.lp.x, s));   // before `out` is written
    PSK_HIP(hipMemsetAsync(r.w.tick, 0, kVcTickBytes, s));
    hipLaunchKernelGGL(vc_init_kernel, dim3(1), dim3(1), 0, s, r.lp.normb2, r.w.st, poll.hdone(), poll.hgen());
    PSK_HIP(hipGetLastError());
    PSK_TRY(poll.wait(s));
    *zero_b = poll.stamp() == 1;
    return PSK_OK;
}

// cycle k, its residual and its check
static int vc_iteration(VcRun &r, const StampPoll &poll, int64_t k) {
    PSK_TRY(amg_cycle(r.M, r.c, r.bd, r.s));      // x = runCycle(b, x)  :81
    PSK_TRY(amg_residual(r.M, r.bd, r.s));        // r = b - A x, ||r||^2 in the same launch  :84, :87
    const dim3 gc((unsigned)((r.n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(vc_check_kernel, gc, dim3(kBlock), 0, r.s, r.n, r.lp.x, r.out, r.lp.sum, r.ctl->tau, r.w.st, r.w.tick,
                       r.w.hist, k, r.maxiter, poll.hdone(), poll.hgen());
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// behind the loop: one copy for the state and the `launched` history entries (into host), the gridsum error word,
// x; one synchronisation; then the two error checks and loop_ms
static int vc_finish(VcRun &r, int64_t launched, bool zero_b, double *xout, int32_t loc, std::vector<double> &host,
                     psk_result *res) {
    hipStream_t s = r.s;
    PSK_HIP(hipEventRecord(r.kit->ev1, s));
    host.resize((size_t)(kVcStateWords + launched));
    int32_t *gs_word = reinterpret_cast<int32_t *>(static_cast<char *>(r.kit->hstage) + kStageBytes - 64);
    PSK_TRY(gridsum_check_enqueue(r.c, gs_word));
    PSK_HIP(hipMemcpyAsync(host.data(), r.w.st, host.size() * 8, hipMemcpyDeviceToHost, s));
    if (zero_b) PSK_HIP(hipMemsetAsync(r.out, 0, (size_t)r.n * 8, s));   // np.zeros_like(b)  :65
    if (!r.dev_io) PSK_TRY(from_device_vec(r.out, loc, r.n, xout, s));
    PSK_HIP(hipStreamSynchronize(s));
    PSK_TRY(gridsum_check_result(r.c, *gs_word));
    PSK_TRY(prec_check_error(r.M, s));
    res->loop_ms = loop_ms(r.kit);
    return PSK_OK;
}

// host = [state][history] of a loop that enqueued `launched` cycles, decoded into res and hist
static int vc_report(const VcRun &r, int64_t launched, bool zero_b, const std::vector<double> &host, psk_result *res,
                     double *hist) {
    VcState hs;
    std::memcpy(&hs, host.data(), sizeof(VcState));
    res->norm_b = hs.normB;
    res->spmv_launches = launched;
    if (zero_b) {                       // handleConvergence(0, zeros, 0, 0)
        result_trivial(res);
        return PSK_OK;
    }
    const int64_t nh = hs.nhist < launched ? hs.nhist : launched;
    res->hist_len = nh;
    res->resid = res->resid_recursive = hs.resid;
    if (hist && nh > 0) std::memcpy(hist, host.data() + kVcStateWords, (size_t)nh * 8);
    if (hs.conv_iter >= 0) {            // handleConvergence(k, x, normR, normB)  :91
        res->status = PSK_CONVERGED;
        res->success = 1;
        res->iters = hs.conv_iter + 1;
        res->exit = PSK_EXIT_TOLERANCE;
    } else {                            // handleMaxiter(maxiter - 1, x, normR, normB)  :95
        if (launched != r.maxiter) return fail(PSK_ERR_HIP, "psk_vcycle: the loop stopped without a converged cycle");
        res->status = PSK_MAXITER;
        res->success = r.ctl->fail_on_maxiter ? 0 : 1;
        res->iters = r.maxiter - 1;
        res->exit = PSK_EXIT_MAXITER;
        if (r.ctl->fail_on_maxiter) result_msg(res, "failure to converge");
    }
    return PSK_OK;
}

// the phases in order; the caller drains the stream when one fails
static int vc_solve(VcRun &r, const double *b, double *xout, psk_result *res, double *hist, int32_t loc) {
    PSK_TRY(vc_workspace(r, xout));
    PSK_TRY(solve_kit(r.c, false, &r.kit));
    StampPoll poll(r.kit);   // the host-mapped done stamp vc_init_kernel and vc_check_kernel write
    bool zero_b;
    PSK_TRY(vc_init(r, poll, b, xout, loc, &zero_b));
    const int C = r.ctl->check_every > 0 ? r.ctl->check_every : 1;
    int64_t launched = 0;
    for (int64_t k = 0; k < r.maxiter && !zero_b; ++k) {
        bool stop;
        PSK_TRY(poll.step<kVcLag>(k, C, r.s, &stop));
        if (stop) break;
        PSK_TRY(vc_iteration(r, poll, k));
        launched = k + 1;
    }
    std::vector<double> host;
    PSK_TRY(vc_finish(r, launched, zero_b, xout, loc, host, res));
    return vc_report(r, launched, zero_b, host, res, hist);
}

}  // namespace psk

using namespace psk;

extern "C" int psk_vcycle(const psk_prec *M, const double *b, double *xout, const psk_ctl *ctl, psk_result *res,
                          double *hist, int32_t flags, int32_t loc) {
    if (!M || !b || !xout || !ctl || !res) return fail(PSK_ERR_ARG, "psk_vcycle: NULL argument");
    if (M->kind != PSK_PREC_AMG || !M->amg) return fail(PSK_ERR_ARG, "psk_vcycle: not an AMG preconditioner");
    if (ctl->maxiter <= 0) return fail(PSK_ERR_ARG, "psk_vcycle: maxiter <= 0");   // the reference: NameError (:95)
    if (flags & ~PSK_VCYCLE_X0_GIVEN) return fail(PSK_ERR_ARG, "psk_vcycle: unknown flags");
    if (loc != PSK_HOST && loc != PSK_DEVICE) return fail(PSK_ERR_ARG, "psk_vcycle: bad loc");
    VcRun r{};
    r.M = M;
    r.ctl = ctl;
    PSK_TRY(ctx(&r.c));
    std::lock_guard<std::mutex> solve_lock(r.c->solve_mu);
    r.s = r.c->stream;
    std::memset(res, 0, sizeof(*res));
    r.n = M->n;
    r.maxiter = ctl->maxiter;
    r.dev_io = loc == PSK_DEVICE;
    r.flags = flags;
    if (r.n == 0) {   // ||b|| = 0
        result_trivial(res);
        return PSK_OK;
    }
    const int rc = vc_solve(r, b, xout, res, hist, loc);
    // a solve that failed on the host side leaves no kernel of its own running behind the next solve
    if (rc != PSK_OK) (void)hipStreamSynchronize(r.s);
    return rc;
}

