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

static void vc_msg(psk_result *res, const char *m) { std::snprintf(res->msg, sizeof(res->msg), "%s", m); }

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

}  // namespace psk

using namespace psk;

extern "C" int psk_vcycle(const psk_prec *M, const double *b, double *xout, const psk_ctl *ctl, psk_result *res,
                          double *hist, int32_t flags, int32_t loc) {
    if (!M || !b || !xout || !ctl || !res) return fail(PSK_ERR_ARG, "psk_vcycle: NULL argument");
    if (M->kind != PSK_PREC_AMG || !M->amg) return fail(PSK_ERR_ARG, "psk_vcycle: not an AMG preconditioner");
    if (ctl->maxiter <= 0) return fail(PSK_ERR_ARG, "psk_vcycle: maxiter <= 0");   // the reference: NameError (:95)
    if (flags & ~PSK_VCYCLE_X0_GIVEN) return fail(PSK_ERR_ARG, "psk_vcycle: unknown flags");
    if (loc != PSK_HOST && loc != PSK_DEVICE) return fail(PSK_ERR_ARG, "psk_vcycle: bad loc");
    Context *c;
    PSK_TRY(ctx(&c));
    std::lock_guard<std::mutex> solve_lock(c->solve_mu);
    hipStream_t s = c->stream;
    std::memset(res, 0, sizeof(*res));
    const int64_t n = M->n, maxiter = ctl->maxiter;
    if (n == 0) {   // ||b|| = 0
        res->status = PSK_CONVERGED;
        res->success = 1;
        res->iters = 1;
        res->exit = PSK_EXIT_NONE;
        return PSK_OK;
    }
    AmgLoop lp;
    PSK_TRY(amg_loop_view(M, &lp));
    const bool dev_io = loc == PSK_DEVICE;
    int64_t need[2];
    vcycle_layout_probe(n, maxiter, dev_io, nullptr, need);
    PSK_TRY(lp.work->ensure((size_t)need[0]));
    Carve cv{lp.work->as<char>()};
    VcWork w;
    vc_layout(cv, n, maxiter, dev_io, w);
    VcState *st = w.st;
    double *dhist = w.hist, *out = dev_io ? xout : w.out;
    uint32_t *tick = w.tick;
    SolveKit *kit;
    PSK_TRY(solve_kit(c, false, &kit));
    StampPoll poll(kit);

    int rc = PSK_OK;
    auto body = [&]() -> int {
        const double *bd = b;
        if (!dev_io) {
            PSK_TRY(to_device_vec(b, loc, n, w.b, s));
            bd = w.b;
        }
        PSK_HIP(hipEventRecord(kit->ev0, s));
        PSK_TRY(amg_loop_start(M, c, bd, s));                                            // ||b||^2, x = copy(b)  :63, :69
        if (flags & PSK_VCYCLE_X0_GIVEN) PSK_TRY(to_device_vec(xout, loc, n, lp.x, s));   // before `out` is written
        PSK_HIP(hipMemsetAsync(tick, 0, kVcTickBytes, s));
        hipLaunchKernelGGL(vc_init_kernel, dim3(1), dim3(1), 0, s, lp.normb2, st, poll.hdone(), poll.hgen());
        PSK_HIP(hipGetLastError());
        // the one wait in front of the loop: b = 0 runs no cycle (:64-65)
        PSK_TRY(poll.wait(s));
        const bool zero_b = poll.stamp() == 1;
        const int C = ctl->check_every > 0 ? ctl->check_every : 1;
        const dim3 gc((unsigned)((n + kBlock - 1) / kBlock));
        int64_t launched = 0;
        for (int64_t k = 0; k < maxiter && !zero_b; ++k) {
            bool stop;
            PSK_TRY(poll.step<kVcLag>(k, C, s, &stop));
            if (stop) break;
            PSK_TRY(amg_cycle(M, c, bd, s));      // x = runCycle(b, x)  :81
            PSK_TRY(amg_residual(M, bd, s));      // r = b - A x, ||r||^2 in the same launch  :84, :87
            hipLaunchKernelGGL(vc_check_kernel, gc, dim3(kBlock), 0, s, n, lp.x, out, lp.sum, ctl->tau, st, tick, dhist, k,
                               maxiter, poll.hdone(), poll.hgen());
            PSK_HIP(hipGetLastError());
            launched = k + 1;
        }
        PSK_HIP(hipEventRecord(kit->ev1, s));
        // one copy for the state and the history, the gridsum error word, x; one synchronisation
        std::vector<double> host((size_t)(kVcStateWords + launched));
        int32_t *gs_word = reinterpret_cast<int32_t *>(static_cast<char *>(kit->hstage) + kStageBytes - 64);
        PSK_TRY(gridsum_check_enqueue(c, gs_word));
        PSK_HIP(hipMemcpyAsync(host.data(), st, host.size() * 8, hipMemcpyDeviceToHost, s));
        if (zero_b) PSK_HIP(hipMemsetAsync(out, 0, (size_t)n * 8, s));   // np.zeros_like(b)  :65
        if (!dev_io) PSK_TRY(from_device_vec(out, loc, n, xout, s));
        PSK_HIP(hipStreamSynchronize(s));
        PSK_TRY(gridsum_check_result(c, *gs_word));
        PSK_TRY(prec_check_error(M, s));
        VcState hs;
        std::memcpy(&hs, host.data(), sizeof(VcState));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, kit->ev0, kit->ev1);
        res->loop_ms = ms;
        res->norm_b = hs.normB;
        res->spmv_launches = launched;
        if (zero_b) {                       // handleConvergence(0, zeros, 0, 0)
            res->status = PSK_CONVERGED;
            res->success = 1;
            res->iters = 1;
            res->exit = PSK_EXIT_NONE;
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
            if (launched != maxiter) return fail(PSK_ERR_HIP, "psk_vcycle: the loop stopped without a converged cycle");
            res->status = PSK_MAXITER;
            res->success = ctl->fail_on_maxiter ? 0 : 1;
            res->iters = maxiter - 1;
            res->exit = PSK_EXIT_MAXITER;
            if (ctl->fail_on_maxiter) vc_msg(res, "failure to converge");
        }
        return PSK_OK;
    };
    rc = body();
    // a solve that failed on the host side leaves no kernel of its own running behind the next solve
    if (rc != PSK_OK) (void)hipStreamSynchronize(s);
    return rc;
}
