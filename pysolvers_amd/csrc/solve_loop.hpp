// solve_loop.hpp — host-side helpers of the device-loop solvers (psk_pcg, psk_bicgstab, psk_minres, psk_gmres, psk_vcycle,
// psk_pcg_multi): the workspace carver, the done-stamp poll, the psk_result lines they all write alike, and the frame
// psk_bicgstab, psk_minres, psk_gmres and psk_pcg_multi share (SolveRun, solve_entry, workspace_carve, poll_loop,
// solve_finish, the result_* functions). Host code only: no kernel lives here (the kernels' side of the stamp is
// done_stamp_store, psk_internal.hpp).
#pragma once
#include "psk_internal.hpp"
#include "dist.hpp"   // solve_entry reads the matrix's communicator

#include <cmath>
#include <cstdio>
#include <cstring>

namespace psk {

// Bump carver of one DevBuf. A solver's layout function fills its pointer struct from a Carve: once on a null base
// (every pointer null, `off` = the bytes DevBuf::ensure needs) and once on the buffer, so the size and the pointers
// come from the same code. take(): the start aligned to `align`, the extent rounded up to it.
struct Carve {
    char *base = nullptr;
    size_t off = 0;
    std::vector<int64_t> *log = nullptr;   // every take's offset, in order (psk_lab_solver_layout)
    template <class T> T *take(size_t bytes, size_t align = 256) {
        const size_t at = (off + align - 1) / align * align;
        off = at + (bytes + align - 1) / align * align;
        if (log) log->push_back((int64_t)at);
        return base ? reinterpret_cast<T *>(base + at) : nullptr;
    }
};
// the solvers' layouts on null-based carvers that log their offsets (ws / ws_small, or the V-cycle's one buffer);
// bytes[2] = what each DevBuf::ensure is asked for. No HIP call (the lab library's CPU test).
void pcg_layout_probe(int64_t n, int64_t ncols, int64_t maxiter, bool gen, bool own_x, int P,
                      std::vector<int64_t> *log, int64_t *bytes);
void gmres_layout_probe(int64_t n, int64_t maxiter, int64_t restart, bool gen, std::vector<int64_t> *log, int64_t *bytes);
void bicgstab_layout_probe(int64_t n, int64_t maxiter, bool gen, std::vector<int64_t> *log, int64_t *bytes);
void minres_layout_probe(int64_t n, int64_t maxiter, bool gen, std::vector<int64_t> *log, int64_t *bytes);
void vcycle_layout_probe(int64_t n, int64_t maxiter, bool dev_io, std::vector<int64_t> *log, int64_t *bytes);
void pcg_multi_layout_probe(int64_t n, int64_t maxiter, int nrhs, std::vector<int64_t> *log, int64_t *bytes);

// A layout callable (Carve &big, Carve &small) on null-based carvers that log their offsets: the body of a
// *_layout_probe. floor: the least the large buffer is sized to (kWsFloor where a solver never leaves it empty).
constexpr size_t kWsFloor = 256;
template <class Layout> void layout_sizes(Layout &&layout, size_t floor, std::vector<int64_t> *log, int64_t *bytes) {
    Carve big, sm;
    big.log = sm.log = log;
    layout(big, sm);
    bytes[0] = (int64_t)(big.off > floor ? big.off : floor);
    bytes[1] = (int64_t)sm.off;
}
// The same callable on A->ws and A->ws_small; need[2] (optional): the bytes of each the layout covers. grow: size the two
// buffers first (a later solve then keeps them); otherwise PSK_ERR_ARG when either is smaller than the layout (the
// lab library's views of a finished solve).
template <class Layout> int workspace_carve(psk_csr *A, size_t floor, bool grow, Layout &&layout, int64_t *need) {
    int64_t sizes[2];
    if (!need) need = sizes;
    layout_sizes(layout, floor, nullptr, need);
    if (grow) {
        PSK_TRY(A->ws.ensure((size_t)need[0]));
        PSK_TRY(A->ws_small.ensure((size_t)need[1]));
    }
    if (!A->ws.p || !A->ws_small.p || A->ws.bytes < (size_t)need[0] || A->ws_small.bytes < (size_t)need[1])
        return fail(PSK_ERR_ARG, "the matrix's workspace is smaller than this layout");
    Carve big{A->ws.as<char>()}, sm{A->ws_small.as<char>()};
    layout(big, sm);
    return PSK_OK;
}

// ---- what every solver writes into its psk_result the same way (res was zeroed by the entry point) ----
inline void result_msg(psk_result *res, const char *m) { std::snprintf(res->msg, sizeof(res->msg), "%s", m); }
// a solve with nothing to do (no rows, b = 0): x = 0, handleConvergence(0, zeros, 0, 0)
inline void result_trivial(psk_result *res) {
    res->status = PSK_CONVERGED;
    res->success = 1;
    res->iters = 1;
    res->exit = PSK_EXIT_NONE;
}
// the interval between the solve's two events, both complete (0 when the runtime cannot tell)
inline double loop_ms(const SolveKit *kit) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, kit->ev0, kit->ev1);
    return ms;
}
// handleMaxiter(maxiter - 1, ...): the iteration a solve that ran out of iterations reports
inline int64_t maxiter_iters(int64_t maxiter) { return maxiter > 0 ? maxiter - 1 : 0; }
// How a loop ended, as its device state says it and its solver words it.
struct SolveOutcome {
    int32_t zero_b;   // b = 0: no iteration ran
    int32_t done;     // 1: stopped (by_tol: by the tolerance test, else at maxiter without fail_on_maxiter),
    int32_t by_tol;   // 2: breakdown, 0: out of iterations
    int64_t iters_stop, iters_brk;   // the iteration number a stop and a breakdown report
    double rec;                      // the last recursive residual
    const char *brk_msg;
};
// status, success, exit, iters, resid and msg of the four outcomes
inline void result_outcome(const SolveOutcome &o, int64_t maxiter, psk_result *res) {
    if (o.zero_b) {   // x = 0 and resid = 0, as psk_pcg reports it
        result_trivial(res);
    } else if (o.done == 1) {
        res->status = PSK_CONVERGED;
        res->success = 1;
        res->iters = o.iters_stop;
        res->resid = o.rec;
        res->exit = o.by_tol ? PSK_EXIT_TOLERANCE : PSK_EXIT_MAXITER;
    } else if (o.done == 2) {
        res->status = PSK_BREAKDOWN;
        res->exit = PSK_EXIT_DOT_BREAKDOWN;
        res->success = 0;
        res->iters = o.iters_brk;
        res->resid = NAN;
        result_msg(res, o.brk_msg);
    } else {
        res->status = PSK_MAXITER;
        res->exit = PSK_EXIT_MAXITER;
        res->success = 0;
        res->iters = maxiter_iters(maxiter);
        res->resid = o.rec;
        result_msg(res, "failure to converge");
    }
}
// A tolerance exit reports the true residual tr = ||b - A x|| in place of the recursive one; enforce: a tr above
// tau ||b|| fails the solve.
inline void result_true_resid(const char *method, double tr, double tauNormB, double tau, double rec, bool enforce,
                              psk_result *res) {
    res->resid = tr;
    if (!enforce || tr <= tauNormB) return;
    res->status = PSK_TRUE_RESID_FAIL;
    res->success = 0;
    std::snprintf(res->msg, sizeof(res->msg),
                  "%s failure: true residual %12.5g did not meet tolerance tau=%12.5g. Recursive residual was %12.5g.",
                  method, tr, tau, rec);
}
// hist_len = the nhist entries the device wrote, at most maxiter, and their copy when the caller asked for it
inline int result_history(int64_t nhist, int64_t maxiter, const double *dhist, psk_result *res, double *hist) {
    const int64_t nh = nhist < maxiter ? nhist : maxiter;
    res->hist_len = nh;
    if (hist && nh > 0) PSK_HIP(hipMemcpy(hist, dhist, (size_t)nh * 8, hipMemcpyDeviceToHost));
    return PSK_OK;
}

// psk_gmres's workspace as the lab library reads it after a solve (gmres.hip gmres_work_view): device pointers
// into the matrix's two buffers. Q: K + 1 columns of stride ldq doubles; H, R: (K + 1) x K column-major.
struct GmresView {
    int64_t n, K, ldq;
    double *Q, *H, *R, *CS, *g, *dy;
    const int32_t *done, *brk, *kconv;
    const double *normB, *tauNormB, *rec;
    void *big, *small;  // the two buffers and the bytes of each this layout covers
    size_t big_bytes, small_bytes;
};
int gmres_work_view(psk_csr *A, int64_t maxiter, int64_t restart, bool gen, bool grow, GmresView *v);

// psk_pcg_multi's workspace as the lab library reads it after a solve (pcg_multi.hip pcg_multi_work_view): device
// pointers into the matrix's two buffers. x, r, p, Ap: n rows of kp interleaved columns; alphas, udrs, paps: kp rows
// of ld = maxiter + 1 entries; state: the solve's device state, pcg_multi_state_bytes() of it, decoded column by
// column by pcg_multi_col_state into kMultiStateWords doubles (done, brk_kind, iters, nhist, normB, tauNormB, udr,
// the last reported ||r||, the init's b.b, the column's last r.r).
struct PcgMultiView {
    int64_t n;
    int kp;
    int64_t ld;
    double *x, *r, *p, *Ap, *alphas, *udrs, *paps;
    const void *state;
};
constexpr int kMultiStateWords = 10;
int pcg_multi_work_view(psk_csr *A, int64_t maxiter, int nrhs, PcgMultiView *v);
size_t pcg_multi_state_bytes();
void pcg_multi_col_state(const void *state, int j, double *out);

// The done stamp (done_stamp_store, called by the kernel of each solver that ends its loop): k + 2 for a kernel of
// iteration k (psk_gmres: step k of the current cycle), 1 for the init (0 = running) — a system-scope store to a
// host-mapped word, drained before the kernel ends, so once an event recorded after this kernel has completed the
// host reads the word directly, with no per-chunk device-to-host copy (a blit kernel) on the solver's stream. The stamp lets the host act on the state as of the chunk it waited
// for, not a later one its GPU has already run: every rank of a sharded solve then stops after the same chunk and
// enqueues the same collectives.
// The word is shared by every solve on the device; each solve tags its stamps with its own generation (high
// bits), so a kernel still queued from an earlier solve that failed on the host side cannot leave a stamp the next
// solve's poll would act on.
constexpr int kStampGenShift = 40;
constexpr int64_t kStampMask = ((int64_t)1 << kStampGenShift) - 1;

// One solve's view of the stamp: a new generation, the word cleared (no kernel of an earlier solve is running).
struct StampPoll {
    SolveKit *kit;
    int64_t gen;
    explicit StampPoll(SolveKit *k) : kit(k), gen((int64_t)(++k->solve_gen & 0x7FFFFF) << kStampGenShift) {
        *static_cast<volatile int64_t *>(kit->hmap) = 0;
    }
    int64_t *hdone() const { return kit->hmap; }   // what the kernels store hgen() | stamp into
    int64_t hgen() const { return gen; }
    int64_t stamp() const {   // a stamp of this solve only (its generation), 0 = none
        const int64_t hv = *static_cast<volatile int64_t *>(kit->hmap);
        return (hv & ~kStampMask) == gen ? (hv & kStampMask) : 0;
    }
    // waits for everything enqueued on s so far (an init whose stamp decides whether the loop runs at all)
    int wait(hipStream_t s) {
        PSK_HIP(hipEventRecord(kit->fev[0], s));
        PSK_HIP(hipEventSynchronize(kit->fev[0]));
        return PSK_OK;
    }
    // In front of iteration k, chunks of C iterations: every C iterations an event; the host waits on the event L
    // chunks back and then reads the stamp. *stop: the solve ended within the chunks that event covers.
    template <int L> int step(int64_t k, int C, hipStream_t s, bool *stop) {
        static_assert(kPollSlots >= L + 2, "poll slots");
        *stop = false;
        if (k == 0 || k % C != 0) return PSK_OK;
        const int64_t chunk = k / C;   // chunks fully enqueued
        PSK_HIP(hipEventRecord(kit->fev[(chunk - 1) % kPollSlots], s));
        if (chunk - 1 - L < 0) return PSK_OK;
        PSK_HIP(hipEventSynchronize(kit->fev[(chunk - 1 - L) % kPollSlots]));
        const int64_t v = stamp();
        *stop = v != 0 && v <= (chunk - L) * (int64_t)C + 1;
        return PSK_OK;
    }
};

// ---- the frame of psk_bicgstab, psk_minres, psk_gmres and psk_pcg_multi -------------------------------------------
// what the phases of one solve share; each solver's *Run adds its own
struct SolveRun {
    psk_csr *A;
    const psk_prec *M;
    const psk_ctl *ctl;
    Context *c;
    SolveKit *kit;
    hipStream_t s;
    int64_t n, nv;   // nv: the one-shot grid of the elementwise kernels
    int C;           // iterations per poll chunk
    bool gen;        // general preconditioner: applied by its own launches (prec_apply_dev)
    const double *dinv;
};

// An entry point `fn` of the method `method`: the arguments every one of them refuses, r filled, the device's solve
// lock, the nres results zeroed, then phases(); a solve that failed on the host side leaves no kernel of its own
// running behind the next solve. tile: rows per workgroup of the elementwise kernels (nv).
template <class Phases>
int solve_entry(const char *fn, const char *method, SolveRun &r, const psk_csr *Ac, const psk_prec *M, const void *b,
                const void *x, const psk_ctl *ctl, psk_result *res, int nres, int tile, Phases &&phases) {
    auto refuse = [fn](int code, const std::string &what) { return fail(code, std::string(fn) + ": " + what); };
    if (!Ac || !b || !x || !ctl || !res) return refuse(PSK_ERR_ARG, "NULL argument");
    if (ctl->maxiter < 0) return refuse(PSK_ERR_ARG, "negative maxiter");
    if (M && M->n != Ac->n) return refuse(PSK_ERR_ARG, "preconditioner size mismatch");
    if (!Ac->comm && Ac->ncols != Ac->n) return refuse(PSK_ERR_ARG, "matrix must be square");
    if (Ac->comm && Ac->comm->nranks > 1)
        return refuse(PSK_ERR_UNSUPPORTED, std::string("sharded ") + method + " not built (replicas only)");
    r.A = const_cast<psk_csr *>(Ac);
    r.M = M;
    r.ctl = ctl;
    PSK_TRY(ctx(&r.c));
    std::lock_guard<std::mutex> solve_lock(r.c->solve_mu);
    r.s = r.c->stream;
    std::memset(res, 0, sizeof(*res) * (size_t)nres);
    r.n = Ac->n;
    r.nv = r.n > 0 ? (r.n + tile - 1) / tile : 1;
    if (r.nv > INT32_MAX) return refuse(PSK_ERR_UNSUPPORTED, "vector too long for a one-shot grid");
    r.C = ctl->check_every > 0 ? ctl->check_every : (r.n >= (1 << 20) ? 2 : 16);
    r.gen = prec_is_general(M);
    r.dinv = prec_jacobi_dinv(M);
    const int rc = phases();
    if (rc != PSK_OK) (void)hipStreamSynchronize(r.s);
    return rc;
}

// The loop: iterations 0 .. kmax - 1 enqueued ahead of the device, polled every r.C of them with a lag of L chunks.
// *launched: the iterations enqueued.
template <int L, class Iteration>
int poll_loop(StampPoll &poll, const SolveRun &r, int64_t kmax, int64_t *launched, Iteration &&iteration) {
    for (int64_t k = 0; k < kmax; ++k) {
        bool stop;
        PSK_TRY(poll.step<L>(k, r.C, r.s, &stop));
        if (stop) break;
        PSK_TRY(iteration(k));
        *launched = k + 1;
    }
    return PSK_OK;
}

// behind the last launch: the end of loop_ms, the wait for the stream, the checks of the in-launch reductions and of
// the preconditioner's triangular solves
inline int solve_finish(const SolveRun &r, psk_result *res) {
    PSK_HIP(hipEventRecord(r.kit->ev1, r.s));
    PSK_HIP(hipStreamSynchronize(r.s));
    // an expired in-launch reduction wait poisons a sum with NaN; report it as the error it is rather than as a
    // numerical non-convergence (and never to a later solve)
    PSK_TRY(gridsum_check(r.c));
    if (r.gen) PSK_TRY(prec_check_error(r.M, r.s));
    res->loop_ms = loop_ms(r.kit);
    return PSK_OK;
}

// the end of a report: the history (result_history), x to the caller, the wait for both
inline int result_copy_out(const SolveRun &r, int64_t nhist, const double *dhist, const double *dx, psk_result *res,
                           double *hist, double *xout, int32_t loc) {
    PSK_TRY(result_history(nhist, r.ctl->maxiter, dhist, res, hist));
    PSK_TRY(from_device_vec(dx, loc, r.n, xout, r.s));
    PSK_HIP(hipStreamSynchronize(r.s));
    return PSK_OK;
}

}  // namespace psk
