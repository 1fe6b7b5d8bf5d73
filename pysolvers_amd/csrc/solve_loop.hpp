// solve_loop.hpp — host-side helpers of the device-loop solvers (psk_pcg, psk_bicgstab, psk_minres, psk_gmres, psk_vcycle): the
// workspace carver, the done-stamp poll and the psk_result lines they all write alike. Host code only: no kernel
// lives here (the kernels' side of the stamp is done_stamp_store, psk_internal.hpp).
#pragma once
#include "psk_internal.hpp"

#include <cstdio>

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

}  // namespace psk
