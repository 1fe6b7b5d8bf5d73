// spmv.hip — the SpMV entry every solver calls (launch_spmv: argument checks, the grid sum and mailbox set-up,
// the empty shard's dot, then the layout's launcher), the layout chooser, and psk_spmv / psk_spmv_timed. The
// kernels are in spmv_csr.hip, spmv_sliced.hip and spmv_diag.hip; what they share is in spmv.hpp.
#include "spmv.hpp"
#include "dist.hpp"
#include "pcg_state.hpp"

#include <cstdlib>

namespace psk {

int csr_choose_layout(psk_csr *A, hipStream_t s) {
    const char *e = std::getenv("PSK_SPMV_LAYOUT");
    if (e && std::strcmp(e, "csr") == 0) return PSK_OK;
    // the diagonal layout first, when the matrix has one (it streams 1 B per row): automatically and with
    // PSK_SPMV_LAYOUT=diag (which otherwise falls back to the automatic choice); PSK_SPMV_DIAG=0 leaves it out
    const char *de = std::getenv("PSK_SPMV_DIAG");
    const bool diag_env = e && std::strcmp(e, "diag") == 0;
    if ((!e || diag_env) && !(de && std::atoi(de) == 0)) {
        PSK_TRY(diag_build(A, s, false));
        if (A->dg_mask) return PSK_OK;
    }
    if (diag_env) e = nullptr;
    const bool wide = e && std::strcmp(e, "sliced_wide") == 0;
    const bool plain = e && std::strcmp(e, "sliced") == 0;
    const bool force = e && (plain || wide || std::strcmp(e, "sliced_dict") == 0);
    // auto and sliced_dict: a dictionary when the values allow one (never an error here)
    int rc = sliced_build(A, s, force, !wide, !wide && !plain, false);
    if (rc != PSK_OK) sliced_free(A);
    return rc;
}

int tile_rows_for(int64_t n, int64_t nnz) {
    // rows per tile so that a typical tile's entries fit one LDS chunk
    const double avg = n > 0 ? (double)nnz / (double)n : 1.0;
    int r = kBlock;
    while (r > 32 && avg * r > kChunk) r >>= 1;
    return r;
}

// the dot of an SpMV over no rows: 0, into partial[0] and the mailbox like a finished grid sum
__global__ void spmv_empty_dot_kernel(GridSum gs, const int32_t *done) {
    if (threadIdx.x != 0 || (done && *done)) return;
    const double z[1] = {0.0};
    gs.out[0] = 0.0;
    gridsum_mail<1>(gs, z);
}

int launch_spmv(const psk_csr *A, int mode, const double *x, double *y, const double *aux_d,
                const double *aux_q, double *partial, const int32_t *done_flag, hipStream_t s, hipEvent_t ev0,
                hipEvent_t ev1, int rev, uint64_t *mail_seq, const SpmvFlush *flush) {
    Context *c;
    PSK_TRY(ctx(&c));
    if (flush && (mode != kSpmvDot || !partial || !spmv_flush_eligible(A) || kPcgStagger == 0 || flush->k < 1))
        return fail(PSK_ERR_ARG, "launch_spmv: the flush role needs the PCG loop's launch in the diagonal pair layout");
    const bool sliced = A->sl_off != nullptr || A->dg_mask != nullptr;   // 256-row slices
    const int64_t nwg = sliced ? (A->n + kSlice - 1) / kSlice : (A->n + A->tile_rows - 1) / A->tile_rows;
    GridSum gs{nullptr, nullptr, nullptr, nullptr, 0, 0, -1, nullptr, nullptr, 0, 0};
    if (partial && nwg > 0) PSK_TRY(gridsum_prepare(c, nwg, 1, partial, &gs));
    if (partial && nwg == 0) gs.out = partial;
    if (mail_seq) {
        if (!partial || !A->comm || !A->comm->mb) return fail(PSK_ERR_ARG, "launch_spmv: mailbox without a dot");
        *mail_seq = mbox_next(A->comm, &gs);
    }
    if (A->n == 0) {   // no rows (an empty shard): the dot is 0, still published
        if (partial) {
            hipLaunchKernelGGL(spmv_empty_dot_kernel, dim3(1), dim3(64), 0, s, gs, done_flag);
            PSK_HIP(hipGetLastError());
        }
        return PSK_OK;
    }
    const SpmvLaunch L{x, y, aux_d, aux_q, gs, done_flag, s, ev0, ev1, rev != 0, nwg};
    if (A->dg_mask) return launch_spmv_diag(A, mode, L, flush);
    if (A->sl_off) return launch_spmv_sliced(A, mode, L);
    return launch_spmv_csr(A, mode, L);
}

}  // namespace psk

using namespace psk;

extern "C" {

int psk_spmv(const psk_csr *Ac, const double *x, double *y, int32_t loc) {
    if (!Ac || !x || !y) return fail(PSK_ERR_ARG, "psk_spmv: NULL argument");
    psk_csr *A = const_cast<psk_csr *>(Ac);
    Context *c;
    PSK_TRY(ctx(&c));
    const double *dx = x;
    double *dy = y;
    DevBuf tmp;
    if (loc == PSK_HOST || A->comm) {
        // stage into [owned | halo] x and y
        PSK_TRY(tmp.ensure((size_t)(A->ncols + A->n) * sizeof(double)));
        double *tx = tmp.as<double>();
        const bool dry = A->comm && A->comm->dry;   // caller passes [owned | halo]
        const int64_t nx = (A->comm && !dry) ? A->n : A->ncols;   // rectangular: x has ncols entries
        PSK_TRY(to_device_vec(x, loc, nx, tx, c->stream));
        if (A->comm) PSK_TRY(halo_exchange(A, tx, c->stream));
        dx = tx;
        dy = (loc == PSK_HOST) ? tx + A->ncols : y;
    }
    PSK_TRY(launch_spmv(A, kSpmvPlain, dx, dy, nullptr, nullptr, nullptr, nullptr, c->stream));
    if (loc == PSK_HOST) PSK_TRY(from_device_vec(dy, PSK_HOST, A->n, y, c->stream));
    PSK_HIP(hipStreamSynchronize(c->stream));
    tmp.release();
    return PSK_OK;
}

int psk_spmv_timed(const psk_csr *A, const double *x, double *y, int32_t reps, double *avg_ms) {
    if (!A || !x || !y || reps < 1 || !avg_ms) return fail(PSK_ERR_ARG, "psk_spmv_timed: bad arguments");
    if (A->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_spmv_timed: sharded matrix");
    Context *c;
    PSK_TRY(ctx(&c));
    hipEvent_t e0, e1;
    PSK_HIP(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));   // timing only (runtime.hip)
    PSK_HIP(hipEventCreateWithFlags(&e1, hipEventDisableSystemFence));
    constexpr int mode = kSpmvPlain;
    DevBuf part;
    if (mode == kSpmvDot) PSK_TRY(part.ensure(64));
    double *pp = mode == kSpmvDot ? part.as<double>() : nullptr;
    int rc = launch_spmv(A, mode, x, y, nullptr, nullptr, pp, nullptr, c->stream);   // warm
    if (rc == PSK_OK && hipEventRecord(e0, c->stream) != hipSuccess) rc = fail(PSK_ERR_HIP, "event record");
    for (int r = 0; r < reps && rc == PSK_OK; ++r)
        rc = launch_spmv(A, mode, x, y, nullptr, nullptr, pp, nullptr, c->stream);
    if (rc == PSK_OK && hipEventRecord(e1, c->stream) != hipSuccess) rc = fail(PSK_ERR_HIP, "event record");
    float ms = 0.f;
    if (rc == PSK_OK && hipEventSynchronize(e1) != hipSuccess) rc = fail(PSK_ERR_HIP, "event sync");
    if (rc == PSK_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = fail(PSK_ERR_HIP, "event time");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (mode == kSpmvDot) (void)hipStreamSynchronize(c->stream);   // before `part` is freed
    part.release();
    if (rc == PSK_OK) *avg_ms = (double)ms / reps;
    return rc;
}

}  // extern "C"
