// pcg_multi.hip — psk_pcg_multi: 1 .. PSK_PCG_MULTI_MAX right-hand sides in ONE device-resident PCG loop (no reference
// counterpart: the reference solves one vector per call).
//
// Each column j is an independent PCG with the recurrence of psk_pcg (PCGSolver.py:97-138), x0 = 0, every elementwise
// operation rounded once (-ffp-contract=off), every matrix row summed in stored order; the columns share nothing but
// the launches, so the matrix is streamed once per iteration for all of them. The work vectors p, Ap, r and x are
// INTERLEAVED: element (i, j) at i * KP + j with KP = nrhs rounded up to 2 or 4, so the SpMM's one gathered column
// index fetches the KP contiguous doubles of that row of p (16-B accesses). Padding columns are b = 0 columns: done at
// the init and never written afterwards.
//
// Three one-shot launches per iteration k (one tile per workgroup), the solver scalars in PcgMultiState on the device,
// advanced by thread 0 of the wave that completes a launch's gridsum (its `fin`: every other workgroup of that launch
// has read its scalars and published by then); the host only enqueues and polls the done stamp (StampPoll):
//   S  Ap = A p for all KP columns over the matrix's plain CSR arrays (the CSR tile kernel's schedule: colidx / vals
//      streamed once with non-temporal loads, KP rounded products per entry staged through LDS, one row per lane summed
//      in stored order with KP accumulators); p.Ap of every column as ONE width-KP gridsum of rounded products.
//      fin: per running column p.Ap == 0 -> breakdown (that column only), else alpha = udr / p.Ap.
//   U  per running column x += alpha p; r -= alpha Ap; u = DInv r (identity: u = r); [r.r, u.r] of every column as one
//      width-2KP gridsum of rounded products (one row per lane: one term per lane and sum).
//      fin: hist[j][k] = sqrt(r.r); the stopping test and the maxiter rule; beta = u.r / udr; udr = u.r.
//   P  p = u + beta p per running column (u recomputed as DInv r: one rounding, the bits U formed; u is never stored).
// A column that has stopped is frozen: no later launch writes its x, r, p or history. The finisher that stops the last
// running column sets the global done flag and the done stamp; every kernel enqueued behind it returns at once.
// Bytes per row and iteration (KP = 4, CSR with e entries per row): S 12 e + 4 (matrix) + 32 (Ap) + the gathers of p;
// U 4 x 32 read + 2 x 32 written (+ 8 DInv); P 2 x 32 read + 32 written (+ 8 DInv): 320 B of vectors for four columns,
// 80 per column, against the matrix's 12 e + 4 once.
#include "psk_internal.hpp"
#include "dist.hpp"
#include "solve_loop.hpp"
#include "spmv.hpp"

#include <cmath>
#include <cstdio>

namespace psk {

constexpr int kMultiMax = PSK_PCG_MULTI_MAX;
constexpr int kMultiTile = kBlock;   // rows of an init / U / P tile: one row per lane
static_assert(2 * kMultiMax <= kGridSumMaxW, "U publishes [r.r, u.r] of every column as one gridsum");

struct PcgMultiCol {
    int32_t done;      // 0 running, 1 converged (or b = 0), 2 breakdown
    int32_t brk_kind;  // 1: dot(u,r) == 0 at the start, 2: dot(p,Ap) == 0
    int32_t by_tol;    // done by the tolerance test (not by k == maxiter-1 with !fail_on_maxiter)
    int32_t zero_b;    // b.b == 0 (padding columns too)
    int64_t iters;     // as psk_result.iters: k + 1 on convergence, k on a breakdown, 1 for b = 0
    int64_t nhist;     // history entries written
    double normB, tauNormB;
    double udr, alpha, beta;
    double rec;        // the last reported ||r||, normB before the first
    double bb, rr;     // the init's b.b and the last r.r this column took part in (lab)
};
struct PcgMultiState {
    int32_t done;      // every column has stopped
    int32_t running;   // columns still running
    int64_t last_k;    // the iteration whose finisher raised `done` (-1: the init)
    int64_t *hdone;    // host-mapped done stamp (solve_loop.hpp)
    int64_t hgen;
    PcgMultiCol col[kMultiMax];
};

// column j stops; the last one to stop ends the solve: the flag and the stamp the host polls (k + 2 for a kernel of
// iteration k, 1 for the init)
__device__ __forceinline__ void pcgm_stop(PcgMultiState *st, int j, int32_t v, int64_t k) {
    st->col[j].done = v;
    if (--st->running == 0) {
        st->last_k = k;
        st->done = 1;
        done_stamp_store(st->hdone, st->hgen, k + 2);
    }
}

// KP contiguous doubles as 16-B accesses
template <int KP>
__device__ __forceinline__ void ldk(const double *p, double *v) {
#pragma unroll
    for (int h = 0; h < KP / 2; ++h) {
        const dv2 t = ld2(p + 2 * h);
        v[2 * h] = t.x;
        v[2 * h + 1] = t.y;
    }
}
// the live columns of a row: 16-B stores where both columns of a pair are live, else the live one alone; a frozen
// column's element is not written
template <int KP>
__device__ __forceinline__ void stk_live(double *p, const double *v, const bool *live) {
#pragma unroll
    for (int h = 0; h < KP / 2; ++h) {
        if (live[2 * h] && live[2 * h + 1]) st2(p + 2 * h, dv2{v[2 * h], v[2 * h + 1]});
        else if (live[2 * h]) p[2 * h] = v[2 * h];
        else if (live[2 * h + 1]) p[2 * h + 1] = v[2 * h + 1];
    }
}

// ---- init: r = b, p = u = M^-1 b, x = 0 (interleaved); [b.b, u.r] of every column; the b = 0 and u.r = 0 exits ----
struct PcgMultiInitFin {
    double tau;
    PcgMultiState *st;
    double *udrs;      // [KP][maxiter + 1]
    int64_t ld;        // maxiter + 1
    int64_t *hdone;
    int64_t hgen;
    int32_t kp;
    __device__ void operator()(const double *s) const {
        st->hdone = hdone;
        st->hgen = hgen;
        int32_t running = 0;
        for (int j = 0; j < kp; ++j) {
            PcgMultiCol &c = st->col[j];
            const double bb = s[j], ur = s[kp + j];
            const double normB = sqrt(bb);                 // self.norm(b)  :86
            c.bb = bb;
            c.normB = normB;
            c.tauNormB = tau * normB;
            c.rec = normB;
            c.udr = ur;                                    // uDotR = np.dot(u, r)  :102
            udrs[j * ld] = ur;
            if (normB == 0.0) {                            // :87-88 handleConvergence(0, zeros, 0, 0)
                c.zero_b = 1;
                c.iters = 1;
                c.done = 1;
            } else if (ur == 0.0) {                        // :104-105
                c.brk_kind = 1;
                c.done = 2;
            } else {
                ++running;
            }
        }
        st->running = running;
        if (running == 0) {
            st->last_k = -1;
            st->done = 1;
            done_stamp_store(hdone, hgen, 1);
        }
    }
};
template <int KP, bool JAC>
__global__ __launch_bounds__(kBlock) void pcgm_init_kernel(int64_t n, int nrhs, const double *__restrict__ B,
                                                           const double *__restrict__ dinv, double *__restrict__ r,
                                                           double *__restrict__ p, double *__restrict__ x, GridSum gs,
                                                           PcgMultiInitFin fin) {
    const int tid = threadIdx.x;
    const int64_t tl[1] = {(int64_t)blockIdx.x};
    const bool tv[1] = {true};
    const int64_t row = tl[0] * kMultiTile + tid;
    const bool has = row < n;
    double acc[1][2 * KP];
    double bv[KP], uv[KP], zv[KP];
    const double d = JAC && has ? dinv[row] : 1.0;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        bv[j] = has && j < nrhs ? B[row * nrhs + j] : 0.0;   // r = np.copy(b)  :97
        uv[j] = JAC ? d * bv[j] : bv[j];                       // p = precond.applyRight(r)  :98
        zv[j] = 0.0;                                           // x = np.zeros_like(b)  :100
        acc[0][j] = bv[j] * bv[j];
        acc[0][KP + j] = uv[j] * bv[j];
    }
    __shared__ GridSumTile<2 * KP> gsl[1];
    uint32_t ticket[1] = {0};
    if (gs.grp_log2 >= 0 && tid == 0) ticket[0] = gridsum_draw(gridsum_counter(gs, gridsum_group_of(tl[0], gs.grp_log2)));
    if (tid == 0) {
        gsl[0].cnt = 0;
        if (gridDim.x != gs.nt) atomicOr(gs.err, 2);
    }
    __syncthreads();
    if (has) {
        bool all[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) all[j] = true;
        stk_live<KP>(r + row * KP, bv, all);
        stk_live<KP>(p + row * KP, uv, all);
        stk_live<KP>(x + row * KP, zv, all);
    }
    gridsum_tiles_publish<1, 2 * KP>(gs, gsl, acc, ticket, tl, tv, fin);
}

// ---- S: Ap = A p, every column; p.Ap as one width-KP gridsum; alpha, the p.Ap == 0 breakdown --------------------
struct PcgMultiSpmmFin {
    PcgMultiState *st;
    double *alphas, *paps;   // [KP][maxiter + 1]
    int64_t ld, k;
    int32_t kp;
    __device__ void operator()(const double *s) const {
        for (int j = 0; j < kp; ++j) {
            PcgMultiCol &c = st->col[j];
            if (c.done) continue;
            const double pTAp = s[j];                      // np.dot(p, Ap)  :113
            paps[j * ld + k] = pTAp;
            if (pTAp == 0.0) {                             // :114-115 handleBreakdown(k, ...)
                c.brk_kind = 2;
                c.iters = k;
                pcgm_stop(st, j, 2, k);
                continue;
            }
            c.alpha = c.udr / pTAp;                        // :118
            alphas[j * ld + k] = c.alpha;
        }
    }
};
// The CSR tile kernel's schedule (spmv_csr.hip) with KP products per entry: one workgroup per tile of `trows` rows,
// the tile's entries streamed in chunks of kChunk with coalesced non-temporal loads, one gather of KP contiguous
// doubles per entry, the rounded products staged through LDS ([entry][KP]), each lane then sums its own row of each
// column sequentially in stored order from 0.0 (the bits of scipy's csr_matvec, column by column). Rows longer than
// a chunk keep their running sums across chunks.
template <int KP>
__global__ __launch_bounds__(kBlock) void pcgm_spmm_kernel(int64_t n, int trows, const int32_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ colidx,
                                                           const double *__restrict__ vals, const double *__restrict__ p,
                                                           double *__restrict__ Ap, GridSum gs, PcgMultiSpmmFin fin,
                                                           int32_t nnz, TileMap tm) {
    if (fin.st->done) return;
    constexpr int KU = kChunk / kBlock;
    __shared__ double prod[kChunk * KP];
    const int tid = threadIdx.x;
    const int64_t t = tile_of_block(tm);
    const int64_t r0 = t * trows;
    const int64_t r1 = (r0 + trows < n) ? r0 + trows : n;
    const int32_t last = nnz > 0 ? nnz - 1 : 0;   // colidx/vals hold at least one (dummy) entry
    const int32_t e0 = rowptr[r0], e1 = rowptr[r1];
    const int64_t row = r0 + tid;
    const bool has = tid < trows && row < r1;
    const int64_t rowc = has ? row : r0;
    const int32_t rs = rowptr[rowc], re = rowptr[rowc + 1];
    double sum[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) sum[j] = 0.0;
    __shared__ GridSumTile<KP> gsl[1];
    uint32_t ticket[1] = {0};
    bool first = true;
    int32_t c0 = e0;
    do {   // at least once, so that every workgroup passes the barriers and draws its ticket
        const int32_t c1 = (e1 - c0 > kChunk) ? c0 + kChunk : e1;
        const int32_t base = c0 < last ? c0 : last;
        int32_t cc[KU];
        double vv[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int32_t e = c0 + k * kBlock + tid;
            const int32_t ee = e < c1 ? e : base;   // past the chunk: one valid entry re-read, its products dropped
            cc[k] = ld_stream(colidx + ee);
            vv[k] = ld_stream(vals + ee);
        }
        if (first) {
            if (gs.grp_log2 >= 0 && tid == 0) ticket[0] = gridsum_draw(gridsum_counter(gs, gridsum_group_of(t, gs.grp_log2)));
            if (tid == 0) {
                gsl[0].cnt = 0;
                if (gridDim.x != gs.nt) atomicOr(gs.err, 2);
            }
            first = false;
        }
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            double pv[KP];
            ldk<KP>(p + (int64_t)cc[k] * KP, pv);
            const int32_t e = c0 + k * kBlock + tid;
            if (e < c1) {
                double *slot = prod + (k * kBlock + tid) * KP;
#pragma unroll
                for (int h = 0; h < KP / 2; ++h)
                    *reinterpret_cast<dv2 *>(slot + 2 * h) = dv2{vv[k] * pv[2 * h], vv[k] * pv[2 * h + 1]};   // rounded products
            }
        }
        __syncthreads();
        const int32_t a = rs > c0 ? rs : c0;
        const int32_t bnd = re < c1 ? re : c1;
        if (has)
            for (int32_t e = a; e < bnd; ++e) {   // stored order
                double q[KP];
                ldk<KP>(prod + (e - c0) * KP, q);
#pragma unroll
                for (int j = 0; j < KP; ++j) sum[j] = sum[j] + q[j];
            }
        __syncthreads();
        c0 += kChunk;
    } while (c0 < e1);
    double eq[KP];
    ldk<KP>(p + rowc * KP, eq);
    double acc[1][KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) acc[0][j] = has ? eq[j] * sum[j] : 0.0;   // as spmv_row_value: one rounded product per row
    const int64_t tl[1] = {t};
    const bool tv[1] = {true};
    gridsum_tiles_publish<1, KP>(gs, gsl, acc, ticket, tl, tv, fin);
    if (has)   // behind the epilogue (spmv.hpp spmv_row_value); a frozen column's p is frozen, its Ap the same bits again
#pragma unroll
        for (int h = 0; h < KP / 2; ++h) st2nt(Ap + row * KP + 2 * h, dv2{sum[2 * h], sum[2 * h + 1]});
}

// ---- U: x += alpha p; r -= alpha Ap; u = M^-1 r; [r.r, u.r]; history, the stopping test, beta ---------------------
struct PcgMultiUpdateFin {
    PcgMultiState *st;
    double *hist;      // [KP][hld]
    double *udrs;      // [KP][ld]
    int64_t hld, ld, k, maxiter;
    int32_t fail_on_maxiter, kp;
    __device__ void operator()(const double *s) const {
        for (int j = 0; j < kp; ++j) {
            PcgMultiCol &c = st->col[j];
            if (c.done) continue;
            const double rr = s[j], ur = s[kp + j];
            const double normR = sqrt(rr);                 // self.norm(r)  :125
            c.rr = rr;
            hist[j * hld + k] = normR;                     // reportIter  :126
            c.rec = normR;
            c.nhist = k + 1;
            const bool tol = normR <= c.tauNormB;
            if (tol || (!fail_on_maxiter && k == maxiter - 1)) {   // :129-131 handleConvergence(k, ...)
                c.by_tol = tol;
                c.iters = k + 1;
                pcgm_stop(st, j, 1, k);
                continue;
            }
            c.beta = ur / c.udr;                           // :134-135
            c.udr = ur;                                    // :136
            udrs[j * ld + k + 1] = ur;
        }
    }
};
template <int KP, bool JAC>
__global__ __launch_bounds__(kBlock) void pcgm_update_kernel(int64_t n, double *__restrict__ x, double *__restrict__ r,
                                                             const double *__restrict__ p, const double *__restrict__ Ap,
                                                             const double *__restrict__ dinv, GridSum gs,
                                                             PcgMultiUpdateFin fin) {
    const PcgMultiState *st = fin.st;
    if (st->done) return;
    double alpha[KP];
    bool live[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        live[j] = st->col[j].done == 0;
        alpha[j] = st->col[j].alpha;
    }
    const int tid = threadIdx.x;
    const int64_t tl[1] = {(int64_t)blockIdx.x};
    const bool tv[1] = {true};
    const int64_t row = tl[0] * kMultiTile + tid;
    const bool has = row < n;
    double acc[1][2 * KP];
#pragma unroll
    for (int j = 0; j < 2 * KP; ++j) acc[0][j] = 0.0;
    __shared__ GridSumTile<2 * KP> gsl[1];
    uint32_t ticket[1] = {0};
    double xn[KP], rn[KP];
    if (has) {
        double po[KP], ao[KP];
        ldk<KP>(x + row * KP, xn);
        ldk<KP>(r + row * KP, rn);
        ldk<KP>(p + row * KP, po);
        ldk<KP>(Ap + row * KP, ao);
        const double d = JAC ? dinv[row] : 1.0;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            if (!live[j]) continue;
            xn[j] = xn[j] + alpha[j] * po[j];              // x = x + alpha*p  :121
            rn[j] = rn[j] - alpha[j] * ao[j];              // r = r - alpha*Ap  :122
            const double u = JAC ? d * rn[j] : rn[j];      // u = precond.applyRight(r)  :123
            acc[0][j] = rn[j] * rn[j];
            acc[0][KP + j] = u * rn[j];
        }
    }
    if (gs.grp_log2 >= 0 && tid == 0) ticket[0] = gridsum_draw(gridsum_counter(gs, gridsum_group_of(tl[0], gs.grp_log2)));
    if (tid == 0) {
        gsl[0].cnt = 0;
        if (gridDim.x != gs.nt) atomicOr(gs.err, 2);
    }
    __syncthreads();
    if (has) {
        stk_live<KP>(x + row * KP, xn, live);
        stk_live<KP>(r + row * KP, rn, live);
    }
    gridsum_tiles_publish<1, 2 * KP>(gs, gsl, acc, ticket, tl, tv, fin);
}

// ---- P: p = u + beta p per running column -------------------------------------------------------------------------
template <int KP, bool JAC>
__global__ __launch_bounds__(kBlock) void pcgm_direction_kernel(int64_t n, const double *__restrict__ r,
                                                                double *__restrict__ p, const double *__restrict__ dinv,
                                                                const PcgMultiState *st) {
    if (st->done) return;
    const int64_t row = (int64_t)blockIdx.x * kMultiTile + threadIdx.x;
    if (row >= n) return;
    double beta[KP], ro[KP], pn[KP];
    bool live[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        live[j] = st->col[j].done == 0;
        beta[j] = st->col[j].beta;
    }
    ldk<KP>(r + row * KP, ro);
    ldk<KP>(p + row * KP, pn);
    const double d = JAC ? dinv[row] : 1.0;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const double u = JAC ? d * ro[j] : ro[j];
        if (live[j]) pn[j] = u + beta[j] * pn[j];          // p = u + beta*p  :138
    }
    stk_live<KP>(p + row * KP, pn, live);
}

// ---- behind the loop: X[i][j] = x[i * KP + j] ----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pcgm_unpack_kernel(int64_t n, int nrhs, int kp, const double *__restrict__ x,
                                                             double *__restrict__ X) {
    const int64_t row = (int64_t)blockIdx.x * kMultiTile + threadIdx.x;
    if (row >= n) return;
    for (int j = 0; j < nrhs; ++j) X[row * nrhs + j] = x[row * kp + j];
}

struct PcgMultiWork {
    double *io, *x, *r, *p, *Ap;   // io: B on its way in and X on its way out (host vectors)
    PcgMultiState *st;
    double *sums, *hist, *alphas, *udrs, *paps;
};
constexpr int kMultiPap = 0, kMultiRr = 4, kMultiBb = 12, kMultiSums = 20;
static int pcgm_kp(int nrhs) { return nrhs <= 2 ? 2 : 4; }
static void pcgm_layout(Carve &big, Carve &sm, int64_t n, int64_t maxiter, int nrhs, PcgMultiWork &w) {
    const int kp = pcgm_kp(nrhs);
    const size_t vec = (size_t)n * kp * 8, it = (size_t)kp * (size_t)(maxiter + 1) * 8;
    w.io = big.take<double>((size_t)n * nrhs * 8);
    w.x = big.take<double>(vec);
    w.r = big.take<double>(vec);
    w.p = big.take<double>(vec);
    w.Ap = big.take<double>(vec);
    w.st = sm.take<PcgMultiState>(sizeof(PcgMultiState));
    w.sums = sm.take<double>(kMultiSums * 8);   // p.Ap [KP], [r.r, u.r] [2 KP], the init's [b.b, u.r] [2 KP]
    w.hist = sm.take<double>((size_t)kp * (size_t)(maxiter > 0 ? maxiter : 1) * 8);
    w.alphas = sm.take<double>(it);
    w.udrs = sm.take<double>(it);
    w.paps = sm.take<double>(it);
}
void pcg_multi_layout_probe(int64_t n, int64_t maxiter, int nrhs, std::vector<int64_t> *log, int64_t *bytes) {
    PcgMultiWork w;
    layout_sizes([&](Carve &big, Carve &sm) { pcgm_layout(big, sm, n, maxiter, nrhs, w); }, kWsFloor, log, bytes);
}
// A->ws and A->ws_small carved by pcgm_layout; grow: as workspace_carve
static int pcgm_workspace(psk_csr *A, int64_t maxiter, int nrhs, bool grow, PcgMultiWork &w) {
    auto layout = [&](Carve &big, Carve &sm) { pcgm_layout(big, sm, A->n, maxiter, nrhs, w); };
    return workspace_carve(A, kWsFloor, grow, layout, nullptr);
}

// psk_pcg_multi's workspace as the lab library reads it after a solve
int pcg_multi_work_view(psk_csr *A, int64_t maxiter, int nrhs, PcgMultiView *v) {
    if (nrhs < 1 || nrhs > kMultiMax || maxiter < 0) return fail(PSK_ERR_ARG, "pcg_multi_work_view: bad arguments");
    PcgMultiWork w;
    PSK_TRY(pcgm_workspace(A, maxiter, nrhs, false, w));
    *v =PcgMultiView{A->n, pcgm_kp(nrhs), maxiter + 1, w.x, w.r, w.p, w.Ap, w.alphas, w.udrs, w.paps, w.st};
    return PSK_OK;
}
void pcg_multi_col_state(const void *state, int j, double *out) {
    const PcgMultiCol &c = static_cast<const PcgMultiState *>(state)->col[j];
    const double v[kMultiStateWords] = {(double)c.done, (double)c.brk_kind, (double)c.iters, (double)c.nhist, c.normB,
                                        c.tauNormB, c.udr, c.rec, c.bb, c.rr};
    for (int i = 0; i < kMultiStateWords; ++i) out[i] = v[i];
}
size_t pcg_multi_state_bytes() { return sizeof(PcgMultiState); }

// what the phases of one solve share
struct PcgMultiRun : SolveRun {
    int64_t nwg;   // the grid of the SpMM: tiles of A->tile_rows rows
    int nrhs, kp;
    PcgMultiWork w;
    GridSum gsS, gsU;
    // ctl->time_kernels = T > 0: every T-th S launch between two events of the kit's ring
    int64_t tk[kTimedSlots];
    double t_sum;
    int64_t t_n;
};

template <class F> static void pcgm_dispatch(int kp, bool jac, F &&f) {
    if (kp == 2) {
        if (jac) f(std::integral_constant<int, 2>{}, std::true_type{});
        else f(std::integral_constant<int, 2>{}, std::false_type{});
    } else {
        if (jac) f(std::integral_constant<int, 4>{}, std::true_type{});
        else f(std::integral_constant<int, 4>{}, std::false_type{});
    }
}

// everything in front of the loop: the gridsums, the state, B and the init launch
static int pcgm_init(PcgMultiRun &r, const StampPoll &poll, const double *B, int32_t loc) {
    PcgMultiWork &w = r.w;
    hipStream_t s = r.s;
    GridSum gs0;
    PSK_TRY(gridsum_prepare(r.c, r.nwg, r.kp, w.sums + kMultiPap, &r.gsS));
    PSK_TRY(gridsum_prepare(r.c, r.nv, 2 * r.kp, w.sums + kMultiRr, &r.gsU));
    PSK_TRY(gridsum_prepare(r.c, r.nv, 2 * r.kp, w.sums + kMultiBb, &gs0));
    PSK_HIP(hipMemsetAsync(w.st, 0, sizeof(PcgMultiState), s));
    const double *Bd = B;
    if (loc == PSK_HOST) {
        PSK_TRY(to_device_vec(B, loc, r.n * r.nrhs, w.io, s));
        Bd = w.io;
    }
    PSK_HIP(hipEventRecord(r.kit->ev0, s));
    const PcgMultiInitFin fin{r.ctl->tau, w.st, w.udrs, r.ctl->maxiter + 1, poll.hdone(), poll.hgen(), r.kp};
    pcgm_dispatch(r.kp, r.dinv != nullptr, [&](auto kp, auto jac) {
        hipLaunchKernelGGL((pcgm_init_kernel<decltype(kp)::value, decltype(jac)::value>), dim3((unsigned)r.nv), dim3(kBlock),
                           0, s, r.n, r.nrhs, Bd, r.dinv, w.r, w.p, w.x, gs0, fin);
    });
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// the slot's sample, counted when its iteration is below `ran` (an S launch enqueued behind `done` returned at once)
static int pcgm_harvest(PcgMultiRun &r, int slot, int64_t ran) {
    if (r.tk[slot] < 0) return PSK_OK;
    float ms = 0.f;
    PSK_HIP(hipEventSynchronize(r.kit->tb[slot]));
    PSK_HIP(hipEventElapsedTime(&ms, r.kit->ta[slot], r.kit->tb[slot]));
    if (r.tk[slot] < ran) {
        r.t_sum += ms;
        ++r.t_n;
    }
    r.tk[slot] = -1;
    return PSK_OK;
}

// iteration k: S, U, P
static int pcgm_iteration(PcgMultiRun &r, int64_t k) {
    PcgMultiWork &w = r.w;
    hipStream_t s = r.s;
    const int64_t ld = r.ctl->maxiter + 1;
    const dim3 gv((unsigned)r.nv), gw((unsigned)r.nwg), blk(kBlock);
    const int T = r.ctl->time_kernels;
    hipEvent_t ea = nullptr, eb = nullptr;
    if (T > 0 && k % T == 0) {
        const int slot = (int)((k / T) % kTimedSlots);
        // a slot comes round again after kTimedSlots samples, far behind the few chunks the host runs ahead of `done`
        PSK_TRY(pcgm_harvest(r, slot, k));
        r.tk[slot] = k;
        ea = r.kit->ta[slot];
        eb = r.kit->tb[slot];
    }
    const TileMap tm = tile_map_chunked(r.nwg, 128);   // as the CSR tile kernel (spmv_csr.hip kCsrChunk)
    const PcgMultiSpmmFin finS{w.st, w.alphas, w.paps, ld, k, r.kp};
    const PcgMultiUpdateFin finU{w.st, w.hist, w.udrs, r.ctl->maxiter > 0 ? r.ctl->maxiter : 1, ld, k, r.ctl->maxiter,
                                 r.ctl->fail_on_maxiter, r.kp};
    const psk_csr *A = r.A;
    pcgm_dispatch(r.kp, r.dinv != nullptr, [&](auto kp, auto jac) {
        constexpr int KP = decltype(kp)::value;
        constexpr bool JAC = decltype(jac)::value;
        hipExtLaunchKernelGGL((pcgm_spmm_kernel<KP>), gw, blk, 0, s, ea, eb, 0, r.n, A->tile_rows, A->rowptr, A->colidx,
                              A->vals, w.p, w.Ap, r.gsS, finS, (int32_t)A->nnz, tm);
        hipLaunchKernelGGL((pcgm_update_kernel<KP, JAC>), gv, blk, 0, s, r.n, w.x, w.r, w.p, w.Ap, r.dinv, r.gsU, finU);
        hipLaunchKernelGGL((pcgm_direction_kernel<KP, JAC>), gv, blk, 0, s, r.n, w.r, w.p, r.dinv, w.st);
    });
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// behind the loop: the state, X, the checks of the in-launch reductions and loop_ms
static int pcgm_finish(PcgMultiRun &r, PcgMultiState *hs, double *X, int32_t loc, double *loop) {
    PcgMultiWork &w = r.w;
    hipStream_t s = r.s;
    double *Xd = loc == PSK_HOST ? w.io : X;
    hipLaunchKernelGGL(pcgm_unpack_kernel, dim3((unsigned)r.nv), dim3(kBlock), 0, s, r.n, r.nrhs, r.kp, w.x, Xd);
    PSK_HIP(hipGetLastError());
    PSK_HIP(hipEventRecord(r.kit->ev1, s));
    PSK_HIP(hipMemcpyAsync(hs, w.st, sizeof(*hs), hipMemcpyDeviceToHost, s));
    if (loc == PSK_HOST) PSK_TRY(from_device_vec(w.io, loc, r.n * r.nrhs, X, s));
    PSK_HIP(hipStreamSynchronize(s));
    // an expired in-launch reduction wait poisons a sum with NaN; report it as the error it is
    PSK_TRY(gridsum_check(r.c));
    *loop = loop_ms(r.kit);
    return PSK_OK;
}

// column j of the finished state decoded into res with the conventions of psk_pcg, and its history
static int pcgm_report(const PcgMultiRun &r, const PcgMultiState &hs, int j, psk_result *res, double *hist) {
    const PcgMultiCol &c = hs.col[j];
    const int64_t maxiter = r.ctl->maxiter;
    res->norm_b = c.normB;
    res->resid_recursive = c.rec;
    const char *brk = c.brk_kind == 1 ? "breakdown dot(u,r)==0" : "breakdown dot(p, Ap)==0";
    result_outcome({c.zero_b, c.done, c.by_tol, c.iters, c.iters, c.rec, brk}, maxiter, res);
    const size_t at = (size_t)j * (size_t)maxiter;   // column j's history, maxiter entries apart on both sides
    return result_history(c.nhist, maxiter, r.w.hist + at, res, hist ? hist + at : nullptr);
}

// the phases in order; the caller drains the stream when one fails
static int pcgm_solve(PcgMultiRun &r, const double *B, double *X, psk_result *res, double *hist, int32_t loc) {
    PSK_TRY(pcgm_workspace(r.A, r.ctl->maxiter, r.nrhs, true, r.w));
    PSK_TRY(solve_kit(r.c, r.ctl->time_kernels > 0, &r.kit));
    StampPoll poll(r.kit);   // the host-mapped done stamp the finishers write (pcgm_stop)
    PSK_TRY(pcgm_init(r, poll, B, loc));
    int64_t launched = 0;
    PSK_TRY(poll_loop<2>(poll, r, r.ctl->maxiter, &launched, [&](int64_t k) { return pcgm_iteration(r, k); }));
    PcgMultiState hs;
    double loop = 0.0;
    PSK_TRY(pcgm_finish(r, &hs, X, loc, &loop));
    // S launches that did their work: those enqueued behind `done` returned at once
    const int64_t ran = hs.done ? hs.last_k + 1 : launched;
    for (int i = 0; i < kTimedSlots; ++i) PSK_TRY(pcgm_harvest(r, i, ran));
    for (int j = 0; j < r.nrhs; ++j) {
        PSK_TRY(pcgm_report(r, hs, j, &res[j], hist));
        res[j].loop_ms = loop;
        res[j].spmv_launches = r.ctl->time_kernels > 0 ? r.t_n : ran;
        res[j].spmv_ms = r.t_n > 0 ? r.t_sum / (double)r.t_n : 0.0;
    }
    return PSK_OK;
}

}  // namespace psk

using namespace psk;

extern "C" int psk_pcg_multi(const psk_csr *Ac, const psk_prec *M, int32_t nrhs, const double *B, double *X,
                             const psk_ctl *ctl, psk_result *res, double *hist, int32_t loc) {
    // what only this entry point refuses, and its own wording for a sharded matrix, in front of solve_entry (which
    // tests the pointers again): nrhs sizes the results it zeroes, and these read the handles
    if (!Ac || !B || !X || !ctl || !res) return fail(PSK_ERR_ARG, "psk_pcg_multi: NULL argument");
    if (nrhs < 1 || nrhs > PSK_PCG_MULTI_MAX)
        return fail(PSK_ERR_ARG, "psk_pcg_multi: nrhs must be 1 .. " + std::to_string(PSK_PCG_MULTI_MAX));
    if (X == B) return fail(PSK_ERR_ARG, "psk_pcg_multi: X must not alias B");
    if (Ac->comm && Ac->comm->nranks > 1)
        return fail(PSK_ERR_UNSUPPORTED, "psk_pcg_multi: sharded multi-column PCG not built");
    if (Ac->ncols != Ac->n) return fail(PSK_ERR_ARG, "psk_pcg_multi: matrix must be square");
    if (M && M->kind != PSK_PREC_IDENTITY && M->kind != PSK_PREC_JACOBI)
        return fail(PSK_ERR_UNSUPPORTED, "psk_pcg_multi: preconditioner kind " + std::to_string(M->kind) +
                                             " not built (identity and Jacobi only)");
    // the SpMM reads the plain CSR arrays, which every creation path keeps beside the sliced and diagonal copies
    if (Ac->n > 0 && (!Ac->rowptr || !Ac->colidx || !Ac->vals))
        return fail(PSK_ERR_UNSUPPORTED, "psk_pcg_multi: the matrix does not hold its CSR arrays");
    PcgMultiRun r{};
    return solve_entry("psk_pcg_multi", "multi-column PCG", r, Ac, M, B, X, ctl, res, nrhs, kMultiTile, [&]() -> int {
        r.nrhs = nrhs;
        r.kp = pcgm_kp(nrhs);
        r.nwg = r.n > 0 ? (r.n + Ac->tile_rows - 1) / Ac->tile_rows : 1;
        if (r.nwg > INT32_MAX) return fail(PSK_ERR_UNSUPPORTED, "psk_pcg_multi: matrix too long for a one-shot grid");
        for (int i = 0; i < kTimedSlots; ++i) r.tk[i] = -1;
        if (r.n == 0) {   // no rows: every b = 0
            for (int j = 0; j < nrhs; ++j) result_trivial(&res[j]);
            return PSK_OK;
        }
        return pcgm_solve(r, B, X, res, hist, loc);
    });
}
