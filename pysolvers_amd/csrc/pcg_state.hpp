// pcg_state.hpp — the PCG solver state and the K3 scalar logic (PCGSolver.py:113-138), shared by pcg.hip
// (the loop, K0/K2/K3) and spmv_diag.hip (the PCG init fused into the first SpMV of the diagonal layout, the
// flush role of the in-loop SpMV).
#pragma once
#include "psk_internal.hpp"
#include "solve_loop.hpp"

namespace psk {

struct PcgState {
    int32_t done;      // 0 running, 1 converged, 2 breakdown
    int32_t brk_kind;  // 1: dot(u,r)==0 at start, 2: dot(p,Ap)==0
    int64_t iters;
    double resid;
    double normB;
    double tauNormB;
    int64_t live;      // k of the last K2 that ran to completion (no breakdown); -1 before the loop
    int64_t *hdone;    // host-mapped stamp of the iteration that set `done` (nullptr: none), see set_done
    int64_t hgen;      // this solve's generation in the stamp's high bits (kStampGenShift)
    double last_hist;  // the latest reported ||r_k|| (resid_recursive without copying the history back)
    int32_t x_written; // 1 once x has been stored (Jacobi/identity: x0 = 0 is implicit until the first flush)
    int32_t pad;
};

// done = v != 0, and the host-mapped stamp the solve loop polls (solve_loop.hpp, StampPoll): k + 2 for a kernel of
// iteration k, 1 for the init
__device__ __forceinline__ void set_done(PcgState *st, int32_t v, int64_t stamp) {
    st->done = v;
    if (st->hdone) done_stamp_store(st->hdone, st->hgen, stamp);
}

// the solver state after the init sums bb = b.b and ur = u.r (PCGSolver.py:86-105)
__device__ __forceinline__ void pcg_init_state(double bb, double ur, double tau, PcgState *st, double *udr,
                                               int64_t *hdone, int64_t hgen, int32_t x_written) {
    const double normB = sqrt(bb);                 // self.norm(b)   :86
    st->normB = normB;
    st->tauNormB = tau * normB;
    st->iters = 0;
    st->resid = 0.0;
    st->brk_kind = 0;
    st->live = -1;
    st->hdone = hdone;
    st->hgen = hgen;
    st->last_hist = normB;
    st->x_written = x_written;
    udr[0] = ur;
    if (normB == 0.0) {                            // :87-88 handleConvergence(0, zeros, 0, 0)
        st->iters = 1;
        set_done(st, 1, 1);
    } else if (ur == 0.0) {                        // :104-105
        st->brk_kind = 1;
        st->iters = 0;
        set_done(st, 2, 1);
    } else {
        st->done = 0;
    }
}

// fused init finish: runs once, in thread 0 of the workgroup that completes the init's grid sums
struct PcgInitFin {
    double tau;
    PcgState *st;
    double *udr;
    int64_t *hdone;
    int64_t hgen;
    int32_t x_written;
    int32_t off;   // b.b and u.r are sums off, off + 1 of the launch (the diagonal layout's fused init: 1)
    __device__ void operator()(const double *r) const {
        pcg_init_state(r[off], r[off + 1], tau, st, udr, hdone, hgen, x_written);
    }
};

// Deferred x updates (Jacobi/identity K3): x is read and written every kPcgDefer-th iteration only.
// p_j lives in ring buffer j mod kPcgDefer; K3 of iteration k reads p_k and writes p_{k+1} over
// p_{k+1-kPcgDefer}, which the last flush consumed (or, on a flush, which this K3 reads first, element
// by element). A flush applies the pending updates in iteration order, x = ((x + a_{k-q} p_{k-q}) + ...)
// + a_k p_k, the reference's two roundings per update in its order (PCGSolver.py:121), so x is
// bit-identical to updating every iteration. x traffic per iteration: 16 B/row updated every
// iteration, 8 (kPcgDefer + 1) / kPcgDefer deferred (12 at 2, 10 at 4, 9 at 8). Round 5 A/B
// (profiles/r5_pcg_defer_ab.txt, same bits): 8 = 4 at N = 10M, +2.2% at 16384^2; 2 and 3 slower.
#ifndef PSK_PCG_DEFER
#define PSK_PCG_DEFER 8
#endif
constexpr int kPcgDefer = PSK_PCG_DEFER;
static_assert(kPcgDefer >= 1 && kPcgDefer <= 8, "kPcgDefer");
struct PRing {
    double *b[kPcgDefer];
};
// iterations whose x update is still pending when K3 of iteration k runs: k - q .. k - 1 (the uniform flush of
// the paths that are not staggered, below)
__host__ __device__ inline int pcg_pending(int64_t k) { return (int)(k % kPcgDefer); }

// The staggered flush (unsharded Jacobi/identity solves in the diagonal pair layout): the flush leaves K3 and
// runs, a block of rows at a time, as extra streaming workgroups of the in-loop SpMV launches (spmv_diag.hip, the
// flush role of spmv_diagp_kernel). The rows are cut into S contiguous blocks on K3-tile boundaries; SpMV launch
// k >= 1 brings block k mod S up to date, i.e. applies every pending update of iterations < k in iteration order.
// Whoever ends the solve (K3 on convergence or at maxiter - 1, pcg_flush_kernel after a breakdown) catches up
// every row with its own block's pending range. The whole rule is pcg_flush_pending; the SpMV's flush role, K3,
// pcg_flush_kernel and the host all call it.
// Ring: SpMV k reads p_{k-S} .. p_{k-1} after K3 k-1 has written p_k over p_{k-kPcgDefer}, so S < kPcgDefer;
// K3 k then overwrites p_{k+1-kPcgDefer}, older than anything still pending (at most S - 1 iterations back).
// -DPSK_PCG_STAGGER=0 builds the uniform flush in K3 everywhere.
#ifndef PSK_PCG_STAGGER
#define PSK_PCG_STAGGER 1
#endif
#define PSK_PCG_STAGGER_ON (PSK_PCG_STAGGER && PSK_PCG_DEFER >= 2)
constexpr int kPcgStagger = PSK_PCG_STAGGER_ON ? kPcgDefer - 1 : 0;   // S (0: not staggered)
static_assert(kPcgStagger >= 0 && kPcgStagger < kPcgDefer, "SpMV k reads p_{k-S} after K3 k-1 wrote p_k: S < ring");

struct PcgPend {
    int64_t first, last;   // iterations first .. last are pending (first > last: none); first == 0: the block
                           // was never stored, x is still the implicit x0 = 0
};
// K3 tiles per block and the block of a tile (nv tiles cut into S blocks; the last blocks may own no tile)
__host__ __device__ inline int64_t pcg_block_tiles(int64_t nv, int S) { return (nv + S - 1) / S; }
__host__ __device__ inline int pcg_block_of_tile(int64_t tile, int64_t nv, int S) {
    return (int)(tile / pcg_block_tiles(nv, S));
}
// The schedule. Block blk of S: the updates pending
//   in_spmv: when the flush role of SpMV launch k runs (it serves blk == k mod S; launches 1 .. k-1 have run),
//   else:    when K3 of iteration k (or pcg_flush_kernel after a breakdown at k) runs (launches 1 .. k have run).
// A block was last brought up to date by launch f, the largest f in [1, kk] with f mod S == blk, which applied
// the iterations < f; no such launch: f = 0.
__host__ __device__ inline PcgPend pcg_flush_pending(int S, int blk, int64_t k, bool in_spmv) {
    const int64_t kk = in_spmv ? k - 1 : k;
    int64_t f = kk - ((kk - blk) % S + S) % S;
    if (f < 1) f = 0;
    return PcgPend{f, k - 1};
}
// the same for the uniform flush: one block, brought up to date by K3 of every kPcgDefer-th iteration
__host__ __device__ inline PcgPend pcg_uniform_pending(int64_t k) { return PcgPend{k - pcg_pending(k), k - 1}; }

// x[j] with the pending updates of iterations first .. k - 1 applied (ring: their p; alphas[i] = a_i)
__device__ __forceinline__ double pcg_catch_up(double xj, const PRing *pr, int64_t first, int64_t k,
                                               const double *__restrict__ alphas, int64_t j) {
    for (int64_t t = first; t < k; ++t) xj = xj + alphas[t] * pr->b[t % kPcgDefer][j];   // :121
    return xj;
}

// The flush role's arguments of an in-loop SpMV launch (launch_spmv fills in the grid fields)
struct SpmvFlush {
    double *x;                // the solution vector
    const double *alphas;     // alphas[i] = a_i
    PRing pr;
    int64_t k;                // this launch's iteration (>= 1)
    int64_t nv;               // K3 tiles of the vector
    uint32_t ost, ofl;        // octets (8 workgroups, one per XCD) of stencil / flush workgroups
    uint32_t nfl;             // flush workgroups (K3 tiles of block k mod S)
    uint32_t mul;             // octet o is a flush octet iff (o mul) >> 16 steps there (0: the flush octets last)
};

// K3 prologue shared by the Jacobi/identity and general-preconditioner variants: alpha again
// (K2's expression on the same partials), the convergence test, beta. Returns false when the
// solve stopped at this iteration; x (which K3 owns) is then still advanced over the tile.
// pr != nullptr: the deferred x updates pd of the tile's rows (the schedule above) are applied first.
__device__ inline bool pcg_direction_scalars(int64_t n, double *__restrict__ x, const double *__restrict__ p,
                                             double pTAp, double rr, double ur, double udk, double tauNB,
                                             PcgState *st, double *__restrict__ udr, double *__restrict__ hist, int64_t k,
                                             int64_t maxiter, int fail_on_maxiter, double &alpha, double &beta,
                                             int64_t tile, const PRing *pr = nullptr,
                                             const double *__restrict__ alphas = nullptr,
                                             PcgPend pd = PcgPend{0, -1}) {
    alpha = udk / pTAp;                                      // :118 (udk = udr[k])
    const double normR = sqrt(rr);                           // self.norm(r)  :125
    if (tile == 0 && threadIdx.x == 0) {
        hist[k] = normR;                                     // reportIter  :126
        st->last_hist = normR;
    }
    if (normR <= tauNB || (!fail_on_maxiter && k == maxiter - 1)) {   // :129-131 (tauNB = st->tauNormB)
        const int64_t i = tile * kVecTile + 2 * threadIdx.x;
        // deferred updates (pr): rows never stored (pd.first == 0) are still the implicit x0 = 0
        const bool x0 = pr && pd.first == 0;
        for (int64_t j = i; j < i + 2 && j < n; ++j) {
            double xj = x0 ? 0.0 : x[j];
            if (pr) xj = pcg_catch_up(xj, pr, pd.first, k, alphas, j);
            x[j] = xj + alpha * p[j];                        // :121
        }
        if (tile == 0 && threadIdx.x == 0) {
            st->iters = k + 1;                               // handleConvergence(k, ...)
            st->resid = normR;
            st->x_written = 1;
            set_done(st, 1, k + 2);
        }
        return false;
    }
    beta = ur / udk;                                         // :134-135
    if (tile == 0 && threadIdx.x == 0) udr[k + 1] = ur;   // :136
    return true;
}

// the PCG init fused into the first SpMV (spmv_diag.hip, pcg_init_diag_kernel): the diagonal layout in the
// 5-diagonal DPP order, unsharded; xs = the one DInv value (Jacobi) or 1.0 (none). [p_0.Ap_0, b.b, u.r] into
// out3[0..2], p_0 into p, Ap_0 into Ap; fin runs on sums 1 and 2 (fin.off = 1)
bool pcg_init_diag_eligible(const psk_csr *A);
// the in-loop SpMV of this matrix is the pair-row diagonal kernel that carries the flush role (spmv_diag.hip)
bool spmv_flush_eligible(const psk_csr *A);
// psk_pcg takes the staggered flush for this matrix and preconditioner (nullptr: none)
bool pcg_staggers(const psk_csr *A, const psk_prec *M);
// pcg_flush_kernel (pcg.hip) over n rows after a breakdown at iteration k; stag: per-block pending ranges
int launch_pcg_flush(int64_t n, double *x, const PRing &pr, const double *alphas, int64_t k, bool stag, hipStream_t s);
int launch_pcg_init_diag(const psk_csr *A, const double *b, double xs, double *p, double *Ap, double *out3,
                         const PcgInitFin &fin, hipStream_t s);

// psk_pcg's workspace as the lab library reads it after a solve (pcg.hip pcg_work_view): device pointers into the
// matrix's two buffers. x: null unless own_x; u and ring[1 ..]: null unless / when gen (the general path keeps one
// p buffer); part1[0] = p.Ap, part2[0..1] = K2's (r.r, u.r) and, gen, part3[0] = pcg_dot_kernel's u.r: the last
// finished grid sums.
struct PcgView {
    int64_t n, ncols;
    double *r, *Ap, *x, *u, *ring[kPcgDefer];
    double *part1, *part2, *part3, *udr, *hist, *alphas;
    const PcgState *st;
    void *big, *small;  // the two buffers and the bytes of each this layout covers
    size_t big_bytes, small_bytes;
};
int pcg_work_view(psk_csr *A, int64_t maxiter, bool gen, bool own_x, bool grow, PcgView *v);

}  // namespace psk
