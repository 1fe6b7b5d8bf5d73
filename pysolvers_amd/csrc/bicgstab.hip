// bicgstab.hip — device-resident right-preconditioned BiCGStab for nonsymmetric systems (no reference
// counterpart: the reference's only nonsymmetric Krylov method is GMRES).
//
// The recurrence, every elementwise operation rounded once (-ffp-contract=off), x0 = 0:
//   r = rhat = p = b; normB = sqrt(b.b) (or ctl->norm_b); rho = rhat.r
//   k:  ph = M^-1 p; v = A ph; alpha = rho / rhat.v; s = r - alpha v; ||s|| <= tau normB: x += alpha ph, stop
//       sh = M^-1 s; t = A sh; omega = t.s / t.t; x = (x + alpha ph) + omega sh; r = s - omega t; hist[k] = ||r||
//       ||r|| <= tau normB (or k == maxiter-1 and !fail_on_maxiter): stop
//       beta = (rhat.r / rho)(alpha / omega); rho = rhat.r; p = r + beta (p - omega v)
// Breakdowns (an ordinary status): rhat.v == 0, t.t == 0, omega == 0, rhat.r == 0.
//
// Schedule built: six launches per iteration for the identity and Jacobi preconditioners, all one-shot (one
// 512-element tile per workgroup, 16-B accesses), every dot finished in its own launch by a deterministic
// gridsum; vector bytes per row:
//   S1  v = A M^-1 p, rhat.v        launch_spmv, kSpmvJacobiDot / kSpmvPlainDot, q = rhat     (the SpMV's)
//   B   alpha; s = r - alpha v; s.s; the half-step test                                       24
//   S2  t = A M^-1 s, t.s           the same SpMV, q = s                                      (the SpMV's)
//   D   t.t                                                                                    8
//   E   omega; x (both terms); r = s - omega t; [r.r, rhat.r] as one width-2 gridsum;
//       convergence test, history, beta, rho, the done stamp                                  56 (+8: DInv, Jacobi)
//   F   p = r + beta (p - omega v)                                                            32
// = 2 SpMV + 120 B/row (128 with Jacobi). The SpMV kernels are untouched: t.t is NOT carried by S2's epilogue
// (its grid sum is one wide). r_0, p_0 and rhat are all b: iteration 0 reads b in their place, so the init is
// one launch (b.b) and nothing is copied.
// General preconditioners (ILU, AMG, dense, Chebyshev): ph and sh are materialised by prec_apply_dev in front of
// S1 and S2 (kSpmvPlainDot), and E reads them (64 B/row; 9 vectors instead of 7).
// The solver scalars (rho, alpha, omega, beta, flags, history) live in BicgState on the device and are advanced
// by thread 0 of the workgroup that completes a launch's gridsum (the `fin` of gridsum_publish: every other
// workgroup of that launch has read its scalars and published by then). The host only enqueues and polls the
// done stamp (StampPoll); every kernel of an iteration enqueued after `done` returns at once. After the loop:
// the half-step exit's x += alpha ph (one small launch, only then), and on a tolerance exit one kSpmvResid
// launch for the true residual ||b - A x||.
#include "psk_internal.hpp"
#include "dist.hpp"
#include "solve_loop.hpp"

#include <cmath>
#include <cstdio>

namespace psk {

struct BicgState {
    int32_t done;      // 0 running, 1 converged, 2 breakdown
    int32_t brk_kind;  // 1: rhat.v == 0, 2: t.t == 0, 3: omega == 0, 4: rhat.r == 0
    int32_t half;      // converged at the half step: x still lacks alpha*ph (bicg_half_x_kernel)
    int32_t by_tol;    // done by the tolerance test (not by k == maxiter-1 with !fail_on_maxiter)
    int32_t zero_b;    // b.b == 0
    int32_t pad;
    int64_t iters;     // the iteration k that raised `done`
    int64_t nhist;     // history entries written
    double normB, tauNormB;
    double rho, alpha, omega, beta;
    double rec;        // the last reported recursive residual
    int64_t *hdone;    // host-mapped done stamp (solve_loop.hpp)
    int64_t hgen;      // this solve's generation in the stamp's high bits
};

// done = v != 0 and the stamp the host polls: k + 2 for a kernel of iteration k, 1 for the init
__device__ __forceinline__ void bicg_set_done(BicgState *st, int32_t v, int64_t stamp) {
    st->done = v;
    done_stamp_store(st->hdone, st->hgen, stamp);
}
__device__ __forceinline__ void bicg_breakdown(BicgState *st, int32_t kind, int64_t k, int64_t nhist) {
    st->brk_kind = kind;
    st->iters = k;
    st->nhist = nhist;
    bicg_set_done(st, 2, k + 2);
}

// ---- init: b.b; normB, rho = rhat.r = b.b, the b = 0 exit ------------------------------------------------
struct BicgInitFin {
    double tau, normb_caller;
    BicgState *st;
    int64_t *hdone;
    int64_t hgen;
    __device__ void operator()(const double *r) const {
        const double bb = r[0];
        const double nb = normb_caller > 0.0 ? normb_caller : sqrt(bb);
        st->normB = nb;
        st->tauNormB = tau * nb;
        st->rho = bb;
        st->rec = nb;
        st->hdone = hdone;
        st->hgen = hgen;
        if (bb == 0.0) {
            st->zero_b = 1;
            bicg_set_done(st, 1, 1);
        }
    }
};
// b.b is summed the way the SpMV sums its dot (spmv.hpp): over the SpMV's tiles of `trows` rows, one row per lane,
// rounded products, DPP wave totals added in wave order, the tiles by gridsum. rho_0 = rhat.r then has the bits
// rhat.v would have for v = b, so a system with A M^-1 b = b exactly (a diagonal A under Jacobi) gives alpha = 1
// and s = 0 exactly, as in exact arithmetic.
__global__ __launch_bounds__(kBlock) void bicg_init_kernel(int64_t n, int trows, const double *__restrict__ b,
                                                           GridSum gs, BicgInitFin fin) {
    const int tid = threadIdx.x;
    const int64_t tl[1] = {(int64_t)blockIdx.x};
    const bool tv[1] = {true};
    const int64_t row = tl[0] * trows + tid;
    const bool has = tid < trows && row < n;
    const double bi = has ? b[row] : 0.0;
    const double acc[1][1] = {{has ? bi * bi : 0.0}};
    __shared__ GridSumTile<1> gsl[1];
    uint32_t ticket[1] = {0};
    if (gs.grp_log2 >= 0 && tid == 0) ticket[0] = gridsum_draw(gridsum_counter(gs, gridsum_group_of(tl[0], gs.grp_log2)));
    if (tid == 0) {
        gsl[0].cnt = 0;
        if (gridDim.x != gs.nt) atomicOr(gs.err, 2);
    }
    __syncthreads();
    gridsum_tiles_publish<1, 1>(gs, gsl, acc, ticket, tl, tv, fin);
}

// ---- B: alpha = rho / rhat.v; s = r - alpha v; s.s; the half-step test ---------------------------------------
struct BicgHalfFin {
    BicgState *st;
    double *hist;
    int64_t k;
    double alpha;
    __device__ void operator()(const double *r) const {
        st->alpha = alpha;
        const double ns = sqrt(r[0]);
        if (ns <= st->tauNormB) {
            hist[k] = ns;
            st->rec = ns;
            st->half = 1;
            st->by_tol = 1;
            st->iters = k;
            st->nhist = k + 1;
            bicg_set_done(st, 1, k + 2);
        }
    }
};
__global__ __launch_bounds__(kBlock) void bicg_s_kernel(int64_t n, const double *__restrict__ r,
                                                        const double *__restrict__ v, double *__restrict__ s,
                                                        const double *__restrict__ rvp, GridSum gs, BicgState *st,
                                                        double *__restrict__ hist, int64_t k) {
    if (st->done) return;
    const double rv = *rvp, rho = st->rho;
    if (rv == 0.0) {   // every workgroup takes this branch on the same bits; none draws a ticket
        if (blockIdx.x == 0 && threadIdx.x == 0) bicg_breakdown(st, 1, k, k);
        return;
    }
    const double alpha = rho / rv;
    __shared__ double sh[kWaves];
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    uint32_t ticket = 0;
    double acc = 0.0;
    if (i + 1 < n) {
        const dv2 ro = ld2(r + i), vo = ld2(v + i);
        ticket = gridsum_ticket(gs);
        dv2 sn;
        sn.x = ro.x - alpha * vo.x;
        sn.y = ro.y - alpha * vo.y;
        st2(s + i, sn);
        acc = fma(sn.x, sn.x, acc);
        acc = fma(sn.y, sn.y, acc);
    } else {
        ticket = gridsum_ticket(gs);
        if (i < n) {
            const double sn = r[i] - alpha * v[i];
            s[i] = sn;
            acc = sn * sn;
        }
    }
    const double sum = block_sum(acc, sh);
    gridsum_publish<1>(gs, &sum, sh, ticket, BicgHalfFin{st, hist, k, alpha});
}

// ---- D: t.t ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void bicg_tt_kernel(int64_t n, const double *__restrict__ t, GridSum gs,
                                                         const BicgState *st) {
    if (st->done) return;
    __shared__ double sh[kWaves];
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    const uint32_t ticket = gridsum_ticket(gs);
    double acc = 0.0;
    if (i + 1 < n) {
        const dv2 tv = ld2(t + i);
        acc = fma(tv.x, tv.x, acc);
        acc = fma(tv.y, tv.y, acc);
    } else if (i < n) {
        acc = t[i] * t[i];
    }
    const double sum = block_sum(acc, sh);
    gridsum_publish<1>(gs, &sum, sh, ticket);
}

// ---- E: omega; x = (x + alpha ph) + omega sh; r = s - omega t; [r.r, rhat.r]; test, history, beta, rho ------
struct BicgFullFin {
    BicgState *st;
    double *hist;
    int64_t k, maxiter;
    int32_t fail_on_maxiter;
    double omega;
    __device__ void operator()(const double *r) const {
        const double nr = sqrt(r[0]);
        hist[k] = nr;
        st->rec = nr;
        st->omega = omega;
        st->nhist = k + 1;
        const bool tol = nr <= st->tauNormB;
        if (tol || (k == maxiter - 1 && !fail_on_maxiter)) {
            st->by_tol = tol;
            st->iters = k;
            bicg_set_done(st, 1, k + 2);
            return;
        }
        const double rho_new = r[1];
        if (rho_new == 0.0) {
            bicg_breakdown(st, 4, k, k + 1);
            return;
        }
        st->beta = (rho_new / st->rho) * (st->alpha / omega);
        st->rho = rho_new;
    }
};
// MODE 0: identity (ph = p, sh = s); 1: Jacobi (ph = d .* p, sh = d .* s, DInv streamed); 2: general (ph and sh
// were materialised: pp = ph, shv = sh)
template <int MODE>
__global__ __launch_bounds__(kBlock) void bicg_xr_kernel(int64_t n, double *__restrict__ x, const double *__restrict__ pp,
                                                         const double *__restrict__ shv, const double *__restrict__ s,
                                                         const double *__restrict__ t, const double *__restrict__ rhat,
                                                         const double *__restrict__ dinv, double *__restrict__ r,
                                                         const double *__restrict__ sums, GridSum gs, BicgState *st,
                                                         double *__restrict__ hist, int64_t k, int64_t maxiter,
                                                         int32_t fail_on_maxiter) {
    if (st->done) return;
    const double ts = sums[0], tt = sums[1], alpha = st->alpha;
    if (tt == 0.0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) bicg_breakdown(st, 2, k, k);
        return;
    }
    const double omega = ts / tt;
    if (omega == 0.0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) bicg_breakdown(st, 3, k, k);
        return;
    }
    __shared__ double sh[2 * kWaves];
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    uint32_t ticket = 0;
    double rr = 0.0, hr = 0.0;
    if (i + 1 < n) {
        const dv2 xo = ld2nt(x + i), po = ld2(pp + i), so = ld2nt(s + i), to = ld2nt(t + i), ho = ld2(rhat + i);
        dv2 ph = po, shh = so;
        if (MODE == 1) {
            const dv2 d = ld2(dinv + i);
            ph.x = d.x * po.x;
            ph.y = d.y * po.y;
            shh.x = d.x * so.x;
            shh.y = d.y * so.y;
        }
        if (MODE == 2) shh = ld2nt(shv + i);
        ticket = gridsum_ticket(gs);
        dv2 xn, rn;
        xn.x = (xo.x + alpha * ph.x) + omega * shh.x;
        xn.y = (xo.y + alpha * ph.y) + omega * shh.y;
        rn.x = so.x - omega * to.x;
        rn.y = so.y - omega * to.y;
        st2nt(x + i, xn);
        st2(r + i, rn);
        rr = fma(rn.x, rn.x, rr);
        rr = fma(rn.y, rn.y, rr);
        hr = fma(ho.x, rn.x, hr);
        hr = fma(ho.y, rn.y, hr);
    } else {
        ticket = gridsum_ticket(gs);
        if (i < n) {
            const double si = s[i];
            const double ph = MODE == 1 ? dinv[i] * pp[i] : pp[i];
            const double shh = MODE == 1 ? dinv[i] * si : MODE == 2 ? shv[i] : si;
            x[i] = (x[i] + alpha * ph) + omega * shh;
            const double rn = si - omega * t[i];
            r[i] = rn;
            rr = rn * rn;
            hr = rhat[i] * rn;
        }
    }
    block_sum2(rr, hr, sh);
    const double v[2] = {rr, hr};
    gridsum_publish<2>(gs, v, sh, ticket, BicgFullFin{st, hist, k, maxiter, fail_on_maxiter, omega});
}

// ---- F: p = r + beta (p - omega v); pin is b at iteration 0, else p itself (updated in place) ---------------
__global__ __launch_bounds__(kBlock) void bicg_p_kernel(int64_t n, const double *__restrict__ r, const double *pin,
                                                        const double *__restrict__ v, double *pout,
                                                        const BicgState *st) {
    if (st->done) return;
    const double beta = st->beta, omega = st->omega;
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    if (i + 1 < n) {
        const dv2 ro = ld2nt(r + i), po = ld2(pin + i), vo = ld2nt(v + i);
        dv2 pn;
        pn.x = ro.x + beta * (po.x - omega * vo.x);
        pn.y = ro.y + beta * (po.y - omega * vo.y);
        st2(pout + i, pn);
    } else if (i < n) {
        pout[i] = r[i] + beta * (pin[i] - omega * v[i]);
    }
}

// ---- the half-step exit's x = x + alpha ph (after the loop, when the state says so) --------------------------
__global__ __launch_bounds__(kBlock) void bicg_half_x_kernel(int64_t n, double *__restrict__ x,
                                                             const double *__restrict__ pp,
                                                             const double *__restrict__ dinv, const BicgState *st) {
    const double alpha = st->alpha;
    const int64_t i0 = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    for (int64_t i = i0; i < i0 + 2 && i < n; ++i) {
        const double ph = dinv ? dinv[i] * pp[i] : pp[i];
        x[i] = x[i] + alpha * ph;
    }
}

struct BicgWork {
    double *bv, *x, *r, *p, *v, *s, *t, *ph, *sh;   // ph, sh: general preconditioners only
    BicgState *st;
    double *sums, *hist;
};
constexpr int kBicgRv = 0, kBicgTs = 1, kBicgTt = 2, kBicgRr = 3, kBicgSs = 5, kBicgBb = 6, kBicgTrue = 7;
// the layout of A->ws (big) and A->ws_small (sm): run on null-based carvers for the sizes, then on the buffers
static void bicg_layout(Carve &big, Carve &sm, int64_t n, int64_t maxiter, bool gen, BicgWork &w) {
    const size_t vec = (size_t)n * 8;
    w.bv = big.take<double>(vec);
    w.x = big.take<double>(vec);
    w.r = big.take<double>(vec);
    w.p = big.take<double>(vec);
    w.v = big.take<double>(vec);
    w.s = big.take<double>(vec);
    w.t = big.take<double>(vec);
    w.ph = gen ? big.take<double>(vec) : nullptr;
    w.sh = gen ? big.take<double>(vec) : nullptr;
    w.st = sm.take<BicgState>(sizeof(BicgState));
    w.sums = sm.take<double>(8 * 8);   // rhat.v, t.s, t.t, [r.r, rhat.r], s.s, b.b, ||b - A x||^2
    w.hist = sm.take<double>((size_t)(maxiter + 1) * 8);
}
void bicgstab_layout_probe(int64_t n, int64_t maxiter, bool gen, std::vector<int64_t> *log, int64_t *bytes) {
    BicgWork w;
    layout_sizes([&](Carve &big, Carve &sm) { bicg_layout(big, sm, n, maxiter, gen, w); }, kWsFloor, log, bytes);
}

// what the phases of one solve share
struct BicgRun : SolveRun {
    BicgWork w;
    GridSum gsB, gsD, gsE;
};

static int bicg_workspace(BicgRun &r) {
    auto layout = [&](Carve &big, Carve &sm) { bicg_layout(big, sm, r.n, r.ctl->maxiter, r.gen, r.w); };
    return workspace_carve(r.A, kWsFloor, true, layout, nullptr);
}

// everything in front of the loop: the gridsums, the state, b, x0 = 0 and the init launch (b.b). *run: iterations
// may be enqueued (false: the stamp already says b = 0; only the general path waits to learn it)
static int bicg_init(BicgRun &r, StampPoll &poll, const double *b, int32_t loc, bool *run) {
    BicgWork &w = r.w;
    hipStream_t s = r.s;
    const int64_t n = r.n;
    GridSum gs0;
    PSK_TRY(gridsum_prepare(r.c, r.nv, 2, w.sums + kBicgRr, &r.gsE));
    PSK_TRY(gridsum_prepare(r.c, r.nv, 1, w.sums + kBicgSs, &r.gsB));
    PSK_TRY(gridsum_prepare(r.c, r.nv, 1, w.sums + kBicgTt, &r.gsD));
    // the init sums b.b over the SpMV's tiles (launch_spmv: 256-row slices, or tile_rows rows in the CSR layout)
    const int trows = (r.A->sl_off || r.A->dg_mask) ? kBlock : r.A->tile_rows;
    const int64_t nwg = (n + trows - 1) / trows;
    PSK_TRY(gridsum_prepare(r.c, nwg, 1, w.sums + kBicgBb, &gs0));
    PSK_HIP(hipMemsetAsync(w.st, 0, sizeof(BicgState), s));
    PSK_TRY(to_device_vec(b, loc, n, w.bv, s));
    PSK_HIP(hipMemsetAsync(w.x, 0, (size_t)n * 8, s));
    PSK_HIP(hipEventRecord(r.kit->ev0, s));
    hipLaunchKernelGGL(bicg_init_kernel, dim3((unsigned)nwg), dim3(kBlock), 0, s, n, trows, w.bv, gs0,
                       BicgInitFin{r.ctl->tau, r.ctl->norm_b, w.st, poll.hdone(), poll.hgen()});
    PSK_HIP(hipGetLastError());
    *run = true;
    if (r.gen) {
        // The preconditioner's kernels do not test `done`: they run in every iteration the host enqueues, also
        // behind the one that ended the solve. So they only ever see defined vectors: p_0 is stored (the other
        // paths read b), s starts at zero, and a b = 0 solve enqueues no iteration at all.
        PSK_HIP(hipMemcpyAsync(w.p, w.bv, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
        PSK_HIP(hipMemsetAsync(w.s, 0, (size_t)n * 8, s));
        PSK_TRY(poll.wait(s));
        *run = poll.stamp() == 0;
    }
    return PSK_OK;
}

// iteration k: [ph], S1, B, [sh], S2, D, E, F
static int bicg_iteration(BicgRun &r, int64_t k) {
    BicgWork &w = r.w;
    hipStream_t s = r.s;
    const int64_t n = r.n;
    const dim3 g((unsigned)r.nv), blk(kBlock);
    const int32_t *done = &w.st->done;
    // r_0 = p_0 = rhat = b: iteration 0 reads b in their place (general path: p_0 was copied, bicg_init)
    const double *rk = k == 0 ? w.bv : w.r, *pk = k == 0 && !r.gen ? w.bv : w.p;
    const int smode = r.dinv ? kSpmvJacobiDot : kSpmvPlainDot;
    if (r.gen) {
        PSK_TRY(prec_apply_dev(r.M, n, pk, w.ph, s));
        PSK_TRY(launch_spmv(r.A, kSpmvPlainDot, w.ph, w.v, nullptr, w.bv, w.sums + kBicgRv, done, s));
    } else {
        PSK_TRY(launch_spmv(r.A, smode, pk, w.v, r.dinv, w.bv, w.sums + kBicgRv, done, s));
    }
    hipLaunchKernelGGL(bicg_s_kernel, g, blk, 0, s, n, rk, w.v, w.s, w.sums + kBicgRv, r.gsB, w.st, w.hist, k);
    if (r.gen) {
        PSK_TRY(prec_apply_dev(r.M, n, w.s, w.sh, s));
        PSK_TRY(launch_spmv(r.A, kSpmvPlainDot, w.sh, w.t, nullptr, w.s, w.sums + kBicgTs, done, s));
    } else {
        PSK_TRY(launch_spmv(r.A, smode, w.s, w.t, r.dinv, w.s, w.sums + kBicgTs, done, s));
    }
    hipLaunchKernelGGL(bicg_tt_kernel, g, blk, 0, s, n, w.t, r.gsD, w.st);
    const int64_t maxiter = r.ctl->maxiter;
    const int32_t fom = r.ctl->fail_on_maxiter;
    if (r.gen)
        hipLaunchKernelGGL(bicg_xr_kernel<2>, g, blk, 0, s, n, w.x, w.ph, w.sh, w.s, w.t, w.bv, r.dinv, w.r,
                           w.sums + kBicgTs, r.gsE, w.st, w.hist, k, maxiter, fom);
    else if (r.dinv)
        hipLaunchKernelGGL(bicg_xr_kernel<1>, g, blk, 0, s, n, w.x, pk, (const double *)nullptr, w.s, w.t, w.bv, r.dinv,
                           w.r, w.sums + kBicgTs, r.gsE, w.st, w.hist, k, maxiter, fom);
    else
        hipLaunchKernelGGL(bicg_xr_kernel<0>, g, blk, 0, s, n, w.x, pk, (const double *)nullptr, w.s, w.t, w.bv, r.dinv,
                           w.r, w.sums + kBicgTs, r.gsE, w.st, w.hist, k, maxiter, fom);
    hipLaunchKernelGGL(bicg_p_kernel, g, blk, 0, s, n, w.r, pk, w.v, w.p, w.st);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// done by the tolerance test on a non-zero b: the exit whose true residual ||b - A x|| is measured and reported
static bool bicg_tol_exit(const BicgState &hs) { return hs.done == 1 && !hs.zero_b && hs.by_tol; }

// behind the loop: the state; what the exit left to do on the device (the half step's x += alpha ph, the true
// residual into *true_sq); the checks of the in-launch reductions and loop_ms
static int bicg_finish(BicgRun &r, BicgState *hs, double *true_sq, psk_result *res) {
    BicgWork &w = r.w;
    hipStream_t s = r.s;
    PSK_HIP(hipMemcpyAsync(hs, w.st, sizeof(*hs), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    if (hs->done == 1 && hs->half) {
        // general path: the iterations enqueued behind the exit recomputed ph from the same p (F returned), the
        // same bits
        hipLaunchKernelGGL(bicg_half_x_kernel, dim3((unsigned)r.nv), dim3(kBlock), 0, s, r.n, w.x,
                           r.gen ? w.ph : (hs->iters == 0 ? w.bv : w.p), r.gen ? nullptr : r.dinv, w.st);
        PSK_HIP(hipGetLastError());
    }
    *true_sq = 0.0;
    if (bicg_tol_exit(*hs)) {   // t is free by now
        PSK_TRY(launch_spmv(r.A, kSpmvResid, w.x, w.t, nullptr, w.bv, w.sums + kBicgTrue, nullptr, s));
        PSK_HIP(hipMemcpyAsync(true_sq, w.sums + kBicgTrue, 8, hipMemcpyDeviceToHost, s));
    }
    return solve_finish(r, res);
}

// SpMV launches of the loop that did their work (those enqueued behind `done` returned at once)
static int64_t bicg_spmv_count(const BicgState &hs, int64_t launched) {
    if (hs.done == 0) return 2 * launched;                      // still running: every enqueued iteration ran S1 and S2
    if (hs.zero_b) return 0;                                    // b = 0: the init raised `done`
    if (hs.half || hs.brk_kind == 1) return 2 * hs.iters + 1;   // B of iteration `iters` raised it: S2 returned at once
    return 2 * hs.iters + 2;                                    // E of iteration `iters` raised it: both had run
}

// The state hs of a finished loop that enqueued `launched` iterations, decoded into res; the history and x.
static int bicg_report(const BicgRun &r, const BicgState &hs, int64_t launched, double true_sq, psk_result *res,
                       double *hist, double *xout, int32_t loc) {
    res->norm_b = hs.normB;
    res->spmv_launches = bicg_spmv_count(hs, launched) + (bicg_tol_exit(hs) ? 1 : 0);   // + the true residual's
    res->resid_recursive = hs.rec;
    const char *brk = hs.brk_kind == 1   ? "breakdown dot(rhat,v)==0"
                      : hs.brk_kind == 2 ? "breakdown dot(t,t)==0"
                      : hs.brk_kind == 3 ? "breakdown omega==0"
                                         : "breakdown dot(rhat,r)==0";
    result_outcome({hs.zero_b, hs.done, hs.by_tol, hs.iters + 1, hs.iters, hs.rec, brk}, r.ctl->maxiter, res);
    if (bicg_tol_exit(hs)) result_true_resid("BiCGStab", std::sqrt(true_sq), hs.tauNormB, r.ctl->tau, hs.rec, true, res);
    return result_copy_out(r, hs.zero_b ? 0 : hs.nhist, r.w.hist, r.w.x, res, hist, xout, loc);
}

// the phases in order; the caller drains the stream when one fails
static int bicg_solve(BicgRun &r, const double *b, double *xout, psk_result *res, double *hist, int32_t loc) {
    PSK_TRY(bicg_workspace(r));
    PSK_TRY(solve_kit(r.c, false, &r.kit));
    StampPoll poll(r.kit);   // the host-mapped done stamp the kernels write (bicg_set_done)
    bool run;
    PSK_TRY(bicg_init(r, poll, b, loc, &run));
    int64_t launched = 0;
    if (run) PSK_TRY(poll_loop<2>(poll, r, r.ctl->maxiter, &launched, [&](int64_t k) { return bicg_iteration(r, k); }));
    BicgState hs;
    double true_sq;
    PSK_TRY(bicg_finish(r, &hs, &true_sq, res));
    return bicg_report(r, hs, launched, true_sq, res, hist, xout, loc);
}

}  // namespace psk

using namespace psk;

extern "C" int psk_bicgstab(const psk_csr *Ac, const psk_prec *M, const double *b, double *xout, const psk_ctl *ctl,
                            psk_result *res, double *hist, int32_t loc) {
    BicgRun r{};
    return solve_entry("psk_bicgstab", "BiCGStab", r, Ac, M, b, xout, ctl, res, 1, kVecTile, [&]() -> int {
        if (r.n == 0) {   // no rows: b = 0
            result_trivial(res);
            return PSK_OK;
        }
        return bicg_solve(r, b, xout, res, hist, loc);
    });
}
