// minres.hip — device-resident preconditioned MINRES for symmetric indefinite systems (no reference counterpart:
// the reference has PCG for SPD systems and GMRES for general ones).
//
// Paige-Saunders MINRES in the operation order of scipy.sparse.linalg.minres, with an SPD preconditioner M,
// x0 = 0, no shift, every elementwise operation rounded once (-ffp-contract=off):
//   r1 = b; z = M^-1 r1; beta1^2 = r1.z        (< 0: preconditioner not positive definite; == 0: b = 0 exit)
//   normB = sqrt(b.b) (or ctl->norm_b); scale = normB / beta1 (exactly 1 for the identity)
//   oldb = 0; beta = beta1; dbar = epsln = 0; phibar = beta1; cs = -1; sn = 0; w = w2 = 0; r2 = r1
//   k = 0, 1, ...:
//     s = 1/beta; v = s z
//     y = A v;  k >= 1: y = y - (beta/oldb) r1
//     alfa = v.y                                  (AFTER the r1 term: the stable ordering, and scipy's)
//     y = y - (alfa/beta) r2;  r1 = r2;  r2 = y;  z = M^-1 r2
//     oldb = beta;  beta^2 = r2.z  (< 0: preconditioner not positive definite);  beta = sqrt(.)
//     oldeps = epsln; delta = cs dbar + sn alfa; gbar = sn dbar - cs alfa; epsln = sn beta; dbar = -cs beta
//     gamma = sqrt(gbar^2 + beta^2)               (== 0: breakdown, singular system)
//     cs = gbar/gamma; sn = beta/gamma; phi = cs phibar; phibar = sn phibar
//     w1 = w2; w2 = w; w = (v - oldeps w1 - delta w2) (1/gamma);  x = x + phi w
//     hist[k] = scale phibar
//     hist[k] <= tau normB, or k == maxiter-1 and !fail_on_maxiter: stop
// phibar is ||r_k|| in the M^-1 norm, the quantity MINRES minimises; with the identity it is ||b - A x_k||_2.
// A Krylov space that is exhausted gives beta = 0, hence phibar = 0, and leaves by the ordinary test. b.z == 0 with
// b != 0 is refused like a negative b.z (M is not positive definite either way).
//
// Schedule built: one SpMV plus three launches per iteration for the identity and Jacobi preconditioners, all
// one-shot (one 512-element tile per workgroup, 16-B accesses), every dot finished in its own launch by the
// deterministic gridsum; vector bytes per row:
//   S   t = A v                                       launch_spmv, kSpmvPlain                    (the SpMV's)
//   U1  y = t - (beta/oldb) r1; alfa = sum v_i y_i                                               32 (24 at k = 0)
//   U2  r2' = y - (alfa/beta) r2 into r1's buffer (the r vectors rotate); beta^2 = r2'.z' with z' = DInv r2' in
//       registers; the finisher runs the whole rotation, the history entry, the test and the done stamp
//                                                                                                24 (32: Jacobi)
//   U3  w = (v - oldeps w1 - delta w2)/gamma over w1's buffer (w_k needs w_k-1 and w_k-2 only: a ring of two
//       buffers, the oldest overwritten element by element); x += phi w; the NEXT Lanczos vector v' = s' z' into the
//       other half of a ring of two v (z' = r2', or DInv r2' recomputed)                         64 (72: Jacobi)
// = 1 SpMV + 120 B/row (136 with Jacobi). The SpMV kernels are untouched.
// v IS stored (16 of those bytes). The cheaper schedule — SpMV on z, s folded into U1 as y = s (A z), U3 without
// the v' part: 104 B/row — computes the same thing in exact arithmetic but rounds y differently, and MINRES
// amplifies that like any other perturbation of the Lanczos vectors: restated on the CPU, its iterates leave
// scipy's by 1e-11 to 4e-5 (relative, in x) within 60 iterations on the 17^2 cases where the order kept here stays
// within 2e-15. The solver is pinned to scipy's iterates, so y = A v runs on the stored v.
// r1_0 and r2_0 are b: iteration 0 reads b in their place and nothing is copied; the init is [b.z, b.b] as one
// width-2 gridsum and one launch for v_0 = s z_0 once its finisher has beta1.
// The iteration whose finisher raises `done` still owes its w and x: its U3 is already enqueued behind it and
// runs on a live stamp (MinresState::owed names that iteration; it leaves v' alone); every other kernel enqueued
// behind `done` returns at once.
// General preconditioners (ILU, AMG, dense, Chebyshev): U2 only forms r2' (24 B/row), z' is materialised by
// prec_apply_dev and r2'.z' takes a dot launch of its own (16 B/row) with the same finisher; U3 reads the stored z'.
// Those apply kernels do not test `done`, so they only ever see defined vectors (the r ring starts at zero) and a
// solve the init ends (b = 0) enqueues no iteration.
// The solver scalars live in MinresState on the device and are advanced by thread 0 of the workgroup that completes
// a launch's gridsum; the host only enqueues and polls the done stamp (StampPoll). On a tolerance exit one
// kSpmvResid launch measures the true residual ||b - A x||_2.
#include "psk_internal.hpp"
#include "dist.hpp"
#include "solve_loop.hpp"

#include <cmath>
#include <cstdio>

namespace psk {

struct MinresState {
    int32_t done;      // 0 running, 1 converged, 2 breakdown
    int32_t brk_kind;  // 1: r.z < 0 (or b.z == 0 with b != 0), 2: gamma == 0
    int32_t by_tol;    // done by the tolerance test (not by k == maxiter-1 with !fail_on_maxiter)
    int32_t zero_b;    // b.b == 0
    int32_t at_init;   // `done` was raised by the init (b = 0, or M refused on b): no iteration ran
    int32_t pad;
    int64_t iters;     // the iteration k that raised `done` (0 for the init)
    int64_t nhist;     // history entries written
    int64_t owed;      // k + 1 of the iteration that raised done = 1: its U3 still runs (0: none)
    double normB, tauNormB, scale;
    double beta, oldb, dbar, epsln, phibar, cs, sn;    // the recurrence, as of the top of the next iteration
    double u_oldeps, u_delta, u_denom, u_phi;          // what U3 of the iteration just rotated reads
    double rec;        // the last reported residual (scale phibar)
    int64_t *hdone;    // host-mapped done stamp (solve_loop.hpp)
    int64_t hgen;      // this solve's generation in the stamp's high bits
};
static_assert(sizeof(MinresState) == 184, "tests/test_minres_cpu.py states this size");

// done = v != 0 and the stamp the host polls: k + 2 for a kernel of iteration k, 1 for the init
__device__ __forceinline__ void minres_set_done(MinresState *st, int32_t v, int64_t stamp) {
    st->done = v;
    done_stamp_store(st->hdone, st->hgen, stamp);
}
// at iteration k (k = -1: the init), with nhist entries written
__device__ __forceinline__ void minres_breakdown(MinresState *st, int32_t kind, int64_t k, int64_t nhist) {
    st->brk_kind = kind;
    st->at_init = k < 0;
    st->iters = k < 0 ? 0 : k;
    st->nhist = nhist;
    minres_set_done(st, 2, k + 2);
}

// ---- init: [b.z, b.b]; beta1, normB, scale, the b = 0 exit and the first refusal -------------------------------
struct MinresInitFin {
    double tau, normb_caller;
    MinresState *st;
    int64_t *hdone;
    int64_t hgen;
    __device__ void operator()(const double *r) const {
        const double bz = r[0], bb = r[1];
        const double nb = normb_caller > 0.0 ? normb_caller : sqrt(bb);
        st->normB = nb;
        st->tauNormB = tau * nb;
        st->rec = nb;
        st->hdone = hdone;
        st->hgen = hgen;
        if (bb == 0.0) {
            st->zero_b = 1;
            st->at_init = 1;
            minres_set_done(st, 1, 1);
            return;
        }
        if (bz <= 0.0) {
            minres_breakdown(st, 1, -1, 0);
            return;
        }
        const double beta1 = sqrt(bz);
        st->scale = nb / beta1;
        st->beta = beta1;
        st->phibar = beta1;
        st->cs = -1.0;   // oldb, dbar, epsln, sn: zero (the state was cleared)
    }
};
// MODE 0: identity (z = r); 1: Jacobi (z = DInv r, in registers); 2: general (z was materialised)
template <int MODE>
__global__ __launch_bounds__(kBlock) void minres_init_kernel(int64_t n, const double *__restrict__ b,
                                                             const double *__restrict__ dinv,
                                                             const double *__restrict__ z, GridSum gs,
                                                             MinresInitFin fin) {
    __shared__ double sh[2 * kWaves];
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    uint32_t ticket = 0;
    double bz = 0.0, bb = 0.0;
    if (i + 1 < n) {
        const dv2 bo = ld2(b + i);
        dv2 zo = bo;
        if (MODE == 1) {
            const dv2 d = ld2(dinv + i);
            zo.x = d.x * bo.x;
            zo.y = d.y * bo.y;
        }
        if (MODE == 2) zo = ld2(z + i);
        ticket = gridsum_ticket(gs);
        bz = fma(bo.x, zo.x, bz);
        bz = fma(bo.y, zo.y, bz);
        bb = fma(bo.x, bo.x, bb);
        bb = fma(bo.y, bo.y, bb);
    } else {
        ticket = gridsum_ticket(gs);
        if (i < n) {
            const double bi = b[i];
            double zi = bi;
            if (MODE == 1) zi = dinv[i] * bi;
            if (MODE == 2) zi = z[i];
            bz = bi * zi;
            bb = bi * bi;
        }
    }
    block_sum2(bz, bb, sh);
    const double v[2] = {bz, bb};
    gridsum_publish<2>(gs, v, sh, ticket, fin);
}

// v = s z for the z of r (MODE as above), s = 1 / st->beta: v_0 behind the init, and inside U3
template <int MODE>
__device__ __forceinline__ dv2 minres_v2(double s, dv2 r, const double *__restrict__ dinv,
                                         const double *__restrict__ z, int64_t i) {
    dv2 zo = r;
    if (MODE == 1) {
        const dv2 d = ld2(dinv + i);
        zo.x = d.x * r.x;
        zo.y = d.y * r.y;
    }
    if (MODE == 2) zo = ld2nt(z + i);
    dv2 v;
    v.x = s * zo.x;
    v.y = s * zo.y;
    return v;
}
template <int MODE>
__device__ __forceinline__ double minres_v1(double s, double r, const double *__restrict__ dinv,
                                            const double *__restrict__ z, int64_t i) {
    const double zi = MODE == 1 ? dinv[i] * r : MODE == 2 ? z[i] : r;
    return s * zi;
}
template <int MODE>
__global__ __launch_bounds__(kBlock) void minres_v0_kernel(int64_t n, const double *__restrict__ b,
                                                           const double *__restrict__ dinv,
                                                           const double *__restrict__ z, double *__restrict__ v,
                                                           const MinresState *st) {
    if (st->done) return;
    const double s = 1.0 / st->beta;
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    if (i + 1 < n)
        st2(v + i, minres_v2<MODE>(s, ld2(b + i), dinv, z, i));
    else if (i < n)
        v[i] = minres_v1<MODE>(s, b[i], dinv, z, i);
}

// ---- U1: y = t - (beta/oldb) r1 (FIRST: y = t); alfa = sum v_i y_i ----------------------------------------------
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void minres_y_kernel(int64_t n, const double *__restrict__ t,
                                                          const double *__restrict__ r1, const double *__restrict__ v,
                                                          double *__restrict__ y, GridSum gs, const MinresState *st) {
    if (st->done) return;
    const double c1 = FIRST ? 0.0 : st->beta / st->oldb;
    __shared__ double sh[kWaves];
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    uint32_t ticket = 0;
    double acc = 0.0;
    if (i + 1 < n) {
        const dv2 to = ld2nt(t + i), vo = ld2(v + i);
        dv2 yn = to;
        if (!FIRST) {
            const dv2 ro = ld2nt(r1 + i);
            yn.x = to.x - c1 * ro.x;
            yn.y = to.y - c1 * ro.y;
        }
        ticket = gridsum_ticket(gs);
        st2(y + i, yn);
        acc = fma(vo.x, yn.x, acc);
        acc = fma(vo.y, yn.y, acc);
    } else {
        ticket = gridsum_ticket(gs);
        if (i < n) {
            double yn = t[i];
            if (!FIRST) yn = yn - c1 * r1[i];
            y[i] = yn;
            acc = v[i] * yn;
        }
    }
    const double sum = block_sum(acc, sh);
    gridsum_publish<1>(gs, &sum, sh, ticket);
}

// ---- the rotation: everything scipy's loop body does between beta = inner(r2, y) and the stopping test --------
struct MinresRotFin {
    MinresState *st;
    double *hist;
    int64_t k, maxiter;
    int32_t fail_on_maxiter;
    double alfa;
    __device__ void operator()(const double *r) const {
        const double b2 = r[0];
        if (b2 < 0.0) {
            minres_breakdown(st, 1, k, k);
            return;
        }
        const double beta = sqrt(b2), oldb = st->beta;
        const double cs = st->cs, sn = st->sn, dbar = st->dbar;
        const double oldeps = st->epsln;
        const double delta = cs * dbar + sn * alfa;
        const double gbar = sn * dbar - cs * alfa;
        const double gamma = sqrt(gbar * gbar + beta * beta);
        if (gamma == 0.0) {
            minres_breakdown(st, 2, k, k);
            return;
        }
        st->epsln = sn * beta;
        st->dbar = -cs * beta;
        const double csn = gbar / gamma, snn = beta / gamma;
        const double phi = csn * st->phibar, phibar = snn * st->phibar;
        st->cs = csn;
        st->sn = snn;
        st->phibar = phibar;
        st->u_oldeps = oldeps;
        st->u_delta = delta;
        st->u_denom = 1.0 / gamma;
        st->u_phi = phi;
        st->oldb = oldb;
        st->beta = beta;
        const double h = st->scale * phibar;
        hist[k] = h;
        st->rec = h;
        st->nhist = k + 1;
        const bool tol = h <= st->tauNormB;
        if (tol || (k == maxiter - 1 && !fail_on_maxiter)) {
            st->by_tol = tol;
            st->iters = k;
            st->owed = k + 1;
            minres_set_done(st, 1, k + 2);
        }
    }
};

// ---- U2: r2' = y - (alfa/beta) r2; MODE 0: beta^2 = r2'.r2'; 1: beta^2 = r2'.(DInv r2'); 2: r2' only (no dot: gs
// is not used; the apply and minres_rz_kernel follow) ----------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(kBlock) void minres_r_kernel(int64_t n, const double *__restrict__ y,
                                                          const double *__restrict__ r2, double *__restrict__ rout,
                                                          const double *__restrict__ dinv,
                                                          const double *__restrict__ alfap, GridSum gs, MinresState *st,
                                                          double *__restrict__ hist, int64_t k, int64_t maxiter,
                                                          int32_t fail_on_maxiter) {
    if (st->done) return;
    const double alfa = *alfap;
    const double c2 = alfa / st->beta;
    __shared__ double sh[kWaves];
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    uint32_t ticket = 0;
    double acc = 0.0;
    if (i + 1 < n) {
        const dv2 yo = ld2nt(y + i), ro = ld2(r2 + i);
        dv2 rn;
        rn.x = yo.x - c2 * ro.x;
        rn.y = yo.y - c2 * ro.y;
        dv2 zn = rn;
        if (MODE == 1) {
            const dv2 d = ld2(dinv + i);
            zn.x = d.x * rn.x;
            zn.y = d.y * rn.y;
        }
        if (MODE != 2) ticket = gridsum_ticket(gs);
        st2(rout + i, rn);
        acc = fma(rn.x, zn.x, acc);
        acc = fma(rn.y, zn.y, acc);
    } else {
        if (MODE != 2) ticket = gridsum_ticket(gs);
        if (i < n) {
            const double rn = y[i] - c2 * r2[i];
            const double zn = MODE == 1 ? dinv[i] * rn : rn;
            rout[i] = rn;
            acc = rn * zn;
        }
    }
    if (MODE == 2) return;
    const double sum = block_sum(acc, sh);
    gridsum_publish<1>(gs, &sum, sh, ticket, MinresRotFin{st, hist, k, maxiter, fail_on_maxiter, alfa});
}

// ---- general preconditioners: beta^2 = r2'.z' behind the apply, with U2's finisher -------------------------------
__global__ __launch_bounds__(kBlock) void minres_rz_kernel(int64_t n, const double *__restrict__ r,
                                                           const double *__restrict__ z,
                                                           const double *__restrict__ alfap, GridSum gs, MinresState *st,
                                                           double *__restrict__ hist, int64_t k, int64_t maxiter,
                                                           int32_t fail_on_maxiter) {
    if (st->done) return;
    const double alfa = *alfap;
    __shared__ double sh[kWaves];
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    const uint32_t ticket = gridsum_ticket(gs);
    double acc = 0.0;
    if (i + 1 < n) {
        const dv2 ro = ld2(r + i), zo = ld2(z + i);
        acc = fma(ro.x, zo.x, acc);
        acc = fma(ro.y, zo.y, acc);
    } else if (i < n) {
        acc = r[i] * z[i];
    }
    const double sum = block_sum(acc, sh);
    gridsum_publish<1>(gs, &sum, sh, ticket, MinresRotFin{st, hist, k, maxiter, fail_on_maxiter, alfa});
}

// ---- U3: w = ((v - oldeps w1) - delta w2) (1/gamma) over w1; x = x + phi w; v' = s' z' for the next iteration
// (rn = r2', zn = its materialised z' for MODE 2). Runs while the solve runs and, on a live stamp and without the v'
// part, for the iteration that ended it (st->owed) ----------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(kBlock) void minres_wx_kernel(int64_t n, const double *__restrict__ v, double *w1,
                                                           const double *__restrict__ w2, double *__restrict__ x,
                                                           const double *__restrict__ rn,
                                                           const double *__restrict__ dinv,
                                                           const double *__restrict__ zn, double *__restrict__ vout,
                                                           const MinresState *st, int64_t k) {
    const bool live = !st->done;
    if (!live && st->owed != k + 1) return;
    const double oldeps = st->u_oldeps, delta = st->u_delta, denom = st->u_denom, phi = st->u_phi;
    const double s = 1.0 / st->beta;   // the NEW beta: v' belongs to iteration k + 1
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    if (i + 1 < n) {
        const dv2 vo = ld2nt(v + i), a = ld2nt(w1 + i), c = ld2(w2 + i), xo = ld2nt(x + i);
        dv2 wn, xn;
        wn.x = ((vo.x - oldeps * a.x) - delta * c.x) * denom;
        wn.y = ((vo.y - oldeps * a.y) - delta * c.y) * denom;
        xn.x = xo.x + phi * wn.x;
        xn.y = xo.y + phi * wn.y;
        st2(w1 + i, wn);
        st2nt(x + i, xn);
        if (live) st2(vout + i, minres_v2<MODE>(s, ld2(rn + i), dinv, zn, i));
    } else if (i < n) {
        const double wn = ((v[i] - oldeps * w1[i]) - delta * w2[i]) * denom;
        w1[i] = wn;
        x[i] = x[i] + phi * wn;
        if (live) vout[i] = minres_v1<MODE>(s, rn[i], dinv, zn, i);
    }
}

struct MinresWork {
    double *bv, *x, *y, *t, *r[2], *w[2], *v[2], *z;   // z: general preconditioners only (the apply's output)
    MinresState *st;
    double *sums, *hist;
};
constexpr int kMinresAlfa = 0, kMinresBeta2 = 1, kMinresBz = 2, kMinresTrue = 4;
// the layout of A->ws (big) and A->ws_small (sm): run on null-based carvers for the sizes, then on the buffers
static void minres_layout(Carve &big, Carve &sm, int64_t n, int64_t maxiter, bool gen, MinresWork &w) {
    const size_t vec = (size_t)n * 8;
    w.bv = big.take<double>(vec);
    w.x = big.take<double>(vec);
    w.y = big.take<double>(vec);
    w.t = big.take<double>(vec);
    for (int j = 0; j < 2; ++j) w.r[j] = big.take<double>(vec);
    for (int j = 0; j < 2; ++j) w.w[j] = big.take<double>(vec);
    for (int j = 0; j < 2; ++j) w.v[j] = big.take<double>(vec);
    w.z = gen ? big.take<double>(vec) : nullptr;
    w.st = sm.take<MinresState>(sizeof(MinresState));
    w.sums = sm.take<double>(8 * 8);   // alfa, beta^2, [b.z, b.b], ||b - A x||^2
    w.hist = sm.take<double>((size_t)(maxiter + 1) * 8);
}
void minres_layout_probe(int64_t n, int64_t maxiter, bool gen, std::vector<int64_t> *log, int64_t *bytes) {
    MinresWork w;
    layout_sizes([&](Carve &big, Carve &sm) { minres_layout(big, sm, n, maxiter, gen, w); }, kWsFloor, log, bytes);
}

// what the phases of one solve share
struct MinresRun : SolveRun {
    MinresWork w;
    GridSum gsA, gsB;   // alfa (U1), beta^2 (U2 or the general path's dot)
};

static int minres_workspace(MinresRun &r) {
    auto layout = [&](Carve &big, Carve &sm) { minres_layout(big, sm, r.n, r.ctl->maxiter, r.gen, r.w); };
    return workspace_carve(r.A, kWsFloor, true, layout, nullptr);
}

// the vectors iteration k reads and writes: r1_0 = r2_0 = b, r2_k = r[(k-1) % 2] and U2 writes r[k % 2], which held
// r1_k (k >= 2; r1_1 = b is kept); v_k = v[k % 2] and U3 writes v[(k+1) % 2]; w_k goes over w[k % 2]
static const double *minres_r2(const MinresWork &w, int64_t k) { return k == 0 ? w.bv : w.r[(k - 1) % 2]; }
static const double *minres_r1(const MinresWork &w, int64_t k) { return k == 1 ? w.bv : w.r[k % 2]; }

// everything in front of the loop: the gridsums, the state, b, x0 = w = 0, the init launch and v_0. *run: iterations
// may be enqueued (false: the stamp already says b = 0 or refuses M; only the general path waits to learn it)
static int minres_init(MinresRun &r, StampPoll &poll, const double *b, int32_t loc, bool *run) {
    MinresWork &w = r.w;
    hipStream_t s = r.s;
    const int64_t n = r.n;
    const size_t vec = (size_t)n * 8;
    GridSum gs0;
    PSK_TRY(gridsum_prepare(r.c, r.nv, 2, w.sums + kMinresBz, &gs0));
    PSK_TRY(gridsum_prepare(r.c, r.nv, 1, w.sums + kMinresAlfa, &r.gsA));
    PSK_TRY(gridsum_prepare(r.c, r.nv, 1, w.sums + kMinresBeta2, &r.gsB));
    PSK_HIP(hipMemsetAsync(w.st, 0, sizeof(MinresState), s));
    PSK_TRY(to_device_vec(b, loc, n, w.bv, s));
    PSK_HIP(hipMemsetAsync(w.x, 0, vec, s));
    PSK_HIP(hipMemsetAsync(w.w[0], 0, vec, s));
    PSK_HIP(hipMemsetAsync(w.w[1], 0, vec, s));
    PSK_HIP(hipEventRecord(r.kit->ev0, s));
    const dim3 g((unsigned)r.nv), blk(kBlock);
    const MinresInitFin fin{r.ctl->tau, r.ctl->norm_b, w.st, poll.hdone(), poll.hgen()};
    *run = true;
    if (r.gen) {
        // The preconditioner's kernels do not test `done`: they run in every iteration the host enqueues, also
        // behind the one that ended the solve. So they only ever see defined vectors (the r ring starts at zero),
        // and a solve the init ends enqueues no iteration at all.
        PSK_HIP(hipMemsetAsync(w.r[0], 0, vec, s));
        PSK_HIP(hipMemsetAsync(w.r[1], 0, vec, s));
        PSK_TRY(prec_apply_dev(r.M, n, w.bv, w.z, s));
        hipLaunchKernelGGL(minres_init_kernel<2>, g, blk, 0, s, n, w.bv, r.dinv, w.z, gs0, fin);
        hipLaunchKernelGGL(minres_v0_kernel<2>, g, blk, 0, s, n, w.bv, r.dinv, w.z, w.v[0], w.st);
        PSK_HIP(hipGetLastError());
        PSK_TRY(poll.wait(s));
        *run = poll.stamp() == 0;
        return PSK_OK;
    }
    if (r.dinv) {
        hipLaunchKernelGGL(minres_init_kernel<1>, g, blk, 0, s, n, w.bv, r.dinv, w.z, gs0, fin);
        hipLaunchKernelGGL(minres_v0_kernel<1>, g, blk, 0, s, n, w.bv, r.dinv, w.z, w.v[0], w.st);
    } else {
        hipLaunchKernelGGL(minres_init_kernel<0>, g, blk, 0, s, n, w.bv, r.dinv, w.z, gs0, fin);
        hipLaunchKernelGGL(minres_v0_kernel<0>, g, blk, 0, s, n, w.bv, r.dinv, w.z, w.v[0], w.st);
    }
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// iteration k: S, U1, U2, [apply, dot], U3
static int minres_iteration(MinresRun &r, int64_t k) {
    MinresWork &w = r.w;
    hipStream_t s = r.s;
    const int64_t n = r.n;
    const dim3 g((unsigned)r.nv), blk(kBlock);
    const double *vk = w.v[k % 2], *r2 = minres_r2(w, k);
    double *rout = w.r[k % 2], *vout = w.v[(k + 1) % 2], *w1 = w.w[k % 2];
    const double *w2 = w.w[(k + 1) % 2], *alfap = w.sums + kMinresAlfa;
    const int64_t maxiter = r.ctl->maxiter;
    const int32_t fom = r.ctl->fail_on_maxiter;
    PSK_TRY(launch_spmv(r.A, kSpmvPlain, vk, w.t, nullptr, nullptr, nullptr, &w.st->done, s));
    if (k == 0)
        hipLaunchKernelGGL(minres_y_kernel<true>, g, blk, 0, s, n, w.t, (const double *)nullptr, vk, w.y, r.gsA, w.st);
    else
        hipLaunchKernelGGL(minres_y_kernel<false>, g, blk, 0, s, n, w.t, minres_r1(w, k), vk, w.y, r.gsA, w.st);
    if (r.gen) {
        hipLaunchKernelGGL(minres_r_kernel<2>, g, blk, 0, s, n, w.y, r2, rout, r.dinv, alfap, r.gsB, w.st, w.hist, k,
                           maxiter, fom);
        PSK_HIP(hipGetLastError());
        PSK_TRY(prec_apply_dev(r.M, n, rout, w.z, s));
        hipLaunchKernelGGL(minres_rz_kernel, g, blk, 0, s, n, rout, w.z, alfap, r.gsB, w.st, w.hist, k, maxiter, fom);
        hipLaunchKernelGGL(minres_wx_kernel<2>, g, blk, 0, s, n, vk, w1, w2, w.x, rout, r.dinv, w.z, vout, w.st, k);
    } else if (r.dinv) {
        hipLaunchKernelGGL(minres_r_kernel<1>, g, blk, 0, s, n, w.y, r2, rout, r.dinv, alfap, r.gsB, w.st, w.hist, k,
                           maxiter, fom);
        hipLaunchKernelGGL(minres_wx_kernel<1>, g, blk, 0, s, n, vk, w1, w2, w.x, rout, r.dinv, w.z, vout, w.st, k);
    } else {
        hipLaunchKernelGGL(minres_r_kernel<0>, g, blk, 0, s, n, w.y, r2, rout, r.dinv, alfap, r.gsB, w.st, w.hist, k,
                           maxiter, fom);
        hipLaunchKernelGGL(minres_wx_kernel<0>, g, blk, 0, s, n, vk, w1, w2, w.x, rout, r.dinv, w.z, vout, w.st, k);
    }
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// done by the tolerance test on a non-zero b: the exit whose true residual ||b - A x|| is measured and reported
static bool minres_tol_exit(const MinresState &hs) { return hs.done == 1 && !hs.zero_b && hs.by_tol; }

// behind the loop: the state; on a tolerance exit the true residual into *true_sq; the checks of the in-launch
// reductions and loop_ms
static int minres_finish(MinresRun &r, MinresState *hs, double *true_sq, psk_result *res) {
    MinresWork &w = r.w;
    hipStream_t s = r.s;
    PSK_HIP(hipMemcpyAsync(hs, w.st, sizeof(*hs), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    *true_sq = 0.0;
    if (minres_tol_exit(*hs)) {   // y is free by now
        PSK_TRY(launch_spmv(r.A, kSpmvResid, w.x, w.y, nullptr, w.bv, w.sums + kMinresTrue, nullptr, s));
        PSK_HIP(hipMemcpyAsync(true_sq, w.sums + kMinresTrue, 8, hipMemcpyDeviceToHost, s));
    }
    return solve_finish(r, res);
}

// SpMV launches of the loop that did their work (those enqueued behind `done` returned at once): `done` is only
// ever raised by the init or behind the SpMV of iteration `iters`
static int64_t minres_spmv_count(const MinresState &hs, int64_t launched) {
    if (hs.done == 0) return launched;
    return hs.at_init ? 0 : hs.iters + 1;
}

// The state hs of a finished loop that enqueued `launched` iterations, decoded into res; the history and x.
static int minres_report(const MinresRun &r, const MinresState &hs, int64_t launched, double true_sq, psk_result *res,
                         double *hist, double *xout, int32_t loc) {
    res->norm_b = hs.normB;
    res->spmv_launches = minres_spmv_count(hs, launched) + (minres_tol_exit(hs) ? 1 : 0);   // + the true residual's
    res->resid_recursive = hs.rec;
    const char *brk = hs.brk_kind == 1 ? "preconditioner not positive definite" : "breakdown gamma==0";
    result_outcome({hs.zero_b, hs.done, hs.by_tol, hs.iters + 1, hs.iters, hs.rec, brk}, r.ctl->maxiter, res);
    // Under a preconditioner the test was made in the M^-1 norm, which is the solve's contract:
    // ||r||_2 / ||b||_2 <= sqrt(cond(M)) tau, and the status stays converged.
    if (minres_tol_exit(hs))
        result_true_resid("MINRES", std::sqrt(true_sq), hs.tauNormB, r.ctl->tau, hs.rec, !r.gen && !r.dinv, res);
    return result_copy_out(r, hs.zero_b ? 0 : hs.nhist, r.w.hist, r.w.x, res, hist, xout, loc);
}

// the phases in order; the caller drains the stream when one fails
static int minres_solve(MinresRun &r, const double *b, double *xout, psk_result *res, double *hist, int32_t loc) {
    PSK_TRY(minres_workspace(r));
    PSK_TRY(solve_kit(r.c, false, &r.kit));
    StampPoll poll(r.kit);   // the host-mapped done stamp the kernels write (minres_set_done)
    bool run;
    PSK_TRY(minres_init(r, poll, b, loc, &run));
    int64_t launched = 0;
    if (run) PSK_TRY(poll_loop<2>(poll, r, r.ctl->maxiter, &launched, [&](int64_t k) { return minres_iteration(r, k); }));
    MinresState hs;
    double true_sq;
    PSK_TRY(minres_finish(r, &hs, &true_sq, res));
    return minres_report(r, hs, launched, true_sq, res, hist, xout, loc);
}

}  // namespace psk

using namespace psk;

extern "C" int psk_minres(const psk_csr *Ac, const psk_prec *M, const double *b, double *xout, const psk_ctl *ctl,
                          psk_result *res, double *hist, int32_t loc) {
    MinresRun r{};
    return solve_entry("psk_minres", "MINRES", r, Ac, M, b, xout, ctl, res, 1, kVecTile, [&]() -> int {
        if (r.n == 0) {   // no rows: b = 0
            result_trivial(res);
            return PSK_OK;
        }
        return minres_solve(r, b, xout, res, hist, loc);
    });
}
