// idrs.hip — device-resident right-preconditioned IDR(s) (Sonneveld and van Gijzen) for nonsymmetric systems: the
// biorthogonal variant with the orthogonalisation of each new direction done from ONE s-wide dot product (Collignon
// and van Gijzen's minimal-synchronisation form). No reference counterpart: this header and tests/idrs_oracle.py are
// the definition.
//
// The recurrence, every elementwise operation rounded once (-ffp-contract=off), x0 = 0, 1 <= s <= PSK_IDRS_MAX_S. One
// STEP is one SpMV; hist, iters and maxiter count steps.
//   P (n x s), never stored: P[i][j] = double(splitmix64(i*s + j) >> 11) * 2^-52 - 1.0 (exact in f64; idrs_shadow)
//   x = 0; r = b; normB = sqrt(b.b) (or ctl->norm_b); thr = tau normB; G = U = 0 (n x s); Mm = I_s; om = 1; j = 0
//   cycle:
//     f_i = p_i.r, i = 0..s-1
//     for k = 0..s-1:
//       c_i, i = k..s-1:  t = f_i;  t = t - Mm[i][l] c_l, l = k..i-1;  c_i = t / Mm[i][i]
//       v = r;  v = v - c_i g_i, i = k..s-1;  v = M^-1 v;  u = om v;  u = u + c_i u_i, i = k..s-1
//       g = A u                                                                   (step j's SpMV)
//       q_i = p_i.g, i = 0..s-1
//       a_i, i = 0..k-1:  t = q_i;  t = t - Mm[i][l] a_l, l = 0..i-1;  a_i = t / Mm[i][i]
//       g = g - a_i g_i, u = u - a_i u_i, i = 0..k-1;  g_k = g;  u_k = u
//       Mm[i][k], i = k..s-1:  t = q_i;  t = t - Mm[i][l] a_l, l = 0..k-1;  Mm[i][k] = t
//       Mm[k][k] == 0: breakdown
//       beta = f_k / Mm[k][k];  r = r - beta g;  x = x + beta u;  hist[j] = sqrt(r.r);  stop test;  j++
//       f_i = f_i - beta Mm[i][k], i = k+1..s-1
//     v = M^-1 r;  t = A v                                                        (step j's SpMV)
//     tt = t.t;  ts = t.r;  rr = the r.r of the previous step;  tt == 0 or ts == 0: breakdown
//     rho = ts / (sqrt(tt) sqrt(rr));  om = ts / tt;  |rho| < 0.7: om = (om 0.7) / |rho|
//     x = x + om v;  r = r - om t;  hist[j] = sqrt(r.r);  stop test;  j++
//   stop test: hist[j] <= thr, or j == maxiter-1 with !fail_on_maxiter.
//
// Schedule built. Every vector kernel is one-shot (one 512-element tile per workgroup, 16-B accesses); every dot
// product is a deterministic gridsum finished inside its own launch, and the small triangular solves run in the `fin`
// of the gridsum that produced their inputs (one lane of the finishing wave, Mm and the scalars held in registers).
// The scalars f, c, a, Mm, om, beta, the flags and the history live in IdrsState on the device; the host only
// enqueues steps and polls the done stamp (StampPoll); every kernel enqueued after `done` returns at once.
// Launches and vector bytes per row of an inner step k (identity; Jacobi streams DInv too):
//   F   (k = 0 only) f = P^T r as ONE s-wide gridsum; fin: c for k = 0                           8
//   V   v = r - sum c_i g_i; M^-1 v (identity / Jacobi in registers); u = om v + sum c_i u_i     16 + 16 (s - k) (+8: DInv)
//   S   g = A u                          launch_spmv, kSpmvPlain, untouched                      (the SpMV's)
//   Q   q = P^T g as ONE s-wide gridsum; fin: a, column k of Mm, the breakdown test, beta        8
//   U   g, u made orthogonal (a_i); g_k, u_k stored; r, x updated; r.r in the epilogue;
//       fin: history, stop test, the done stamp, f, and c for k + 1                              64 + 16 k
//       (Jacobi, k = s-1: + 16, it also stores M^-1 r for the omega step's SpMV)
// = 4 launches (5 at k = 0) and 1 SpMV + 88 + 16 s B/row whatever k (+8 at k = 0, +8 Jacobi). The omega step:
//   S   t = A M^-1 r                     kSpmvPlain on r (identity) or on the stored M^-1 r      (the SpMV's)
//   T   [t.t, t.r] as one width-2 gridsum; fin: the breakdown tests, rho, om                     16
//   W   x = x + om v; r = r - om t; r.r; fin: history, stop test, the done stamp                 40 (+8: v is stored)
// = 3 launches and 1 SpMV + 56 B/row. A cycle of s + 1 SpMVs moves s (88 + 16 s) + 64 B/row: 134 B/row per SpMV at
// s = 4, 199 at s = 8 (BiCGStab: 60).
// beta depends on a, and both are finished in Q's fin: U reads them as scalars and stays ONE pass.
// P is regenerated from the hash in registers by F and Q instead of being stored: a stored P costs 8 s B/row in each
// of the two passes (64 B/row at s = 8 against the 8 B/row they read otherwise) and s more vectors of footprint; the
// hash is two 64-bit multiplies and a conversion per entry and reads nothing.
// The SpMV carries no dot here (its tiles differ between layouts; t.r is summed in T over the vector tiles), so all
// SpMV layouts give the same bits.
// General preconditioners (ILU, AMG, dense, Chebyshev, FSAI, multicolour GS): V is split around prec_apply_dev (v
// stored, M^-1 v applied, then u formed: +24 B/row and two launches more), and the omega step applies it to r.
#include "psk_internal.hpp"
#include "dist.hpp"
#include "solve_loop.hpp"

#include <cmath>
#include <cstdio>

namespace psk {

constexpr int kIdrsS = PSK_IDRS_MAX_S;
static_assert(kIdrsS <= kGridSumMaxW, "P^T r and P^T g are one grid sum of width s");

struct IdrsState {
    int32_t done;      // 0 running, 1 stopped, 2 breakdown
    int32_t brk_kind;  // 1: Mm[k][k] == 0, 2: t.t == 0, 3: t.r == 0
    int32_t by_tol;    // stopped by the tolerance test (not by j == maxiter-1 with !fail_on_maxiter)
    int32_t zero_b;    // b.b == 0
    int64_t iters;     // the step j that raised `done`
    int64_t nhist;     // history entries written
    double normB, tauNormB;
    double om, beta;
    double rr;         // r.r of the last step
    double rec;        // the last reported recursive residual
    double f[kIdrsS], c[kIdrsS], a[kIdrsS];
    double Mm[kIdrsS * kIdrsS];   // row-major, stride kIdrsS; the identity outside s x s
    int64_t *hdone;    // host-mapped done stamp (solve_loop.hpp)
    int64_t hgen;      // this solve's generation in the stamp's high bits
};

// done = v != 0 and the stamp the host polls: j + 2 for a kernel of step j, 1 for the init
__device__ __forceinline__ void idrs_set_done(IdrsState *st, int32_t v, int64_t stamp) {
    st->done = v;
    done_stamp_store(st->hdone, st->hgen, stamp);
}
__device__ __forceinline__ void idrs_breakdown(IdrsState *st, int32_t kind, int64_t j) {
    st->brk_kind = kind;
    st->iters = j;
    st->nhist = j;
    idrs_set_done(st, 2, j + 2);
}

// P[i][j] at t = i*s + j: splitmix64's output, its top 53 bits scaled into [-1, 1). Every operation is exact.
__device__ __forceinline__ double idrs_shadow(uint64_t t) {
    uint64_t z = t + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * 0x1.0p-52 - 1.0;
}

// elements i, i + 1 of a vector of n (i even): one 16-B access inside the vector, zeros past its end
__device__ __forceinline__ dv2 idrs_ld(const double *p, int64_t i, int64_t n) {
    if (i + 1 < n) return ld2(p + i);
    dv2 v;
    v.x = i < n ? p[i] : 0.0;
    v.y = 0.0;
    return v;
}
__device__ __forceinline__ void idrs_st(double *p, int64_t i, int64_t n, dv2 v) {
    if (i + 1 < n)
        st2(p + i, v);
    else if (i < n)
        p[i] = v.x;
}

// The W sums of this workgroup's tile (per-lane partials in acc) into the launch's gridsum; fin runs in one lane of
// the wave that finished the grid sums. ticket: idrs_ticket's, drawn once the tile's loads were issued.
__device__ __forceinline__ uint32_t idrs_ticket(const GridSum &gs) {
    uint32_t t = 0;
    if (gs.grp_log2 >= 0 && threadIdx.x == 0)
        t = gridsum_draw(gridsum_counter(gs, gridsum_group_of((int64_t)blockIdx.x, gs.grp_log2)));
    return t;
}
template <int W, class F>
__device__ __forceinline__ void idrs_publish(const GridSum &gs, const double (&acc)[W], uint32_t ticket, const F &fin) {
    __shared__ GridSumTile<W> gsl[1];
    const int64_t tl[1] = {(int64_t)blockIdx.x};
    const bool tv[1] = {true};
    const uint32_t tk[1] = {ticket};
    if (threadIdx.x == 0) {
        gsl[0].cnt = 0;
        if (gridDim.x != gs.nt) atomicOr(gs.err, 2);
    }
    __syncthreads();
    gridsum_tiles_publish<1, W>(gs, gsl, &acc, tk, tl, tv, fin);
}

// ---- init: b.b; normB, thr, om = 1, Mm = I, the b = 0 exit ---------------------------------------------------------
struct IdrsInitFin {
    double tau, normb_caller;
    IdrsState *st;
    int64_t *hdone;
    int64_t hgen;
    __device__ void operator()(const double *r) const {
        const double bb = r[0];
        const double nb = normb_caller > 0.0 ? normb_caller : sqrt(bb);
        st->normB = nb;
        st->tauNormB = tau * nb;
        st->rec = nb;
        st->rr = bb;
        st->om = 1.0;
        for (int i = 0; i < kIdrsS; ++i) st->Mm[i * kIdrsS + i] = 1.0;   // the state was zeroed
        st->hdone = hdone;
        st->hgen = hgen;
        if (bb == 0.0) {
            st->zero_b = 1;
            idrs_set_done(st, 1, 1);
        }
    }
};
__global__ __launch_bounds__(kBlock) void idrs_init_kernel(int64_t n, const double *__restrict__ b, GridSum gs,
                                                           IdrsInitFin fin) {
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    const dv2 bv = idrs_ld(b, i, n);
    const uint32_t ticket = idrs_ticket(gs);
    double acc[1];
    acc[0] = bv.x * bv.x;
    acc[0] = acc[0] + bv.y * bv.y;
    idrs_publish<1>(gs, acc, ticket, fin);
}

// ---- F and Q: P^T w as ONE S-wide gridsum, P from the hash ----------------------------------------------------------
// F's fin (w = r, the head of a cycle): f = P^T r and c for k = 0
template <int S>
struct IdrsCycleFin {
    IdrsState *st;
    __device__ void operator()(const double *q) const {
        double M[S][S], c[S];
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int l = 0; l <= i; ++l) M[i][l] = st->Mm[i * kIdrsS + l];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            double t = q[i];
#pragma unroll
            for (int l = 0; l < i; ++l) t = t - M[i][l] * c[l];
            c[i] = t / M[i][i];
            st->f[i] = q[i];
            st->c[i] = c[i];
        }
    }
};
// Q's fin (w = g = A u of inner step k, step j): a, column k of Mm, the breakdown test, beta
template <int S>
struct IdrsOrthFin {
    IdrsState *st;
    int k;
    int64_t j;
    __device__ void operator()(const double *q) const {
        double M[S][S], a[S];
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int l = 0; l < S; ++l) M[i][l] = st->Mm[i * kIdrsS + l];
        const double fk = st->f[k];
        double mkk = 0.0;
#pragma unroll
        for (int i = 0; i < S; ++i) {
            double t = q[i];
            if (i < k) {
#pragma unroll
                for (int l = 0; l < i; ++l) t = t - M[i][l] * a[l];
                a[i] = t / M[i][i];
                st->a[i] = a[i];
            } else {
#pragma unroll
                for (int l = 0; l < i; ++l)
                    if (l < k) t = t - M[i][l] * a[l];
                a[i] = 0.0;
                st->Mm[i * kIdrsS + k] = t;
                if (i == k) mkk = t;
            }
        }
        if (mkk == 0.0) {
            idrs_breakdown(st, 1, j);
            return;
        }
        st->beta = fk / mkk;
    }
};
template <int S, class Fin>
__global__ __launch_bounds__(kBlock) void idrs_pdot_kernel(int64_t n, const double *__restrict__ w, GridSum gs,
                                                           const IdrsState *st, Fin fin) {
    if (st->done) return;
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    const dv2 wv = idrs_ld(w, i, n);   // zeros past the end: those rows add +-0
    const uint32_t ticket = idrs_ticket(gs);
    double acc[S];
    const uint64_t t0 = (uint64_t)i * S;
#pragma unroll
    for (int c = 0; c < S; ++c) {
        acc[c] = idrs_shadow(t0 + c) * wv.x;
        acc[c] = acc[c] + idrs_shadow(t0 + S + c) * wv.y;
    }
    idrs_publish<S>(gs, acc, ticket, fin);
}

// ---- V: v = r - sum c_i g_i; M^-1 v; u = om v + sum c_i u_i (i = k..s-1) --------------------------------------------
// MODE 0: identity; 1: Jacobi (DInv streamed); 2: general, first half: out = v; 3: general, second half: vh = M^-1 v
// was materialised, out = u
template <int MODE>
__global__ __launch_bounds__(kBlock) void idrs_v_kernel(int64_t n, const double *__restrict__ r,
                                                        const double *__restrict__ vh, const double *__restrict__ G,
                                                        const double *__restrict__ U, int64_t ld, int s, int k,
                                                        const double *__restrict__ dinv, double *__restrict__ out,
                                                        const IdrsState *__restrict__ st) {
    if (st->done) return;
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    if (i >= n) return;
    dv2 v;
    if (MODE != 3) {
        v = idrs_ld(r, i, n);
#pragma unroll 4
        for (int q = k; q < s; ++q) {
            const double cq = st->c[q];
            const dv2 g = idrs_ld(G + q * ld, i, n);
            v.x = v.x - cq * g.x;
            v.y = v.y - cq * g.y;
        }
        if (MODE == 2) {
            idrs_st(out, i, n, v);
            return;
        }
        if (MODE == 1) {
            const dv2 d = idrs_ld(dinv, i, n);
            v.x = d.x * v.x;
            v.y = d.y * v.y;
        }
    } else {
        v = idrs_ld(vh, i, n);
    }
    const double om = st->om;
    dv2 u;
    u.x = om * v.x;
    u.y = om * v.y;
#pragma unroll 4
    for (int q = k; q < s; ++q) {
        const double cq = st->c[q];
        const dv2 uq = idrs_ld(U + q * ld, i, n);
        u.x = u.x + cq * uq.x;
        u.y = u.y + cq * uq.y;
    }
    idrs_st(out, i, n, u);
}

// ---- U and W: r, x updated, r.r; fin: history, stop test, f and the next c --------------------------------------------
// the end of step j; k = the inner step (s for the omega step: nothing of f or c is left to do)
struct IdrsStepFin {
    IdrsState *st;
    double *hist;
    int64_t j, maxiter;
    int32_t fail_on_maxiter;
    int k, s;
    __device__ void operator()(const double *r) const {
        const double rr = r[0], nr = sqrt(rr);
        hist[j] = nr;
        st->rec = nr;
        st->rr = rr;
        st->nhist = j + 1;
        const bool tol = nr <= st->tauNormB;
        if (tol || (j == maxiter - 1 && !fail_on_maxiter)) {
            st->by_tol = tol;
            st->iters = j;
            idrs_set_done(st, 1, j + 2);
            return;
        }
        if (k + 1 >= s) return;
        // f_i = f_i - beta Mm[i][k], i > k; then c for k + 1. The loops are unrolled to kIdrsS and guarded by k and s,
        // so Mm, f and c stay in registers
        const double beta = st->beta;
        double M[kIdrsS][kIdrsS], f[kIdrsS], c[kIdrsS];
#pragma unroll
        for (int i = 0; i < kIdrsS; ++i) {
            f[i] = st->f[i];
            c[i] = 0.0;
#pragma unroll
            for (int l = 0; l <= i; ++l) M[i][l] = st->Mm[i * kIdrsS + l];
        }
#pragma unroll
        for (int i = 1; i < kIdrsS; ++i) {
            if (i <= k || i >= s) continue;
            double mik = 0.0;
#pragma unroll
            for (int l = 0; l < i; ++l)
                if (l == k) mik = M[i][l];
            f[i] = f[i] - beta * mik;
            double t = f[i];
#pragma unroll
            for (int l = 1; l < i; ++l)
                if (l > k) t = t - M[i][l] * c[l];
            c[i] = t / M[i][i];
            st->f[i] = f[i];
            st->c[i] = c[i];
        }
    }
};
// U. VH: also vh = DInv r (Jacobi, k = s-1: the omega step's SpMV reads it)
template <bool VH>
__global__ __launch_bounds__(kBlock) void idrs_gu_kernel(int64_t n, const double *__restrict__ gw,
                                                         const double *__restrict__ uw, double *G, double *U, int64_t ld,
                                                         int k, double *__restrict__ r, double *__restrict__ x,
                                                         const double *__restrict__ dinv, double *__restrict__ vh,
                                                         GridSum gs, IdrsState *st, IdrsStepFin fin) {
    if (st->done) return;
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    dv2 g = idrs_ld(gw, i, n), u = idrs_ld(uw, i, n);
    const dv2 ro = idrs_ld(r, i, n), xo = idrs_ld(x, i, n);
    const uint32_t ticket = idrs_ticket(gs);
#pragma unroll 4
    for (int q = 0; q < k; ++q) {
        const double aq = st->a[q];
        const dv2 gq = idrs_ld(G + q * ld, i, n), uq = idrs_ld(U + q * ld, i, n);
        g.x = g.x - aq * gq.x;
        g.y = g.y - aq * gq.y;
        u.x = u.x - aq * uq.x;
        u.y = u.y - aq * uq.y;
    }
    const double beta = st->beta;
    dv2 rn, xn;
    rn.x = ro.x - beta * g.x;
    rn.y = ro.y - beta * g.y;
    xn.x = xo.x + beta * u.x;
    xn.y = xo.y + beta * u.y;
    idrs_st(G + k * ld, i, n, g);
    idrs_st(U + k * ld, i, n, u);
    idrs_st(r, i, n, rn);
    idrs_st(x, i, n, xn);
    if (VH) {
        const dv2 d = idrs_ld(dinv, i, n);
        dv2 h;
        h.x = d.x * rn.x;
        h.y = d.y * rn.y;
        idrs_st(vh, i, n, h);
    }
    double acc[1];
    acc[0] = rn.x * rn.x;
    acc[0] = acc[0] + rn.y * rn.y;
    idrs_publish<1>(gs, acc, ticket, fin);
}

// T: [t.t, t.r]; fin: the breakdown tests, rho, om
struct IdrsOmegaFin {
    IdrsState *st;
    int64_t j;
    __device__ void operator()(const double *r) const {
        const double tt = r[0], ts = r[1];
        if (tt == 0.0 || ts == 0.0) {
            idrs_breakdown(st, tt == 0.0 ? 2 : 3, j);
            return;
        }
        const double rho = ts / (sqrt(tt) * sqrt(st->rr));
        double om = ts / tt;
        if (fabs(rho) < 0.7) om = (om * 0.7) / fabs(rho);
        st->om = om;
    }
};
__global__ __launch_bounds__(kBlock) void idrs_tt_kernel(int64_t n, const double *__restrict__ t,
                                                         const double *__restrict__ r, GridSum gs, const IdrsState *st,
                                                         IdrsOmegaFin fin) {
    if (st->done) return;
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    const dv2 tv = idrs_ld(t, i, n), rv = idrs_ld(r, i, n);
    const uint32_t ticket = idrs_ticket(gs);
    double acc[2];
    acc[0] = tv.x * tv.x;
    acc[0] = acc[0] + tv.y * tv.y;
    acc[1] = tv.x * rv.x;
    acc[1] = acc[1] + tv.y * rv.y;
    idrs_publish<2>(gs, acc, ticket, fin);
}
// W: x = x + om v; r = r - om t; r.r. v: the stored M^-1 r, or null for the identity (v = r)
__global__ __launch_bounds__(kBlock) void idrs_w_kernel(int64_t n, const double *__restrict__ v,
                                                        const double *__restrict__ t, double *__restrict__ r,
                                                        double *__restrict__ x, GridSum gs, IdrsState *st,
                                                        IdrsStepFin fin) {
    if (st->done) return;
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    const dv2 ro = idrs_ld(r, i, n), xo = idrs_ld(x, i, n), to = idrs_ld(t, i, n);
    const dv2 vo = v ? idrs_ld(v, i, n) : ro;
    const uint32_t ticket = idrs_ticket(gs);
    const double om = st->om;
    dv2 rn, xn;
    xn.x = xo.x + om * vo.x;
    xn.y = xo.y + om * vo.y;
    rn.x = ro.x - om * to.x;
    rn.y = ro.y - om * to.y;
    idrs_st(x, i, n, xn);
    idrs_st(r, i, n, rn);
    double acc[1];
    acc[0] = rn.x * rn.x;
    acc[0] = acc[0] + rn.y * rn.y;
    idrs_publish<1>(gs, acc, ticket, fin);
}

struct IdrsWork {
    double *bv, *x, *r, *uw, *gw, *vh, *vv;   // vh: Jacobi and general; vv: general only
    double *G, *U;                            // s columns of stride ld each
    int64_t ld;
    IdrsState *st;
    double *sums, *hist;
};
constexpr int kIdrsPd = 0, kIdrsTt = 8, kIdrsRr = 10, kIdrsBb = 11, kIdrsTrue = 12;
// the layout of A->ws (big) and A->ws_small (sm): run on null-based carvers for the sizes, then on the buffers
static void idrs_layout(Carve &big, Carve &sm, int64_t n, int64_t maxiter, int s, bool gen, bool jac, IdrsWork &w) {
    const size_t vec = (size_t)n * 8;
    w.ld = (n + 31) / 32 * 32;   // columns start on 256-B lines
    w.bv = big.take<double>(vec);
    w.x = big.take<double>(vec);
    w.r = big.take<double>(vec);
    w.uw = big.take<double>(vec);
    w.gw = big.take<double>(vec);
    w.vh = gen || jac ? big.take<double>(vec) : nullptr;
    w.vv = gen ? big.take<double>(vec) : nullptr;
    w.G = big.take<double>((size_t)w.ld * 8 * (size_t)s);
    w.U = big.take<double>((size_t)w.ld * 8 * (size_t)s);
    w.st = sm.take<IdrsState>(sizeof(IdrsState));
    w.sums = sm.take<double>(16 * 8);   // P^T r / P^T g (8), [t.t, t.r], r.r, b.b, ||b - A x||^2
    w.hist = sm.take<double>((size_t)(maxiter + 1) * 8);
}

// what the phases of one solve share
struct IdrsRun : SolveRun {
    IdrsWork w;
    int sdim;
    GridSum gsP, gsT, gsR;
};

static int idrs_workspace(IdrsRun &r) {
    auto layout = [&](Carve &big, Carve &sm) {
        idrs_layout(big, sm, r.n, r.ctl->maxiter, r.sdim, r.gen, r.dinv != nullptr, r.w);
    };
    return workspace_carve(r.A, kWsFloor, true, layout, nullptr);
}

// everything in front of the loop: the gridsums, the state, b, x0 = 0, r = b, G = U = 0 and the init launch (b.b).
// *run: steps may be enqueued (false: the stamp already says b = 0; only the general path waits to learn it)
static int idrs_init(IdrsRun &r, StampPoll &poll, const double *b, int32_t loc, bool *run) {
    IdrsWork &w = r.w;
    hipStream_t s = r.s;
    const int64_t n = r.n;
    GridSum gs0;
    PSK_TRY(gridsum_prepare(r.c, r.nv, r.sdim, w.sums + kIdrsPd, &r.gsP));   // the widest first: it sizes the slots
    PSK_TRY(gridsum_prepare(r.c, r.nv, 2, w.sums + kIdrsTt, &r.gsT));
    PSK_TRY(gridsum_prepare(r.c, r.nv, 1, w.sums + kIdrsRr, &r.gsR));
    PSK_TRY(gridsum_prepare(r.c, r.nv, 1, w.sums + kIdrsBb, &gs0));
    PSK_HIP(hipMemsetAsync(w.st, 0, sizeof(IdrsState), s));
    PSK_TRY(to_device_vec(b, loc, n, w.bv, s));
    PSK_HIP(hipMemsetAsync(w.x, 0, (size_t)n * 8, s));
    PSK_HIP(hipMemsetAsync(w.G, 0, (size_t)w.ld * 8 * (size_t)r.sdim, s));
    PSK_HIP(hipMemsetAsync(w.U, 0, (size_t)w.ld * 8 * (size_t)r.sdim, s));
    PSK_HIP(hipMemcpyAsync(w.r, w.bv, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    PSK_HIP(hipEventRecord(r.kit->ev0, s));
    hipLaunchKernelGGL(idrs_init_kernel, dim3((unsigned)r.nv), dim3(kBlock), 0, s, n, w.bv, gs0,
                       IdrsInitFin{r.ctl->tau, r.ctl->norm_b, w.st, poll.hdone(), poll.hgen()});
    PSK_HIP(hipGetLastError());
    *run = true;
    if (r.gen) {
        // The preconditioner's kernels do not test `done`: they run in every step the host enqueues, also behind
        // the one that ended the solve. So they only ever see defined vectors: v starts at zero, and a b = 0 solve
        // enqueues no step at all.
        PSK_HIP(hipMemsetAsync(w.vv, 0, (size_t)n * 8, s));
        PSK_TRY(poll.wait(s));
        *run = poll.stamp() == 0;
    }
    return PSK_OK;
}

// F / Q for the run's s
template <template <int> class Fin, class... Args>
static void idrs_launch_pdot(const IdrsRun &r, const double *vec, Args... args) {
    const dim3 g((unsigned)r.nv), blk(kBlock);
    switch (r.sdim) {
#define PSK_IDRS_CASE(S)                                                                                              \
    case S:                                                                                                          \
        hipLaunchKernelGGL((idrs_pdot_kernel<S, Fin<S>>), g, blk, 0, r.s, r.n, vec, r.gsP,                            \
                           (const IdrsState *)r.w.st, Fin<S>{r.w.st, args...});                                      \
        break;
        PSK_IDRS_CASE(1)
        PSK_IDRS_CASE(2)
        PSK_IDRS_CASE(3)
        PSK_IDRS_CASE(4)
        PSK_IDRS_CASE(5)
        PSK_IDRS_CASE(6)
        PSK_IDRS_CASE(7)
        PSK_IDRS_CASE(8)
#undef PSK_IDRS_CASE
    }
}

// step j: inner step k = j mod (s + 1) < s: [F], V, S, Q, U; k = s: S, T, W
static int idrs_step(IdrsRun &r, int64_t j) {
    IdrsWork &w = r.w;
    hipStream_t s = r.s;
    const int64_t n = r.n;
    const int sd = r.sdim, k = (int)(j % (sd + 1));
    const dim3 g((unsigned)r.nv), blk(kBlock);
    const int32_t *done = &w.st->done;
    const IdrsState *cst = w.st;
    const double *nul = nullptr;
    const IdrsStepFin fin{w.st, w.hist, j, r.ctl->maxiter, r.ctl->fail_on_maxiter, k, sd};
    if (k < sd) {
        if (k == 0) idrs_launch_pdot<IdrsCycleFin>(r, w.r);
        if (r.gen) {
            hipLaunchKernelGGL(idrs_v_kernel<2>, g, blk, 0, s, n, w.r, nul, w.G, w.U, w.ld, sd, k, nul, w.vv, cst);
            PSK_HIP(hipGetLastError());
            PSK_TRY(prec_apply_dev(r.M, n, w.vv, w.vh, s));
            hipLaunchKernelGGL(idrs_v_kernel<3>, g, blk, 0, s, n, nul, w.vh, w.G, w.U, w.ld, sd, k, nul, w.uw, cst);
        } else if (r.dinv) {
            hipLaunchKernelGGL(idrs_v_kernel<1>, g, blk, 0, s, n, w.r, nul, w.G, w.U, w.ld, sd, k, r.dinv, w.uw, cst);
        } else {
            hipLaunchKernelGGL(idrs_v_kernel<0>, g, blk, 0, s, n, w.r, nul, w.G, w.U, w.ld, sd, k, nul, w.uw, cst);
        }
        PSK_HIP(hipGetLastError());
        PSK_TRY(launch_spmv(r.A, kSpmvPlain, w.uw, w.gw, nullptr, nullptr, nullptr, done, s));
        idrs_launch_pdot<IdrsOrthFin>(r, w.gw, k, j);
        if (r.dinv && k == sd - 1)
            hipLaunchKernelGGL(idrs_gu_kernel<true>, g, blk, 0, s, n, w.gw, w.uw, w.G, w.U, w.ld, k, w.r, w.x, r.dinv, w.vh,
                               r.gsR, w.st, fin);
        else
            hipLaunchKernelGGL(idrs_gu_kernel<false>, g, blk, 0, s, n, w.gw, w.uw, w.G, w.U, w.ld, k, w.r, w.x, nul,
                               (double *)nullptr, r.gsR, w.st, fin);
    } else {
        if (r.gen) PSK_TRY(prec_apply_dev(r.M, n, w.r, w.vh, s));
        const double *v = r.gen || r.dinv ? w.vh : nul;
        PSK_TRY(launch_spmv(r.A, kSpmvPlain, v ? v : w.r, w.gw, nullptr, nullptr, nullptr, done, s));
        hipLaunchKernelGGL(idrs_tt_kernel, g, blk, 0, s, n, w.gw, w.r, r.gsT, cst, IdrsOmegaFin{w.st, j});
        hipLaunchKernelGGL(idrs_w_kernel, g, blk, 0, s, n, v, w.gw, w.r, w.x, r.gsR, w.st, fin);
    }
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// stopped by the tolerance test on a non-zero b: the exit whose true residual ||b - A x|| is measured and reported
static bool idrs_tol_exit(const IdrsState &hs) { return hs.done == 1 && !hs.zero_b && hs.by_tol; }

// behind the loop: the state; on a tolerance exit the true residual into *true_sq; the checks of the in-launch
// reductions and loop_ms
static int idrs_finish(IdrsRun &r, IdrsState *hs, double *true_sq, psk_result *res) {
    IdrsWork &w = r.w;
    hipStream_t s = r.s;
    PSK_HIP(hipMemcpyAsync(hs, w.st, sizeof(*hs), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    *true_sq = 0.0;
    if (idrs_tol_exit(*hs)) {   // gw is free by now
        PSK_TRY(launch_spmv(r.A, kSpmvResid, w.x, w.gw, nullptr, w.bv, w.sums + kIdrsTrue, nullptr, s));
        PSK_HIP(hipMemcpyAsync(true_sq, w.sums + kIdrsTrue, 8, hipMemcpyDeviceToHost, s));
    }
    return solve_finish(r, res);
}

// The state hs of a finished loop that enqueued `launched` steps, decoded into res; the history and x.
static int idrs_report(const IdrsRun &r, const IdrsState &hs, int64_t launched, double true_sq, psk_result *res,
                       double *hist, double *xout, int32_t loc) {
    res->norm_b = hs.normB;
    // SpMV launches that did their work: one per step up to the one that raised `done` (those behind it returned at
    // once), + the true residual's
    res->spmv_launches = (hs.zero_b ? 0 : hs.done ? hs.iters + 1 : launched) + (idrs_tol_exit(hs) ? 1 : 0);
    res->resid_recursive = hs.rec;
    const char *brk = hs.brk_kind == 1   ? "breakdown Mm[k][k]==0"
                      : hs.brk_kind == 2 ? "breakdown dot(t,t)==0"
                                         : "breakdown dot(t,r)==0";
    result_outcome({hs.zero_b, hs.done, hs.by_tol, hs.iters + 1, hs.iters, hs.rec, brk}, r.ctl->maxiter, res);
    if (idrs_tol_exit(hs)) result_true_resid("IDR(s)", std::sqrt(true_sq), hs.tauNormB, r.ctl->tau, hs.rec, true, res);
    return result_copy_out(r, hs.zero_b ? 0 : hs.nhist, r.w.hist, r.w.x, res, hist, xout, loc);
}

// the phases in order; the caller drains the stream when one fails
static int idrs_solve(IdrsRun &r, const double *b, double *xout, psk_result *res, double *hist, int32_t loc) {
    PSK_TRY(idrs_workspace(r));
    PSK_TRY(solve_kit(r.c, false, &r.kit));
    StampPoll poll(r.kit);   // the host-mapped done stamp the kernels write (idrs_set_done)
    bool run;
    PSK_TRY(idrs_init(r, poll, b, loc, &run));
    int64_t launched = 0;
    if (run) PSK_TRY(poll_loop<2>(poll, r, r.ctl->maxiter, &launched, [&](int64_t j) { return idrs_step(r, j); }));
    IdrsState hs;
    double true_sq;
    PSK_TRY(idrs_finish(r, &hs, &true_sq, res));
    return idrs_report(r, hs, launched, true_sq, res, hist, xout, loc);
}

}  // namespace psk

using namespace psk;

extern "C" int psk_idrs(const psk_csr *Ac, const psk_prec *M, const double *b, double *xout, const psk_ctl *ctl,
                        int32_t s, psk_result *res, double *hist, int32_t loc) {
    if (s < 1 || s > PSK_IDRS_MAX_S) return fail(PSK_ERR_ARG, "psk_idrs: s must be 1.." + std::to_string(PSK_IDRS_MAX_S));
    IdrsRun r{};
    r.sdim = s;
    return solve_entry("psk_idrs", "IDR(s)", r, Ac, M, b, xout, ctl, res, 1, kVecTile, [&]() -> int {
        if (r.n == 0) {   // no rows: b = 0
            result_trivial(res);
            return PSK_OK;
        }
        return idrs_solve(r, b, xout, res, hist, loc);
    });
}
