// pcg.hip — device-resident preconditioned CG (PCGSolver.solve, PCGSolver.py:64-142).
//
// Per iteration k three launches, no host synchronisation:
//   K1  Ap = A p  and p.Ap                                         (launch_spmv, kSpmvDot) :111,:113
//   K2  alpha = uDotR/pTAp; r -= alpha Ap; u = M^-1 r; r.r and u.r   :114-125,:134
//   K3  x += alpha p (alpha recomputed from K1's sum); ||r|| test (tau*||b||, or
//       k==maxiter-1 when !failOnMaxiter); beta; p = u + beta p       :121,:125-138
// x is updated in K3 rather than K2 because K3 streams p anyway: that saves one read of p (8n
// bytes per iteration). x depends on nothing else in the iteration, so the order is invisible.
// All three are one-shot launches (one tile per workgroup); K1 and K2 finish their dot products in
// the same launch with a fixed reduction order (gridsum, psk_internal.hpp), so every workgroup
// (and every rank, after the RCCL sum) reads bit-identical scalars and takes identical branches; the
// control state (done flag, iteration count, residual) lives in HBM and the host only polls it
// every `check_every` iterations with a lag, keeping the launch queue full.
// u is never stored: K2 and K3 both recompute u_i = DInv_i * r_i (one rounding, as np.multiply).
// Elementwise updates use two roundings (-ffp-contract=off), exactly as numpy's x + alpha*p.
#include "psk_internal.hpp"
#include "dist.hpp"
#include "pcg_state.hpp"

#include <cstdlib>

#include <climits>
#include <cmath>
#include <cstdio>
#include <type_traits>

namespace psk {

// ---- K0 (Jacobi/identity): p_0 = M b; [b.b, u.r] --------------------------------------------
// One-shot, the two sums finished in the same launch by gridsum and, unsharded, the solver state set by the
// wave that completes them (PcgInitFin; a sharded solve gathers the per-rank sums and runs
// pcg_init_finish_kernel). x0 = 0 is not stored: K3's first flush of the deferred x updates starts from the
// literal 0.0 (x = np.zeros_like(b) :100, then x + alpha*p :121: the same roundings). r = np.copy(b) (:97) is
// not stored either (round 5): K2 of iteration 0 reads b where it would read r, and writes r. 16 B/row.
// Round 5: the sums run over the SpMV's 256-row gridsum tiles with one row per lane (two tiles per
// workgroup) and the SpMV's tile epilogue (per-row products, wave totals in wave order): the diagonal
// layout's init fused into the first SpMV (spmv_diag.hip pcg_init_diag_kernel) then has the same bits.
template <int JAC, bool FUSED>
__global__ __launch_bounds__(kBlock) void pcg_init_kernel(int64_t n, const double *__restrict__ b,
                                                          const double *__restrict__ dinv, double ds,
                                                          double *__restrict__ p, GridSum gs, PcgInitFin fin,
                                                          int64_t ntiles) {
    constexpr int TPW = 2;
    const int tid = threadIdx.x;
    int64_t tl[TPW];
    bool tv[TPW];
    double acc[TPW][2];
    uint32_t ticket[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t t = (int64_t)blockIdx.x * TPW + q;
        tv[q] = t < ntiles;
        tl[q] = tv[q] ? t : ntiles - 1;
        const int64_t row = tl[q] * kBlock + tid;
        const bool has = tv[q] && row < n;
        const double bi = has ? __builtin_nontemporal_load(b + row) : 0.0;
        const double d = JAC == 1 ? (has ? dinv[row] : 0.0) : ds;
        const double u = JAC ? d * bi : bi;                     // p = precond.applyRight(r)  :98
        if (has) p[row] = u;                                    // (r = np.copy(b) :97 is read from b by K2)
        acc[q][0] = has ? bi * bi : 0.0;                        // self.norm(b)  :86
        acc[q][1] = has ? u * bi : 0.0;                         // uDotR = np.dot(u, r)  :102
    }
    __shared__ GridSumTile<2> gsl[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        ticket[q] = 0;
        if (tv[q] && gs.grp_log2 >= 0 && tid == 0)
            ticket[q] = gridsum_draw(gridsum_counter(gs, gridsum_group_of(tl[q], gs.grp_log2)));
    }
    if (tid < TPW) gsl[tid].cnt = 0;
    if (tid == 0 && blockIdx.x == 0 && (gs.nt + TPW - 1) / TPW != gridDim.x) atomicOr(gs.err, 2);
    __syncthreads();
    if (FUSED)
        gridsum_tiles_publish<TPW, 2>(gs, gsl, acc, ticket, tl, tv, fin);
    else
        gridsum_tiles_publish<TPW, 2>(gs, gsl, acc, ticket, tl, tv);
}

// sharded init: the per-rank sums all-gathered, added in rank order (bit-identical on every rank)
__global__ void pcg_init_finish_kernel(const double *g, int P, double tau, PcgState *st, double *udr,
                                       int64_t *hdone, int64_t hgen) {
    if (threadIdx.x == 0) pcg_init_state(rank_sum(g, P, 2, 0), rank_sum(g, P, 2, 1), tau, st, udr, hdone, hgen, 0);
}

// ---- K2: r update + grid sums [r.r, u.r] -------------------------------------------------
// One-shot: workgroup b owns elements [512b, 512b+512), two per lane (16-B accesses). Round 6 measured three other
// forms of its grid sums, none better at both N = 10M and 16384^2 (profiles/r6_k2_wave_ab.txt,
// r6_k2_gridmask_ab.txt): one tile per WAVE with the workgroup's bits (-1 to -2%), one tile per wave with DPP wave
// totals (+1% / -2%), DPP wave totals combined in LDS instead of block_sum (+-0). JAC: Jacobi
// preconditioner fused: 1 = DInv streamed, 2 = every DInv entry the same double `ds` (constant-
// diagonal matrices such as stencils: the same products, 8 B/row less per kernel).
// FIRST (iteration 0): r_0 = b is read from b (the init does not copy it, K0 above).
template <int JAC, bool FIRST>
__global__ __launch_bounds__(kBlock) void pcg_update_kernel(
    int64_t n, double *__restrict__ r, const double *__restrict__ b, const double *__restrict__ Ap,
    const double *__restrict__ dinv, double ds, const double *__restrict__ pap, int nparts, GridSum gs, PcgState *st,
    const double *__restrict__ udr, int64_t k, TileMap tm) {
    // the done flag, p.Ap and udr[k] loaded together (one scalar round trip, not three in a chain): every
    // address is valid whatever the flag says, and the asm keeps the loads above the branch (round 6: +0.5-1.8%
    // PCG it/s at N = 10M, profiles/r6_prologue_ab.txt)
    const double udk = udr[k];
    const int32_t dn = st->done;
    const double pap0 = pap[0];
    __asm__ volatile("" ::"s"(dn), "s"(pap0), "s"(udk));
    if (dn) return;
    double pTAp = pap0;                                      // np.dot(p, Ap)  :113 (K1's grid sum; rank_sum)
    for (int q = 1; q < nparts; ++q) pTAp += pap[q];
    __shared__ double sh[2 * kWaves];
    if (pTAp == 0.0) {                                       // :114-115 handleBreakdown(k, ...)
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->brk_kind = 2;
            st->iters = k;
            set_done(st, 2, k + 2);
        }
        return;
    }
    const double alpha = udk / pTAp;                         // :118
    // K3 (x update) runs iff this K2 did: it tests `live`, written by the previous kernel, never its
    // own done flag, which its first workgroup may set while later ones are still starting
    if (blockIdx.x == 0 && threadIdx.x == 0) st->live = k;
    // tile of this workgroup: XCD-banded like the SpMV's (tm), so the Ap rows a tile reads were
    // written through the same XCD's L2; the grid sums are published by tile (order-independent)
    const int64_t tile = tile_of_block(tm);
    const int64_t i = tile * kVecTile + 2 * threadIdx.x;
    const bool pair = i + 1 < n;
    uint32_t ticket = 0;   // gridsum ticket, drawn by thread 0 once its loads are issued
    double rr = 0.0, ur = 0.0;
    if (pair) {
        // (issued after the done test: issued before it, K2 measured 1-5% slower, profiles/r6_k2_early_sum2_ab.txt)
        const dv2 ro = FIRST ? ld2nt(b + i) : ld2(r + i), a = ld2nt(Ap + i);
        dv2 d{ds, ds};
        if (JAC == 1) d = ld2(dinv + i);
        ticket = gridsum_ticket(gs, tile);
        dv2 rn;
        rn.x = ro.x - alpha * a.x;                           // r = r - alpha*Ap  :122
        rn.y = ro.y - alpha * a.y;
        double u0 = rn.x, u1 = rn.y;
        if (JAC) {
            u0 = d.x * rn.x;                                 // u = precond.applyRight(r)  :123
            u1 = d.y * rn.y;
        }
        st2(r + i, rn);
        rr = fma(rn.x, rn.x, rr);
        rr = fma(rn.y, rn.y, rr);
        ur = fma(u0, rn.x, ur);
        ur = fma(u1, rn.y, ur);
    } else if (i < n) {   // odd tail element
        ticket = gridsum_ticket(gs, tile);
        const double rn = (FIRST ? b[i] : r[i]) - alpha * Ap[i];
        const double u0 = JAC == 2 ? ds * rn : JAC ? dinv[i] * rn : rn;
        r[i] = rn;
        rr = rn * rn;
        ur = u0 * rn;
    }
    block_sum2(rr, ur, sh);   // both sums in one barrier pair (same bits as two block_sums; round 6: +0.3%)
    const double v[2] = {rr, ur};
    // wave 0 alone publishes the tile and, holding its group's last ticket, reduces the group and takes part in the
    // final stage in the wave forms (gridsum_take<2, 64>, gridsum_final_wave): no barrier after the totals (round 6:
    // +0.3-0.7% PCG it/s at N = 10M, profiles/r6_k2_wpub_ab.txt; the group and final sums run in the wave order)
    if (threadIdx.x >= 64) return;
    const bool lane0 = threadIdx.x == 0;
    if (gs.grp_log2 < 0) {
        if (lane0) {
            gridsum_put(gs.gslots + tile * 2, v[0]);
            gridsum_put(gs.gslots + tile * 2 + 1, v[1]);
        }
        gridsum_final_wave<2>(gs);
        return;
    }
    if (lane0) {
        gridsum_put(gs.slots + gridsum_slot(gs, tile) * 2, v[0]);
        gridsum_put(gs.slots + gridsum_slot(gs, tile) * 2 + 1, v[1]);
    }
    const uint32_t tk = __builtin_amdgcn_readfirstlane(ticket);
    const int64_t g = gridsum_group_of(tile, gs.grp_log2);
    int64_t base;
    const int64_t cnt = gridsum_members(gs, g, base);
    if (tk != (uint32_t)(cnt - 1)) return;
    double gr[2];
    gridsum_take<2, 64>(gs.slots, g << gs.grp_log2, cnt, gs.err, nullptr, gr);
    if (lane0) {
        gridsum_reset(gridsum_counter(gs, g));
        gridsum_put(gs.gslots + g * 2, gr[0]);
        gridsum_put(gs.gslots + g * 2 + 1, gr[1]);
    }
    gridsum_final_wave<2>(gs);
}

// ---- K3: x += alpha p (deferred, above), convergence test, beta, p = u + beta p (one-shot, as K2) --
// A breakdown leaves the updates of the iterations since the last flush pending (pcg_flush_kernel).
// STAG (pcg_state.hpp, the staggered flush): the in-loop SpMV launches flush x block by block, so K3 touches x
// only on the iteration that ends the solve, where it catches up every row with its own block's pending range.
template <int JAC, bool STAG>
__global__ __launch_bounds__(kBlock) void pcg_direction_kernel(
    int64_t n, double *__restrict__ x, const double *__restrict__ r, PRing pr, const double *__restrict__ dinv,
    double ds, const double *__restrict__ pap, const double *__restrict__ rrur, int nparts, PcgState *st,
    double *__restrict__ udr, double *__restrict__ hist, double *__restrict__ alphas, int64_t k, int64_t maxiter,
    int fail_on_maxiter, int64_t tile_base, TileMap tm) {
    // every solver scalar loaded together with the live flag (one scalar round trip; see K2)
    const double udk = udr[k];
    const int64_t live = st->live;
    const double tauNB = st->tauNormB, pap0 = pap[0], rr0 = rrur[0], ur0 = rrur[1];
    __asm__ volatile("" ::"s"(live), "s"(pap0), "s"(rr0), "s"(ur0), "s"(udk), "s"(tauNB));
    if (live != k) return;   // K2 returned (stopped earlier, or breakdown at :114)
    double pTAp = pap0, rr = rr0, ur = ur0;   // rank_sum's order
    for (int q = 1; q < nparts; ++q) {
        pTAp += pap[q];
        rr += rrur[2 * q];
        ur += rrur[2 * q + 1];
    }
    // tile_base: a sharded solve launches the tiles holding the rows its neighbours need first (the
    // halo exchange then overlaps the rest); tile 0 alone writes the solver state. tm: XCD bands
    // over the launch's tiles (see K2)
    const int64_t tile = tile_base + tile_of_block(tm);
    const double *pcur = pr.b[k % kPcgDefer];
    // NOT __restrict__: on a uniform flush pnext is p_{k+1-kPcgDefer}'s buffer, which the x catch-up below reads
    // through pr.b first; the store to pnext must stay after those loads. Staggered, pnext (still
    // p_{k+1-kPcgDefer}, ring slot (k + 1) % kPcgDefer) is older than every pending iteration: a block's range
    // starts at k - (kPcgStagger - 1) or later (pcg_flush_pending) and kPcgStagger < kPcgDefer, so no catch-up
    // reads it; the order of the loads and the store is kept all the same
    double *pnext = pr.b[(k + 1) % kPcgDefer];
    constexpr int S = kPcgStagger > 0 ? kPcgStagger : 1;
    const PcgPend pd = STAG ? pcg_flush_pending(S, pcg_block_of_tile(tile, (n + kVecTile - 1) / kVecTile, S), k, false)
                            : pcg_uniform_pending(k);
    const int q = (int)(k - pd.first);   // < kPcgDefer
    double alpha, beta;
    if (!pcg_direction_scalars(n, x, pcur, pTAp, rr, ur, udk, tauNB, st, udr, hist, k, maxiter, fail_on_maxiter,
                               alpha, beta, tile, &pr, alphas, pd))
        return;
    const bool flush = (!STAG && q == kPcgDefer - 1) || k == maxiter - 1;
    const bool x0 = pd.first == 0;   // the rows were never stored: x is the implicit x0 = 0 (never loaded)
    if (tile == 0 && threadIdx.x == 0) {
        alphas[k] = alpha;
        if (flush) st->x_written = 1;
    }
    const int64_t i = tile * kVecTile + 2 * threadIdx.x;
    // r, dinv and x are not needed again this iteration (non-temporal); p is gathered by the next SpMV
    if (i + 1 < n) {
        const dv2 ro = ld2nt(r + i), po = ld2(pcur + i);
        dv2 d{ds, ds};
        if (JAC == 1) d = ld2nt(dinv + i);
        double u0 = ro.x, u1 = ro.y;
        if (JAC) {
            u0 = d.x * ro.x;
            u1 = d.y * ro.y;
        }
        if (flush) {
            dv2 xo{0.0, 0.0};
            if (!x0) xo = ld2nt(x + i);
            dv2 pp[kPcgDefer > 1 ? kPcgDefer - 1 : 1];
#pragma unroll
            for (int t = 1; t < kPcgDefer; ++t)
                if (t <= q) pp[t - 1] = ld2nt(pr.b[(k - t) % kPcgDefer] + i);
#pragma unroll
            for (int t = kPcgDefer - 1; t >= 1; --t)
                if (t <= q) {
                    const double a = alphas[k - t];
                    xo.x = xo.x + a * pp[t - 1].x;           // x = x + alpha*p  :121 (iteration k-t)
                    xo.y = xo.y + a * pp[t - 1].y;
                }
            dv2 xn;
            xn.x = xo.x + alpha * po.x;                      // :121
            xn.y = xo.y + alpha * po.y;
            st2nt(x + i, xn);
        }
        dv2 pn;
        pn.x = u0 + beta * po.x;                             // p = u + beta*p  :138
        pn.y = u1 + beta * po.y;
        st2(pnext + i, pn);   // (non-temporal and write-through p stores measured no faster, round 4)
    } else if (i < n) {
        const double u0 = JAC == 2 ? ds * r[i] : JAC ? dinv[i] * r[i] : r[i];
        const double pi = pcur[i];
        if (flush) x[i] = pcg_catch_up(x0 ? 0.0 : x[i], &pr, pd.first, k, alphas, i) + alpha * pi;
        pnext[i] = u0 + beta * pi;
    }
}

// the x updates a breakdown at iteration k left pending: the iterations pcg_flush_pending (STAG: of the row's
// block) or pcg_uniform_pending names; rows with nothing pending keep the x they hold
template <bool STAG>
__global__ void pcg_flush_kernel(int64_t n, double *__restrict__ x, PRing pr, const double *__restrict__ alphas,
                                 int64_t k) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    constexpr int S = kPcgStagger > 0 ? kPcgStagger : 1;
    const PcgPend pd = STAG ? pcg_flush_pending(S, pcg_block_of_tile(i / kVecTile, (n + kVecTile - 1) / kVecTile, S), k,
                                                false)
                            : pcg_uniform_pending(k);
    if (i < n && pd.first <= pd.last) x[i] = pcg_catch_up(pd.first == 0 ? 0.0 : x[i], &pr, pd.first, k, alphas, i);
}

// pcg_flush_kernel on the solver's stream (psk_pcg after a breakdown; the lab library's test entry point)
int launch_pcg_flush(int64_t n, double *x, const PRing &pr, const double *alphas, int64_t k, bool stag, hipStream_t s) {
    if (n <= 0) return PSK_OK;
    const dim3 g((unsigned)((n + kBlock - 1) / kBlock));
    if (stag && kPcgStagger > 0) hipLaunchKernelGGL(pcg_flush_kernel<true>, g, dim3(kBlock), 0, s, n, x, pr, alphas, k);
    else hipLaunchKernelGGL(pcg_flush_kernel<false>, g, dim3(kBlock), 0, s, n, x, pr, alphas, k);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// ---- end of a solve: the state, the scan of the gridsum ticket counters (gridsum_counter_check_kernel's)
// and the gridsum error word into the host-mapped words at kit->hmap + kPcgFinishWord (system scope)
constexpr int kPcgStateWords = (int)(sizeof(PcgState) / 8);
constexpr int kPcgFinishWord = 8;
static_assert(sizeof(PcgState) % 8 == 0 && kPcgFinishWord + kPcgStateWords + 1 <= 64, "SolveKit::hmap words");
__global__ __launch_bounds__(kBlock) void pcg_finish_kernel(const PcgState *st, const uint32_t *cnt, const int32_t *err,
                                                            int64_t *hw) {
    // every counter (kGridSumMaxGroups + 1) loaded at once, unconditionally (indices clamped): one memory
    // round trip instead of a dependent chain of nine
    constexpr int kPer = (kGridSumMaxGroups + kBlock) / kBlock;
    uint32_t v[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int g = (int)threadIdx.x + i * kBlock;
        v[i] = cnt[(int64_t)(g < kGridSumMaxGroups ? g : kGridSumMaxGroups) * kGridSumCntStride];
    }
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) any |= v[i];
    const bool bad = __syncthreads_or(any != 0);
    if (threadIdx.x < kPcgStateWords)
        __hip_atomic_store(hw + threadIdx.x, reinterpret_cast<const int64_t *>(st)[threadIdx.x], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    if (threadIdx.x == 0)
        __hip_atomic_store(hw + kPcgStateWords, (int64_t)(*err | (bad ? 4 : 0)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- general preconditioner (ILU, ...): u = M^-1 r is materialised by the preconditioner's own
// kernels between K2 and K3, so u.r gets its own reduction and K3 reads u ----------------------
__global__ __launch_bounds__(kBlock) void pcg_gen_init_kernel(int64_t n, const double *__restrict__ b,
                                                              double *__restrict__ x, double *__restrict__ r) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        r[i] = b[i];   // r = np.copy(b)        :97
        x[i] = 0.0;    // x = np.zeros_like(b)  :100
    }
}

// p = u (copy of M^-1 r, :98-99); [b.b, u.r] finished in-launch and the state set (one-shot, as K0)
__global__ __launch_bounds__(kBlock) void pcg_gen_init2_kernel(int64_t n, const double *__restrict__ r,
                                                               const double *__restrict__ u, double *__restrict__ p,
                                                               GridSum gs, PcgInitFin fin) {
    __shared__ double sh[kWaves];
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    const uint32_t ticket = gridsum_ticket(gs);
    double bb = 0.0, ur = 0.0;
    for (int64_t j = i; j < i + 2 && j < n; ++j) {
        const double rj = r[j], uj = u[j];
        p[j] = uj;
        bb = fma(rj, rj, bb);
        ur = fma(uj, rj, ur);
    }
    const double v[2] = {block_sum(bb, sh), block_sum(ur, sh)};
    gridsum_publish<2>(gs, v, sh, ticket, fin);
}

__global__ __launch_bounds__(kBlock) void pcg_dot_kernel(int64_t n, const double *__restrict__ a,
                                                         const double *__restrict__ c, GridSum gs,
                                                         const PcgState *st) {
    if (st->done) return;
    __shared__ double sh[kWaves];
    const int64_t i = (int64_t)blockIdx.x * kVecTile + threadIdx.x;
    const uint32_t ticket = gridsum_ticket(gs);
    double acc = 0.0;
    if (i < n) acc = a[i] * c[i];                                               // np.dot(u, r) :134
    if (i + kBlock < n) acc = fma(a[i + kBlock], c[i + kBlock], acc);
    const double v = block_sum(acc, sh);
    gridsum_publish<1>(gs, &v, sh, ticket);
}

__global__ __launch_bounds__(kBlock) void pcg_gen_direction_kernel(
    int64_t n, double *__restrict__ x, const double *__restrict__ u, double *__restrict__ p,
    const double *__restrict__ pap, const double *__restrict__ rrur, const double *__restrict__ ur_gen, PcgState *st,
    double *__restrict__ udr, double *__restrict__ hist, int64_t k, int64_t maxiter, int fail_on_maxiter) {
    if (st->live != k) return;
    double alpha, beta;
    if (!pcg_direction_scalars(n, x, p, *pap, rrur[0], *ur_gen, udr[k], st->tauNormB, st, udr, hist, k, maxiter,
                               fail_on_maxiter, alpha, beta, blockIdx.x))
        return;
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    for (int64_t j = i; j < i + 2 && j < n; ++j) {
        const double pj = p[j];
        x[j] = x[j] + alpha * pj;                            // :121
        p[j] = u[j] + beta * pj;                             // :138
    }
}

// -------------------------------------------------------------------------------------------------
// host driver: psk_pcg = plan, init, the loop (one iteration a function of k), finish, report

struct PcgWork {
    double *x, *r, *p, *Ap, *u, *part1, *part2, *part3, *udr, *hist;
    PRing pr;              // Jacobi/identity K3: p_j in pr.b[j % kPcgDefer] (pr.b[0] = p)
    double *alphas;        // alpha_k (deferred x updates)
    double *pinit;         // the init's two grid sums [b.b, u.r] (this rank's, sharded)
    // sharded (P ranks): the ranks' gathered scalars, [P] p.Ap, [P][2] (r.r, u.r) and [P][2] init sums;
    // unsharded: part1g/part2g alias part1/part2
    double *part1g, *part2g, *initg;
    PcgState *st;
};

// the layout of A->ws (big) and A->ws_small (sm): run on null-based carvers for the sizes, then on the buffers
static void pcg_layout(Carve &big, Carve &sm, int64_t n, int64_t ncols, int64_t maxiter, bool gen, bool own_x, int P,
                       PcgWork &w) {
    const size_t vec = (size_t)n * 8, vecc = (size_t)ncols * 8, it = (size_t)(maxiter + 1) * 8;
    w.r = big.take<double>(vec);
    w.Ap = big.take<double>(vec);
    // x lives in the caller's device vector when the solve writes there directly (own_x false)
    w.x = own_x ? big.take<double>(vec) : nullptr;
    for (int t = 0; t < kPcgDefer; ++t) w.pr.b[t] = gen && t > 0 ? nullptr : big.take<double>(vecc);
    w.p = w.pr.b[0];
    w.u = gen ? big.take<double>(vec) : nullptr;
    w.st = sm.take<PcgState>(sizeof(PcgState));
    w.part1 = sm.take<double>(kMaxGrid * 8);
    w.part3 = sm.take<double>(kMaxGrid * 8);
    w.part2 = sm.take<double>(2 * kMaxGrid * 8);
    w.udr = sm.take<double>(it + 8);
    w.hist = sm.take<double>(it);
    w.alphas = sm.take<double>(it);
    w.pinit = sm.take<double>(256);
    w.part1g = P > 1 ? sm.take<double>((size_t)P * 8) : w.part1;
    w.part2g = P > 1 ? sm.take<double>((size_t)P * 16) : w.part2;
    w.initg = P > 1 ? sm.take<double>((size_t)P * 16) : w.pinit;
}

void pcg_layout_probe(int64_t n, int64_t ncols, int64_t maxiter, bool gen, bool own_x, int P, std::vector<int64_t> *log,
                      int64_t *bytes) {
    Carve big, sm;
    big.log = sm.log = log;
    PcgWork w;
    pcg_layout(big, sm, n, ncols, maxiter, gen, own_x, P, w);
    bytes[0] = big.off > 0 ? (int64_t)big.off : 256;
    bytes[1] = (int64_t)sm.off;
}

static int pcg_workspace(psk_csr *A, int64_t maxiter, bool gen, bool own_x, int P, PcgWork &w) {
    int64_t need[2];
    pcg_layout_probe(A->n, A->ncols, maxiter, gen, own_x, P, nullptr, need);
    PSK_TRY(A->ws.ensure((size_t)need[0]));
    PSK_TRY(A->ws_small.ensure((size_t)need[1]));
    Carve big{A->ws.as<char>()}, sm{A->ws_small.as<char>()};
    pcg_layout(big, sm, A->n, A->ncols, maxiter, gen, own_x, P, w);
    return PSK_OK;
}

// the regions psk_pcg(maxiter, gen, own_x) carved on this unsharded matrix. grow: size the two buffers first (a
// later solve then keeps them); otherwise PSK_ERR_ARG when either is smaller than the layout. Host code only
// (psk_lab_pcg_internals, psk_lab_pcg_prefill).
int pcg_work_view(psk_csr *A, int64_t maxiter, bool gen, bool own_x, bool grow, PcgView *v) {
    if (!A || !v || maxiter < 0 || A->n < 0) return fail(PSK_ERR_ARG, "pcg_work_view: bad arguments");
    if (A->comm) return fail(PSK_ERR_ARG, "pcg_work_view: sharded matrix");
    int64_t need[2];
    pcg_layout_probe(A->n, A->ncols, maxiter, gen, own_x, 1, nullptr, need);
    if (grow) {
        PSK_TRY(A->ws.ensure((size_t)need[0]));
        PSK_TRY(A->ws_small.ensure((size_t)need[1]));
    }
    if (!A->ws.p || !A->ws_small.p || A->ws.bytes < (size_t)need[0] || A->ws_small.bytes < (size_t)need[1])
        return fail(PSK_ERR_ARG, "pcg_work_view: the matrix's workspace is smaller than this layout");
    Carve big{A->ws.as<char>()}, sm{A->ws_small.as<char>()};
    PcgWork w;
    pcg_layout(big, sm, A->n, A->ncols, maxiter, gen, own_x, 1, w);
    v->n = A->n;
    v->ncols = A->ncols;
    v->r = w.r;
    v->Ap = w.Ap;
    v->x = w.x;
    v->u = w.u;
    for (int t = 0; t < kPcgDefer; ++t) v->ring[t] = w.pr.b[t];
    v->part1 = w.part1;
    v->part2 = w.part2;
    v->part3 = w.part3;
    v->udr = w.udr;
    v->hist = w.hist;
    v->alphas = w.alphas;
    v->st = w.st;
    v->big = A->ws.p;
    v->big_bytes = (size_t)need[0];
    v->small = A->ws_small.p;
    v->small_bytes = (size_t)need[1];
    return PSK_OK;
}

// psk_pcg's choice of the staggered x flush for a solve of A with preconditioner M (the lab library asks too)
bool pcg_staggers(const psk_csr *A, const psk_prec *M) {
    return kPcgStagger > 0 && !prec_is_general(M) && !A->comm && A->n > 0 && spmv_flush_eligible(A);
}

// every path of a solve, decided once (pcg_plan); the phases read it
struct PcgPlan {
    int64_t n, maxiter;
    bool gen;             // general preconditioner (ILU): u = M^-1 r materialised between K2 and K3
    bool sharded;         // P ranks, scalars gathered (not all-reduced) and summed in rank order on every rank
    bool dev_io;          // b and x in HBM: read b in place, write x in place
    int P, jac;           // jac: 0 none, 1 DInv streamed, 2 one DInv value ds
    const double *dinv;
    double ds;
    // one-shot grid of K0/K2/K3 (one 512-element tile per workgroup); K0/K1/K2 finish their dot products
    // in-launch (gridsum), so the loop's scalars are part1[0] = p.Ap and part2[0..1] = (r.r, u.r)
    int64_t nv, nsl;      // nsl: the SpMV's 256-row gridsum tiles
    // the init: unsharded with the diagonal layout (5 diagonals, one DInv value or none) fused into the first
    // SpMV (spmv_diag.hip pcg_init_diag_kernel, [p.Ap, b.b, u.r] into part1); otherwise pcg_init_kernel over the
    // SpMV's 256-row tiles (the same bits for b.b and u.r), or the general path's init over 512-element tiles
    bool init_diag;
    // the staggered x flush (pcg_state.hpp): unsharded Jacobi/identity solves whose in-loop SpMV is the pair-row
    // diagonal kernel; every other path keeps the uniform flush in K3
    bool stag;
    // halo overlap (sharded, Jacobi/identity): when every row a neighbour needs lies in the first ov_lo
    // or the last nv - ov_hi K3 tiles (row-block shards of a banded matrix: one grid line each side),
    // those tiles run first and the exchange of p overlaps the remaining tiles of K3
    bool overlap;
    int64_t ov_lo, ov_hi;
    int C;                // iterations per poll chunk
    // sharded with a mailbox (psk_comm_mailbox): the ranks' scalars go kernel -> mailbox -> gather kernel
    // instead of ncclAllGather; same gathered arrays, same rank-order sums
    psk_comm *mbc;
};

static int pcg_plan(const psk_csr *A, const psk_prec *M, const psk_ctl *ctl, int32_t loc, PcgPlan &pl) {
    pl.n = A->n;
    pl.maxiter = ctl->maxiter;
    pl.gen = prec_is_general(M);
    if (pl.gen && A->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_pcg: ILU preconditioning of a sharded matrix");
    pl.sharded = A->comm != nullptr;
    pl.P = pl.sharded ? A->comm->nranks : 1;
    pl.dev_io = loc == PSK_DEVICE;
    pl.dinv = (M && M->kind == PSK_PREC_JACOBI) ? M->dinv : nullptr;
    pl.jac = !pl.dinv ? 0 : M->dinv_uniform ? 2 : 1;
    pl.ds = pl.jac == 2 ? M->dinv_value : 0.0;
    pl.nv = pl.n > 0 ? (pl.n + kVecTile - 1) / kVecTile : 1;
    if (pl.nv > INT32_MAX) return fail(PSK_ERR_UNSUPPORTED, "psk_pcg: vector too long for a one-shot grid");
    pl.nsl = pl.n > 0 ? (pl.n + kBlock - 1) / kBlock : 1;
    pl.init_diag = !pl.gen && !pl.sharded && (pl.jac == 0 || pl.jac == 2) && pcg_init_diag_eligible(A);
    pl.stag = pcg_staggers(A, M);
    pl.C = ctl->check_every > 0 ? ctl->check_every : (pl.n >= (1 << 20) ? 2 : 16);
    // On by default (PSK_HALO_OVERLAP=0 turns it off); DESIGN.md §6 states the rule: the overlap moves
    // no arithmetic (sharded histories are bit-identical either way) and takes the halo's latency off
    // the critical path whenever K3's interior tiles outlast the exchange, which they do at every
    // size the 8-GPU run uses (>= 1.25M rows per rank); an 8-GPU A/B of the driver's run decides it.
    static const bool overlap_on = [] {
        const char *e = std::getenv("PSK_HALO_OVERLAP");
        return !(e && std::atoi(e) == 0);
    }();
    pl.ov_lo = 0;
    pl.ov_hi = pl.nv;
    pl.overlap = overlap_on && pl.sharded && !pl.gen && halo_split(A, kVecTile, pl.nv, pl.ov_lo, pl.ov_hi);
    pl.mbc = pl.sharded && A->comm->mb ? A->comm : nullptr;
    return PSK_OK;
}

// what the phases of one solve share
struct PcgRun {
    psk_csr *A;
    const psk_prec *M;
    const psk_ctl *ctl;
    Context *c;
    SolveKit *kit;
    hipStream_t s, cs;            // cs: the halo exchanges of the overlap
    PcgPlan pl;
    PcgWork w;
    GridSum gs2, gs3;
    const double *bd;             // b on the device
    bool halo_pending = false;    // an exchange on cs the next SpMV (or the end of the solve) waits for
};

// f(integral_constant<int, jac>, bool_constant<flag>): the <JAC, bool> forms of K0, K2 and K3
template <class F> static void pcg_dispatch(int jac, bool flag, F &&f) {
    auto on = [&](auto J) {
        if (flag) f(J, std::true_type{});
        else f(J, std::false_type{});
    };
    if (jac == 2) on(std::integral_constant<int, 2>{});
    else if (jac == 1) on(std::integral_constant<int, 1>{});
    else on(std::integral_constant<int, 0>{});
}

// Optional timing (ctl.time_kernels = S > 0): every S-th SpMV between two events of a ring of kTimedSlots
// (sampled: an event pair costs ~5% of an iteration at N = 10M); sharded, the same iterations time this rank's
// p.Ap gather and the halo exchange of the iteration (ABI 4: psk_result.gather_ms / halo_ms)
struct PcgTimers {
    SolveKit *kit;
    int S;
    bool skip0;   // init_diag: iteration 0's SpMV ran inside the init launch, not sampled
    int64_t tk[kTimedSlots];                        // the iteration a slot holds (-1: free)
    bool tgat[kTimedSlots], thalo[kTimedSlots];     // sharded: the slot's gather / halo events were recorded
    std::vector<float> spmv_ms;                     // by iteration; -1: not sampled
    double gat_sum = 0.0, halo_sum = 0.0;
    int64_t gat_n = 0, halo_n = 0;
    PcgTimers(SolveKit *k, int stride, bool init_diag, int64_t maxiter) : kit(k), S(stride > 0 ? stride : 0), skip0(init_diag) {
        for (int i = 0; i < kTimedSlots; ++i) {
            tk[i] = -1;
            tgat[i] = thalo[i] = false;
        }
        if (S) spmv_ms.assign((size_t)maxiter, -1.0f);
    }
    int sample(hipEvent_t a, hipEvent_t b, float *ms) {
        PSK_HIP(hipEventSynchronize(b));
        PSK_HIP(hipEventElapsedTime(ms, a, b));
        return PSK_OK;
    }
    int harvest(int slot) {
        if (tk[slot] < 0) return PSK_OK;
        float ms = 0.f;
        PSK_TRY(sample(kit->ta[slot], kit->tb[slot], &ms));
        spmv_ms[(size_t)tk[slot]] = ms;
        tk[slot] = -1;
        if (tgat[slot]) {
            PSK_TRY(sample(kit->ga[slot], kit->gb[slot], &ms));
            gat_sum += ms;
            ++gat_n;
            tgat[slot] = false;
        }
        if (thalo[slot]) {
            PSK_TRY(sample(kit->ha[slot], kit->hb[slot], &ms));
            halo_sum += ms;
            ++halo_n;
            thalo[slot] = false;
        }
        return PSK_OK;
    }
    // iteration k: whether it is timed and its slot, harvested first when the ring has wrapped
    int begin(int64_t k, int *slot, bool *timed) {
        *timed = S > 0 && k % S == 0 && !(skip0 && k == 0);
        *slot = (int)((k / (S > 0 ? S : 1)) % kTimedSlots);
        if (*timed) {
            PSK_TRY(harvest(*slot));
            tk[*slot] = k;
        }
        return PSK_OK;
    }
    // the means over the harvested slots; nk: iterations whose SpMV ran
    void finish(int64_t nk, psk_result *res) const {
        if (!S) return;
        double tot = 0.0;
        const int64_t cnt = nk < (int64_t)spmv_ms.size() ? nk : (int64_t)spmv_ms.size();
        int64_t nt = 0;
        for (int64_t i = 0; i < cnt; i += S)
            if (spmv_ms[(size_t)i] >= 0.0f) {
                tot += spmv_ms[(size_t)i];
                ++nt;
            }
        res->spmv_launches = nt;
        res->spmv_ms = nt > 0 ? tot / (double)nt : 0.0;
        res->gather_ms = gat_n > 0 ? gat_sum / (double)gat_n : 0.0;
        res->halo_ms = halo_n > 0 ? halo_sum / (double)halo_n : 0.0;
        res->comm_samples = gat_n;
    }
};

// the init: the general form, the one fused into the first SpMV (diagonal layout) or pcg_init_kernel; sharded, the
// ranks' sums gathered and the state set by pcg_init_finish_kernel
static int pcg_init(PcgRun &r, const StampPoll &poll, const double *b, int32_t loc) {
    const PcgPlan &pl = r.pl;
    PcgWork &w = r.w;
    const int64_t n = pl.n;
    hipStream_t s = r.s;
    GridSum gs0;
    if (!pl.init_diag) PSK_TRY(gridsum_prepare(r.c, pl.gen ? pl.nv : pl.nsl, 2, w.pinit, &gs0));
    PSK_TRY(gridsum_prepare(r.c, pl.nv, 2, w.part2, &r.gs2));
    PSK_TRY(gridsum_prepare(r.c, pl.nv, 1, w.part3, &r.gs3));
    const PcgInitFin fin{r.ctl->tau, w.st, w.udr, poll.hdone(), poll.hgen(), pl.gen ? 1 : 0, 0};
    r.bd = b;
    if (!pl.dev_io) {   // host b staged in r (r_0 = b already: K2 of iteration 0 then reads r as usual), or, on
                        // the general path, in Ap (unused until the first SpMV; its init copies r = b)
        PSK_TRY(to_device_vec(b, loc, n, pl.gen ? w.Ap : w.r, s));
        r.bd = pl.gen ? w.Ap : w.r;
    }
    const uint64_t seq0 = pl.mbc ? mbox_next(pl.mbc, &gs0) : 0;
    PSK_HIP(hipEventRecord(r.kit->ev0, s));
    if (pl.gen) {
        const unsigned nb = (unsigned)((n + kBlock - 1) / kBlock);
        if (n > 0) hipLaunchKernelGGL(pcg_gen_init_kernel, dim3(nb), dim3(kBlock), 0, s, n, r.bd, w.x, w.r);
        PSK_TRY(prec_apply_dev(r.M, n, w.r, w.u, s));                   // p = precond.applyRight(r)  :98
        hipLaunchKernelGGL(pcg_gen_init2_kernel, dim3((unsigned)pl.nv), dim3(kBlock), 0, s, n, w.r, w.u, w.p, gs0, fin);
    } else if (pl.init_diag) {
        PcgInitFin fin3 = fin;
        fin3.off = 1;
        PSK_TRY(launch_pcg_init_diag(r.A, r.bd, pl.jac == 2 ? pl.ds : 1.0, w.p, w.Ap, w.part1, fin3, s));
    } else {
        const dim3 gi((unsigned)((pl.nsl + 1) / 2));
        pcg_dispatch(pl.jac, !pl.sharded, [&](auto J, auto FUSED) {
            hipLaunchKernelGGL((pcg_init_kernel<decltype(J)::value, decltype(FUSED)::value>), gi, dim3(kBlock), 0, s, n,
                               r.bd, pl.dinv, pl.ds, w.p, gs0, fin, pl.nsl);
        });
    }
    PSK_HIP(hipGetLastError());
    if (pl.sharded) {
        if (pl.mbc) PSK_TRY(mbox_gather(pl.mbc, seq0, 2, w.initg, nullptr, s));
        else PSK_TRY(allgather(r.A, w.pinit, w.initg, 2, s));
        hipLaunchKernelGGL(pcg_init_finish_kernel, dim3(1), dim3(64), 0, s, w.initg, pl.P, r.ctl->tau, w.st, w.udr,
                           poll.hdone(), poll.hgen());
        PSK_HIP(hipGetLastError());
    }
    return PSK_OK;
}

// K3 of iteration k over tiles [t0, t1)
static void pcg_k3(PcgRun &r, int64_t k, int64_t t0, int64_t t1) {
    if (t1 <= t0) return;
    const PcgPlan &pl = r.pl;
    PcgWork &w = r.w;
    const dim3 g3((unsigned)(t1 - t0));
    const TileMap tm3 = tile_map_for(t1 - t0, false);
    pcg_dispatch(pl.jac, pl.stag, [&](auto J, auto SG) {
        hipLaunchKernelGGL((pcg_direction_kernel<decltype(J)::value, decltype(SG)::value && (kPcgStagger > 0)>), g3,
                           dim3(kBlock), 0, r.s, pl.n, w.x, w.r, w.pr, pl.dinv, pl.ds, w.part1g, w.part2g, pl.P, w.st, w.udr,
                           w.hist, w.alphas, k, pl.maxiter, r.ctl->fail_on_maxiter, t0, tm3);
    });
}

// iteration k: the halo of p_k, K1 (with the flush role), K2, the preconditioner or nothing, K3
static int pcg_iteration(PcgRun &r, PcgTimers &tm, int64_t k) {
    const PcgPlan &pl = r.pl;
    PcgWork &w = r.w;
    psk_csr *A = r.A;
    SolveKit *kit = r.kit;
    hipStream_t s = r.s;
    const int64_t n = pl.n;
    // p_k and the buffer K3 writes p_{k+1} into (Jacobi/identity: a ring of kPcgDefer; general: in place)
    double *pk = pl.gen ? w.p : w.pr.b[k % kPcgDefer];
    double *pn = pl.gen ? w.p : w.pr.b[(k + 1) % kPcgDefer];
    int slot;
    bool timed;
    PSK_TRY(tm.begin(k, &slot, &timed));
    if (r.halo_pending) {   // exchanged during the previous K3
        PSK_HIP(hipStreamWaitEvent(s, kit->ev_b, 0));
        r.halo_pending = false;
    } else if (A->comm) {
        const bool th = timed && !A->comm->dry && !A->peers.empty();
        if (th) PSK_HIP(hipEventRecord(kit->ha[slot], s));
        PSK_TRY(halo_exchange(A, pk, s));
        if (th) {
            PSK_HIP(hipEventRecord(kit->hb[slot], s));
            tm.thalo[slot] = true;
        }
    }
    // a timed launch records its events in its own dispatch (kernel start / end)
    uint64_t seq1 = 0;
    // staggered: launch k >= 1 also brings block k mod kPcgStagger of x up to date (launch_spmv sizes the role)
    const SpmvFlush fl{w.x, w.alphas, w.pr, k, pl.nv, 0, 0, 0, 0};
    if (!(pl.init_diag && k == 0))
        PSK_TRY(launch_spmv(A, kSpmvDot, pk, w.Ap, nullptr, nullptr, w.part1, &w.st->done, s, timed ? kit->ta[slot] : nullptr,
                            timed ? kit->tb[slot] : nullptr, 0, pl.mbc ? &seq1 : nullptr, pl.stag && k >= 1 ? &fl : nullptr));
    // K2/K3 tiles in block order: XCD bands matching the SpMV's, and bands walked in alternating
    // directions (a serpentine over SpMV, K2, K3 meant to re-read Ap, r and p from the Infinity Cache),
    // measured no faster (round 4, profiles/r4_spmv_ab.txt: band1 / band2)
    const TileMap tm2 = tile_map_for(pl.nv, false);
    if (pl.sharded) {
        hipEvent_t g0 = timed ? kit->ga[slot] : nullptr, g1 = timed ? kit->gb[slot] : nullptr;
        if (pl.mbc) {
            PSK_TRY(mbox_gather(pl.mbc, seq1, 1, w.part1g, &w.st->done, s, g0, g1));
        } else {
            if (g0) PSK_HIP(hipEventRecord(g0, s));
            PSK_TRY(allgather(A, w.part1, w.part1g, 1, s));
            if (g1) PSK_HIP(hipEventRecord(g1, s));
        }
        if (timed) tm.tgat[slot] = true;
    }
    GridSum gs2k = r.gs2;   // this iteration's mailbox slot (sharded with a mailbox)
    const uint64_t seq2 = pl.mbc ? mbox_next(pl.mbc, &gs2k) : 0;
    // the general path copied r = b in its init (pcg_gen_init_kernel): it never takes the FIRST form
    const dim3 gk((unsigned)pl.nv);
    pcg_dispatch(pl.jac, k == 0 && !pl.gen && pl.dev_io, [&](auto J, auto FIRST) {
        hipLaunchKernelGGL((pcg_update_kernel<decltype(J)::value, decltype(FIRST)::value>), gk, dim3(kBlock), 0, s, n, w.r,
                           r.bd, w.Ap, pl.dinv, pl.ds, w.part1g, pl.P, gs2k, w.st, w.udr, k, tm2);
    });
    if (pl.sharded) {
        if (pl.mbc) PSK_TRY(mbox_gather(pl.mbc, seq2, 2, w.part2g, &w.st->done, s));
        else PSK_TRY(allgather(A, w.part2, w.part2g, 2, s));
    }
    if (pl.gen) {
        PSK_TRY(prec_apply_dev(r.M, n, w.r, w.u, s));          // u = M^-1 r  :123
        hipLaunchKernelGGL(pcg_dot_kernel, gk, dim3(kBlock), 0, s, n, w.u, w.r, r.gs3, w.st);
        hipLaunchKernelGGL(pcg_gen_direction_kernel, gk, dim3(kBlock), 0, s, n, w.x, w.u, w.p, w.part1, w.part2,
                           w.part3, w.st, w.udr, w.hist, k, pl.maxiter, r.ctl->fail_on_maxiter);
    } else if (pl.overlap && k + 1 < pl.maxiter) {
        // the tiles holding the rows the neighbours need first, then their halo exchange on the
        // second stream while the other tiles run; the next SpMV waits for it
        pcg_k3(r, k, 0, pl.ov_lo);
        pcg_k3(r, k, pl.ov_hi, pl.nv);
        PSK_TRY(halo_exchange_async(A, pn, s, r.cs, kit->ev_a, kit->ev_b, timed ? kit->ha[slot] : nullptr,
                                    timed ? kit->hb[slot] : nullptr));
        if (timed) tm.thalo[slot] = true;
        pcg_k3(r, k, pl.ov_lo, pl.ov_hi);
        r.halo_pending = true;
    } else {
        pcg_k3(r, k, 0, pl.nv);
    }
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// the end of the loop: one launch and one synchronisation for the state, the ticket-counter scan and the gridsum
// error word, all written by pcg_finish_kernel into the host-mapped words (round 5: was two copies and a kernel)
static int pcg_finish(PcgRun &r, PcgTimers &tm, PcgState *hs, psk_result *res) {
    SolveKit *kit = r.kit;
    // a halo exchange still in flight (the host stopped enqueueing first) completes before the end
    if (r.halo_pending) PSK_HIP(hipStreamWaitEvent(r.s, kit->ev_b, 0));
    r.halo_pending = false;
    PSK_HIP(hipEventRecord(kit->ev1, r.s));
    int64_t *hw = kit->hmap + kPcgFinishWord;
    hipLaunchKernelGGL(pcg_finish_kernel, dim3(1), dim3(kBlock), 0, r.s, r.w.st, r.c->gs_cnt, r.c->gs_err, hw);
    PSK_HIP(hipGetLastError());
    PSK_HIP(hipStreamSynchronize(r.s));
    std::memcpy(hs, hw, sizeof(PcgState));
    PSK_TRY(gridsum_check_result(r.c, (int32_t)hw[kPcgStateWords]));
    if (r.pl.gen) PSK_TRY(prec_check_error(r.M, r.s));
    for (int i = 0; i < kTimedSlots; ++i) PSK_TRY(tm.harvest(i));
    res->loop_ms = loop_ms(kit);
    return PSK_OK;
}

// The state hs of a finished loop that enqueued `launched` iterations, decoded into res; the history, and x with
// whatever the end of the solve left pending. *nk: iterations whose SpMV ran (the timing count).
static int pcg_report(const PcgState &hs, const PcgPlan &pl, int64_t launched, const psk_ctl *ctl, const PcgWork &w,
                      hipStream_t s, psk_result *res, double *hist, double *xout, int32_t loc, int64_t *nk) {
    const int64_t n = pl.n, maxiter = pl.maxiter;
    res->norm_b = hs.normB;
    // nhist: iterations that reported a residual (K3 wrote hist[k]) — a dot(p,Ap) breakdown at k ran the SpMV
    // of k but reports only 0..k-1, as the reference's loop does (PCGSolver.py:114-115 returns before :126)
    int64_t nhist = 0;
    if (hs.done == 1) {
        res->status = PSK_CONVERGED;
        res->success = 1;
        res->iters = hs.iters;
        res->resid = hs.resid;
        res->exit = hs.normB == 0.0 ? PSK_EXIT_NONE : hs.resid <= hs.tauNormB ? PSK_EXIT_TOLERANCE : PSK_EXIT_MAXITER;
        *nk = nhist = hs.normB == 0.0 ? 0 : hs.iters;
    } else if (hs.done == 2) {
        res->status = PSK_BREAKDOWN;
        res->exit = PSK_EXIT_DOT_BREAKDOWN;
        res->success = 0;
        res->iters = hs.iters;
        res->resid = NAN;
        result_msg(res, hs.brk_kind == 1 ? "breakdown dot(u,r)==0" : "breakdown dot(p, Ap)==0");
        *nk = hs.brk_kind == 1 ? 0 : hs.iters + 1;
        nhist = hs.brk_kind == 1 ? 0 : hs.iters;
    } else {
        // handleMaxiter(k=maxiter-1, ...) (IterativeSolver.py:115-129); maxiter==0 -> k unset
        res->status = PSK_MAXITER;
        res->exit = PSK_EXIT_MAXITER;
        res->success = 0;
        res->iters = maxiter > 0 ? maxiter - 1 : 0;
        result_msg(res, "failure to converge");
        *nk = nhist = launched;
    }
    // residual history (only when asked for), the recursive residual and the solution
    const int64_t nh = nhist < maxiter ? nhist : maxiter;
    if (hist && nh > 0) PSK_HIP(hipMemcpy(hist, w.hist, (size_t)nh * 8, hipMemcpyDeviceToHost));
    res->hist_len = nh;
    res->resid_recursive = nh > 0 ? hs.last_hist : hs.normB;
    if (res->status == PSK_MAXITER) res->resid = maxiter > 0 ? res->resid_recursive : hs.normB;
    bool x_written = hs.x_written != 0;
    bool more = !pl.dev_io;   // work enqueued after the sync: the caller's x is ready only after another sync
    // a dot(p,Ap) breakdown at k: the iterations since the last flush deferred their x updates (staggered: every
    // SpMV launch 1 .. k ran its flush role, so the schedule says per block what is stored and what is pending;
    // uniform: one block)
    if (!pl.gen && hs.done == 2 && hs.brk_kind != 1 && n > 0) {
        bool pending = false;
        const int nblk = pl.stag ? kPcgStagger : 1;
        for (int b = 0; b < nblk; ++b) {
            if (pl.stag && (int64_t)b * pcg_block_tiles(pl.nv, kPcgStagger) >= pl.nv) continue;   // owns no tile
            const PcgPend pd = pl.stag ? pcg_flush_pending(kPcgStagger, b, hs.iters, false) : pcg_uniform_pending(hs.iters);
            pending = pending || pd.first <= pd.last;
            x_written = x_written || pd.first > 0;
        }
        if (pending) {
            PSK_TRY(launch_pcg_flush(n, w.x, w.pr, w.alphas, (int64_t)hs.iters, pl.stag, s));
            x_written = true;   // rows with nothing pending were stored by an earlier flush
            more = true;        // also when an earlier flush had already stored x
        }
    }
    // no iteration stored x (b = 0, dot(u,r) = 0 at the start, maxiter = 0, or a dot(p,Ap) breakdown at k = 0):
    // the solution is x0 = 0
    if (!x_written && n > 0) {
        PSK_HIP(hipMemsetAsync(w.x, 0, (size_t)n * 8, s));
        more = true;
    }
    if (!pl.dev_io) PSK_TRY(from_device_vec(w.x, loc, n, xout, s));
    if (more) PSK_HIP(hipStreamSynchronize(s));
    return PSK_OK;
}

// the phases in order; the caller drains the stream when one fails
static int pcg_solve(PcgRun &r, const double *b, double *xout, psk_result *res, double *hist, int32_t loc) {
    const PcgPlan &pl = r.pl;
    PSK_TRY(pcg_workspace(r.A, pl.maxiter, pl.gen, !pl.dev_io, pl.P, r.w));
    if (pl.dev_io) r.w.x = xout;
    PSK_TRY(solve_kit(r.c, r.ctl->time_kernels > 0, &r.kit));
    if (pl.overlap) PSK_TRY(comm_stream(r.c, &r.cs));
    StampPoll poll(r.kit);   // the host-mapped done stamp the kernels write (set_done)
    PcgTimers tm(r.kit, r.ctl->time_kernels, pl.init_diag, pl.maxiter);
    PSK_TRY(pcg_init(r, poll, b, loc));
    int64_t launched = 0, nk = 0;
    for (int64_t k = 0; k < pl.maxiter; ++k) {
        bool stop;
        PSK_TRY(poll.step<2>(k, pl.C, r.s, &stop));
        if (stop) break;
        PSK_TRY(pcg_iteration(r, tm, k));
        launched = k + 1;
    }
    PcgState hs;
    PSK_TRY(pcg_finish(r, tm, &hs, res));
    PSK_TRY(pcg_report(hs, pl, launched, r.ctl, r.w, r.s, res, hist, xout, loc, &nk));
    tm.finish(nk, res);
    return PSK_OK;
}

}  // namespace psk

using namespace psk;

// Per-call cost (round 4): the host-mapped poll word, the staging buffer and every
// event come from the device's SolveKit (allocated once); the init's sums and the solver state are
// finished inside the init launch; a device-resident b is read in place and a device-resident x is
// written in place (no staging copies); the history is copied back only when the caller asks for it;
// the state, the gridsum error word and the end event share ONE stream synchronisation.
extern "C" int psk_pcg(const psk_csr *Ac, const psk_prec *M, const double *b, double *xout,
                       const psk_ctl *ctl, psk_result *res, double *hist, int32_t loc) {
    if (!Ac || !b || !xout || !ctl || !res) return fail(PSK_ERR_ARG, "psk_pcg: NULL argument");
    if (ctl->maxiter < 0) return fail(PSK_ERR_ARG, "psk_pcg: maxiter < 0");
    if (M && M->n != Ac->n) return fail(PSK_ERR_ARG, "psk_pcg: preconditioner size mismatch");
    if (!Ac->comm && Ac->ncols != Ac->n) return fail(PSK_ERR_ARG, "psk_pcg: matrix must be square");
    PcgRun r{};
    r.A = const_cast<psk_csr *>(Ac);
    r.M = M;
    r.ctl = ctl;
    PSK_TRY(ctx(&r.c));
    std::lock_guard<std::mutex> solve_lock(r.c->solve_mu);
    r.s = r.c->stream;
    std::memset(res, 0, sizeof(*res));
    PSK_TRY(pcg_plan(Ac, M, ctl, loc, r.pl));
    const int rc = pcg_solve(r, b, xout, res, hist, loc);
    // a solve that failed on the host side leaves no kernel of its own running behind the next solve
    if (rc != PSK_OK) {
        if (r.halo_pending) (void)hipStreamWaitEvent(r.s, r.kit->ev_b, 0);
        (void)hipStreamSynchronize(r.s);
    }
    return rc;
}
