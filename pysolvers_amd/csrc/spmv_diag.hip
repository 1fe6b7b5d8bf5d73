// spmv_diag.hip — the diagonal layout: the one-row kernel (spmv_diag_kernel), the pair-row kernel the 5-point
// stencils run on (spmv_diagp_kernel) with the PCG loop's x flush role, the PCG init fused into the first SpMV
// (pcg_init_diag_kernel), the detector and builder (diag_build), and the launchers.
#include "spmv.hpp"
#include "pcg_state.hpp"

#include <algorithm>
#include <climits>

namespace psk {

// this file's copy of the done flag that is never set (spmv.hpp)
static __device__ int32_t g_spmv_never_done = 0;

// Diagonal layout (round 5; DIA format, Saad's "diagonal storage", with one value per diagonal): when every
// row's entries lie, IN STORED ORDER, on a subsequence of K <= 8 diagonals c = row + d_j, and every entry
// of diagonal j holds the same double v_j (constant-coefficient stencils: FDLaplacian2D's rows are
// [diag, -m, +m, -1, +1] minus the absent neighbours, two distinct values), the whole matrix is the K
// offsets, the K values and ONE presence byte per row (bit j: the row stores an entry on diagonal j).
// Detected at creation (diag_build) by checking every stored entry against the rule, so a row's present
// diagonals, visited in j order, ARE its stored entries in stored order: each lane sums its row from 0.0
// with rounded products exactly as csr_matvec does, and y is bit-identical to the CSR and sliced layouts.
// A row-block shard of such a matrix maps columns outside [0, n) to its halo (c + lo below, c + hi
// above: the FD shard's [owned | halo_lo | halo_hi] columns), checked the same way.
// Stream: 1 B per row instead of the compact sliced layout's 12 (FD at N = 10M: 10 MB instead of 120 MB
// per SpMV); x is gathered and y written as before (16 B per row). Same 256-row slices, one row per lane,
// TPW slices per workgroup and gridsum tiles as spmv_uniform_multi_kernel: p.Ap has the same bits.
constexpr int kDiagMax = 8;
constexpr int kDiagTpw = 2;   // slices per workgroup of the one-row kernel (profiles/r5_diag_tpw_ab.txt)
struct DiagDesc {
    int32_t d[kDiagMax];   // diagonal offsets, in every row's stored order
    double v[kDiagMax];    // the value (bit pattern) of every entry on diagonal j
    int64_t lo, hi;        // local column of c = row + d: c + lo when c < 0, c + hi when c >= n (shards)
    int64_t ncols;
    int32_t K, jd;         // diagonals; jd = the one with d = 0 (-1: none)
};

__device__ __forceinline__ int64_t diag_col(const DiagDesc &dd, int64_t n, int64_t row, int j) {
    int64_t c = row + dd.d[j];
    c += c < 0 ? dd.lo : (c >= n ? dd.hi : 0);
    return c < 0 ? 0 : (c >= dd.ncols ? dd.ncols - 1 : c);   // absent diagonals gather a valid x (unused)
}

// a zero the compiler cannot see through: turns a uniform load into a per-lane (vector) load
__device__ __forceinline__ int32_t spmv_vzero() {
    int32_t z;
    __asm__ volatile("v_mov_b32 %0, 0" : "=v"(z));
    return z;
}

// a double moved one lane along the wave (DPP wavefront shift; both halves by the same pattern): SHR: lane l
// receives lane l-1's value, SHL: lane l+1's; the lane with no source keeps `edge`
template <bool SHR>
__device__ __forceinline__ double wave_shift1(double v, double edge) {
    constexpr int ctrl = SHR ? 0x138 : 0x130;   // wave_shr:1 / wave_shl:1
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(v), ctrl, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(v), ctrl, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// column of row + off under the diagonal layout's mapping (diag_col with an explicit offset)
__device__ __forceinline__ int64_t diag_col_off(const DiagDesc &dd, int64_t n, int64_t row, int64_t off) {
    int64_t c = row + off;
    c += c < 0 ? dd.lo : (c >= n ? dd.hi : 0);
    return c < 0 ? 0 : (c >= dd.ncols ? dd.ncols - 1 : c);
}

// NB (round 5): the diagonals -1 and +1 are not gathered: lane l's x[row -/+ 1] is
// lane l -/+ 1's x[row] (the d = 0 gather of the same wave), moved by a DPP wave shift; the two wave-edge
// lanes load theirs (one more load instruction, its other lanes re-reading their own x[row]). Exact for
// any mapping: the d = 0 gather of a row r >= n is diag_col(r) = the column of (r - 1) + 1. NB = 1: the
// FD stored order (0, -m, +m, -1, +1); NB = 2: sorted (-m, -1, 0, +1, +m). (Against gathers for every diagonal:
// in-loop SpMV at N = 10M 0.0587 -> 0.0550 ms, 16384^2 1.44 -> 1.28 ms, same bits; profiles/r5_diag_dpp_ab.txt.)
template <int MODE, int KM, int TPW, int NB = 0>
__global__ __launch_bounds__(kBlock) void spmv_diag_kernel(
    int64_t n, const uint8_t *__restrict__ mask, DiagDesc dd, const double *__restrict__ x, double *__restrict__ y,
    const double *__restrict__ aux_d, const double *__restrict__ aux_q, GridSum gs, const int32_t *__restrict__ done,
    TileMap tm, int64_t ntiles) {
    constexpr int JD = NB == 1 ? 0 : NB == 2 ? 2 : -1, JM1 = NB == 1 ? 3 : NB == 2 ? 1 : -1,
                  JP1 = NB == 1 ? 4 : NB == 2 ? 3 : -1;
    static_assert(NB == 0 || KM == 5, "NB: the 5-diagonal patterns only");
    // ONE memory round trip per workgroup: the done flag (a vector load, so that waiting for it leaves the
    // loads issued after it in flight), the presence bytes and every diagonal's x (clamped addresses that do
    // not depend on the bytes) all go out before anything waits. Tested first, the flag's scalar load and
    // the presence bytes each cost a round trip of their own in front of the gathers (round 5 probe).
    const int32_t dnv = (done ? done : &g_spmv_never_done)[spmv_vzero()];
    const int tid = threadIdx.x;
    const int64_t grp = tile_of_block(tm);
    int64_t tl[TPW];
    bool tv[TPW];
    uint32_t mk[TPW];
    double xv[TPW][KM], eq[TPW], xe[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t t = grp * TPW + q;
        tv[q] = t < ntiles;
        tl[q] = tv[q] ? t : ntiles - 1;
        mk[q] = __builtin_nontemporal_load(mask + tl[q] * kSlice + tid);   // padded to whole slices
    }
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t row = tl[q] * kSlice + tid;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (NB && (j == JM1 || j == JP1)) continue;   // from the d = 0 value of the neighbouring lane
            const int64_t c = diag_col(dd, n, row, j);
            xv[q][j] = x[c];
            if (MODE == kSpmvJacobiDot) xv[q][j] = aux_d[c] * xv[q][j];   // (DInv*q)[c], rounded
        }
        if (NB) {   // the wave-edge lanes' neighbours: lane 0 x[row - 1], lane 63 x[row + 1]
            const int lane = tid & 63;
            const int64_t c = diag_col_off(dd, n, row, lane == 0 ? -1 : (lane == 63 ? 1 : 0));
            xe[q] = x[c];
            if (MODE == kSpmvJacobiDot) xe[q] = aux_d[c] * xe[q];
        }
        eq[q] = 0.0;
        if (MODE == kSpmvResid || MODE == kSpmvAdd || MODE == kSpmvJacobiDot || MODE == kSpmvPlainDot)
            eq[q] = aux_q[row < n ? row : 0];
    }
    // the tiles' gridsum tickets drawn now, while the loads are in flight (their values are read at publish)
    constexpr bool PUB = MODE != kSpmvPlain && MODE != kSpmvAdd;
    const bool pub = PUB && spmv_publishes<MODE>(gs);
    uint32_t ticket[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        ticket[q] = 0;
        if (pub && tv[q] && gs.grp_log2 >= 0 && tid == 0)
            ticket[q] = gridsum_draw(gridsum_counter(gs, gridsum_group_of(tl[q], gs.grp_log2)));
    }
    if (__builtin_amdgcn_readfirstlane(dnv) != 0) {   // uniform: the solve has stopped
        // consumed on this path too, so the loads are issued before the test on both; the tickets are
        // handed back (every workgroup of this launch leaves here: nobody reduces)
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
            __asm__ volatile("" ::"v"(mk[q]));
            if (NB) __asm__ volatile("" ::"v"(xe[q]));
#pragma unroll
            for (int j = 0; j < KM; ++j)
                if (!(NB && (j == JM1 || j == JP1))) __asm__ volatile("" ::"v"(xv[q][j]));
            if (pub && tv[q] && gs.grp_log2 >= 0 && tid == 0)
                __hip_atomic_fetch_sub(gridsum_counter(gs, gridsum_group_of(tl[q], gs.grp_log2)), 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    __shared__ GridSumTile<1> gsl[TPW];
    if (pub) {
        if (tid < TPW) gsl[tid].cnt = 0;
        if (tid == 0 && blockIdx.x == 0 && (gs.nt + TPW - 1) / TPW != gridDim.x) atomicOr(gs.err, 2);
        __syncthreads();
    }
    double acc[TPW], yv[TPW];
    if (NB) {
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
            xv[q][JM1] = wave_shift1<true>(xv[q][JD], xe[q]);
            xv[q][JP1] = wave_shift1<false>(xv[q][JD], xe[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t row = tl[q] * kSlice + tid;
        const bool has = tv[q] && row < n;
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < KM; ++j) {   // stored order, rounded product; absent diagonals by a select
            const double t = sum + dd.v[j] * xv[q][j];
            sum = ((mk[q] >> j) & 1u) ? t : sum;
        }
        if (MODE == kSpmvDot) {   // x[row]: the gathered diagonal when the row stores it
            double d = 0.0;
            bool found = false;
#pragma unroll
            for (int j = 0; j < KM; ++j) {
                const bool here = j == dd.jd && ((mk[q] >> j) & 1u);
                d = here ? xv[q][j] : d;
                found = found || here;
            }
            if (!found && has) d = x[row];   // rare: a row without its diagonal
            eq[q] = d;
        }
        yv[q] = spmv_row_value<MODE>(has, sum, eq[q], acc[q]);
    }
    if (pub) spmv_publish_multi<TPW>(gs, gsl, acc, ticket, tl, tv);
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t row = tl[q] * kSlice + tid;
        spmv_store_row<MODE>(tv[q] && row < n, row, yv[q], y);
    }
}

// ---- Pair-row diagonal SpMV (round 6): 16-B accesses, two CONTIGUOUS rows per lane ---------------------
// spmv_diag_kernel gives each lane one row of a slice: every x gather, the y store and the aux loads move 8 B
// per lane, the rate the guide puts at 0.54-0.70x of 16-B accesses (MI355X_MICROARCH.md, L2 table). Here a
// lane owns rows (2l, 2l+1) of a 128-row half-slice, so x[row + d] for both rows is ONE 16-B load (8-B aligned
// when d is odd; the rare pair whose two columns are not adjacent after the shard mapping — it straddles
// column 0, n or the halo — is loaded element-wise), as are y, aux_q and aux_d; the presence bytes are one
// 2-B load. The -1/+1 diagonals: row 2l's +1 and row 2l+1's -1 are the lane's own pair, row 2l's -1 and row
// 2l+1's +1 come from the neighbouring lanes by DPP wave shifts (NB orders only). A wave owns the two
// half-slices of a whole 256-row slice = one gridsum tile (4 slices per workgroup): it publishes its tile's slot
// itself — no LDS combine, no workgroup barrier; the halves' edge columns come from each other by readlane, so
// one edge load per wave. (Two waves per slice, their totals combined in LDS, measured slower:
// profiles/r6_diag_pair_ab.txt.)
// Bits: y as spmv_diag_kernel (each row summed from 0.0 in stored order). p.Ap: the tile sum of the one-row
// kernels is ((T0 + T1) + T2) + T3 over their wave totals T_w = wave_total over 64 rows; a lane here holds
// the first level of that tree (a_{2l} + a_{2l+1}), and diag_pair_totals runs the remaining levels in the same
// operand pairs, so p.Ap is bit-identical to the CSR, sliced and one-row diagonal kernels.

// 16-B accesses at 8-B alignment (x + row + d with d odd; aux arrays that are column views)
typedef double dv2u __attribute__((ext_vector_type(2), aligned(8)));
__device__ __forceinline__ dv2 ldu2(const double *p) {
    const dv2u v = *reinterpret_cast<const dv2u *>(p);
    return dv2{v.x, v.y};
}
__device__ __forceinline__ dv2 ldu2nt(const double *p) {
    const dv2u v = __builtin_nontemporal_load(reinterpret_cast<const dv2u *>(p));
    return dv2{v.x, v.y};
}
__device__ __forceinline__ void stu2(double *p, dv2 v) { *reinterpret_cast<dv2u *>(p) = dv2u{v.x, v.y}; }
__device__ __forceinline__ void stu2nt(double *p, dv2 v) {
    __builtin_nontemporal_store(dv2u{v.x, v.y}, reinterpret_cast<dv2u *>(p));
}

// the wave totals of the two 64-row halves of a 128-row half-slice whose lane l holds v = a_{2l} + a_{2l+1}:
// wave_total's levels after its first (quad_perm [1,0,3,2] on a_{2l}, a_{2l+1}) in the same operand pairs —
//   quad sums: lanes 2j, 2j+1 of the pair layout hold the one-row layout's quad j;
//   wave_total's row_ror 4 then row_ror 8 leave ((Q0 + Q3) + (Q2 + Q1)) in lane 0 of each 16-lane row: here a
//   row's four quads are lanes 8r..8r+7, so row_half_mirror puts Q0 + Q3 in lane 8r and Q2 + Q1 in lane 8r+4,
//   and row_shl 4 adds the latter to the former;
//   the four row totals of a one-row wave (its lanes 0/16/32/48) are lanes 0/8/16/24 (first half) and
//   32/40/48/56 (second half), added in that order.
__device__ __forceinline__ double lane_f64(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l),
                            __builtin_amdgcn_readlane(__double2loint(x), l));
}
__device__ __forceinline__ void diag_pair_totals(double v, double &t0, double &t1) {
    v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_f64<0x141>(v);   // row_half_mirror
    v += dpp_f64<0x104>(v);   // row_shl:4
    t0 = ((lane_f64(v, 0) + lane_f64(v, 8)) + lane_f64(v, 16)) + lane_f64(v, 24);
    t1 = ((lane_f64(v, 32) + lane_f64(v, 40)) + lane_f64(v, 48)) + lane_f64(v, 56);
}

// x at the columns of rows r, r + 1 on diagonal offset d (the diag_col mapping): one 16-B load at the pair's
// first column when the two columns are adjacent and in range. The rare pair that is not (it straddles column
// 0 or n, or a shard's halo) is marked in `fix` and re-read element-wise by diag_pair_fix once every load of
// the wave has been issued and waited for: a fix-up branch between the loads put a vmcnt wait (the pair load
// and the element loads share their destination registers) in front of every later gather
struct PairFix {
    int64_t c0, c1;   // the clamped columns (diag_col's clamp)
    bool bad;         // not one 16-B pair
};
__device__ __forceinline__ dv2 diag_pair_x(const DiagDesc &dd, int64_t n, int64_t r, int64_t d,
                                           const double *__restrict__ x, PairFix &f) {
    int64_t c0 = r + d, c1 = c0 + 1;
    c0 += c0 < 0 ? dd.lo : (c0 >= n ? dd.hi : 0);
    c1 += c1 < 0 ? dd.lo : (c1 >= n ? dd.hi : 0);
    f.bad = !(c1 == c0 + 1 && c0 >= 0 && c1 < dd.ncols);
    f.c0 = c0 < 0 ? 0 : (c0 >= dd.ncols ? dd.ncols - 1 : c0);
    f.c1 = c1 < 0 ? 0 : (c1 >= dd.ncols ? dd.ncols - 1 : c1);
    const int64_t a = c0 < 0 ? 0 : (c0 > dd.ncols - 2 ? dd.ncols - 2 : c0);   // ncols >= 2 (host check)
    return ldu2(x + a);
}
__device__ __forceinline__ void diag_pair_fix(dv2 &v, const PairFix &f, const double *__restrict__ x) {
    if (f.bad) {
        v.x = x[f.c0];
        v.y = x[f.c1];
    }
}

// ---- the PCG loop's x flush as a second role of the in-loop launch (pcg_state.hpp: the staggered flush) ----
// The launch of iteration k carries, beside its stencil workgroups, one flush workgroup per K3 tile of block
// k mod S of x. A flush workgroup streams: it issues every load of its 512 rows (x unless still implicit, the
// q <= S pending p's; 16-B, non-temporal, as K3's flush), consumes them in iteration order and stores x. It
// draws no gridsum ticket, publishes nothing and exits at once when the solve has stopped. It reads x, p_{k-q}
// .. p_{k-1} and alphas, none of which the stencil workgroups (x = p_k -> y = Ap) touch, and writes rows of x
// no other workgroup of the launch owns.
// Placement: workgroups are dealt in octets (8 consecutive blocks, one per XCD), an octet being all stencil or all
// flush, so a stencil workgroup's index among the stencil workgroups keeps blockIdx.x mod 8 and the XCD bands of
// the TileMap hold. The flush octets are dealt at a uniform ratio among the stencil octets (octet o is a flush
// octet iff (o mul) >> 16 steps there): all of them first or all last measured 5-7% slower.
// mul == 0 (a ratio the 16-bit step cannot express): the flush octets follow the stencil octets.
// The flush octets among the launch's first o octets:
__host__ __device__ inline uint32_t spmv_flush_octets_before(const SpmvFlush &f, uint32_t o) {
    if (f.mul == 0) return o > f.ost ? o - f.ost : 0;
    return (uint32_t)(((uint64_t)o * f.mul) >> 16);
}
__device__ __forceinline__ const SpmvFlush &spmv_flush_arg(const SpmvFlush &f) { return f; }

template <int S>
__device__ __forceinline__ void spmv_flush_tile(const SpmvFlush &fl, uint32_t f, int64_t n) {
    const int64_t k = fl.k;
    const int blk = (int)(k % S);
    const PcgPend pd = pcg_flush_pending(S, blk, k, true);
    const int q = (int)(k - pd.first);   // 1 .. S pending iterations
    const bool x0 = pd.first == 0;       // never stored: the implicit x0 = 0
    const int64_t i = ((int64_t)blk * pcg_block_tiles(fl.nv, S) + f) * kVecTile + 2 * threadIdx.x;
    double *__restrict__ x = fl.x;
    if (i + 1 < n) {
        dv2 xo{0.0, 0.0};
        if (!x0) xo = ld2nt(x + i);
        dv2 pp[S];
#pragma unroll
        for (int t = 1; t <= S; ++t)
            if (t <= q) pp[t - 1] = ld2nt(fl.pr.b[(k - t) % kPcgDefer] + i);
#pragma unroll
        for (int t = S; t >= 1; --t)
            if (t <= q) {
                const double a = fl.alphas[k - t];
                xo.x = xo.x + a * pp[t - 1].x;           // x = x + alpha*p  (PCGSolver.py:121, iteration k-t)
                xo.y = xo.y + a * pp[t - 1].y;
            }
        st2nt(x + i, xo);
    } else if (i < n) {
        x[i] = pcg_catch_up(x0 ? 0.0 : x[i], &fl.pr, pd.first, k, fl.alphas, i);
    }
}

// 8 workgroups per CU (<= 64 VGPRs) where that does not spill: the modes with aux loads keep more in flight and
// are left at 4
// FLUSH: empty, or one SpmvFlush — the launch then carries the flush role (kSpmvDot only; the other
// instantiations' arguments and registers are those of the kernel without it)
template <int MODE, int NB, typename... FLUSH>
__global__ __launch_bounds__(kBlock, (MODE != kSpmvPlain && MODE != kSpmvDot) ? 4 : 8) void spmv_diagp_kernel(
    int64_t n, const uint8_t *__restrict__ mask, DiagDesc dd, const double *__restrict__ x, double *__restrict__ y,
    const double *__restrict__ aux_d, const double *__restrict__ aux_q, GridSum gs, const int32_t *__restrict__ done,
    TileMap tm, int64_t ntiles, FLUSH... flush) {
    constexpr int KM = 5;
    constexpr int H = 2;   // the half-slices of the wave's slice
    constexpr bool FL = sizeof...(FLUSH) == 1;
    static_assert(sizeof...(FLUSH) <= 1 && (!FL || (MODE == kSpmvDot && kPcgStagger > 0)),
                  "the flush role rides on the PCG loop's launch only");
    static_assert(NB == 1 || NB == 2, "the 5-diagonal DPP orders");
    constexpr int JD = NB == 1 ? 0 : 2, JM1 = NB == 1 ? 3 : 1, JP1 = NB == 1 ? 4 : 3;
    constexpr int GD = NB == 1 ? 0 : 1;   // the d = 0 pair among the three gathered diagonals
    constexpr int TPB = kWaves;           // slices (gridsum tiles) per workgroup: a wave each
    constexpr bool JX = MODE == kSpmvJacobiDot;           // gathers of (DInv * q)[c]
    constexpr bool EQ = MODE == kSpmvResid || MODE == kSpmvAdd || MODE == kSpmvJacobiDot || MODE == kSpmvPlainDot;
    const int32_t dnv = (done ? done : &g_spmv_never_done)[spmv_vzero()];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t sidx = blockIdx.x, scnt = gridDim.x;   // this workgroup's index among the stencil workgroups, their count
    if constexpr (FL) {
        const SpmvFlush &fl = spmv_flush_arg(flush...);
        const uint32_t o = blockIdx.x >> 3, fb = spmv_flush_octets_before(fl, o);
        if (spmv_flush_octets_before(fl, o + 1) != fb) {   // a flush octet
            const uint32_t f = fb * 8 + (blockIdx.x & 7);
            if (f >= fl.nfl || __builtin_amdgcn_readfirstlane(dnv) != 0) return;   // no tile, or the solve has stopped
            spmv_flush_tile<kPcgStagger>(fl, f, n);
            return;
        }
        sidx = (int64_t)(o - fb) * 8 + (blockIdx.x & 7);
        scnt = (gs.nt + TPB - 1) / TPB;
        if (sidx >= scnt) return;   // the last stencil octet's spare workgroups
    }
    const int64_t grp = tile_of_index(tm, sidx, scnt);
    const int64_t t = grp * TPB + wave;   // this wave's slice
    const bool tv = t < ntiles;           // wave-uniform
    const int64_t tl = tv ? t : ntiles - 1;
    const int64_t r0 = tl * kSlice;       // first row of the wave's first half
    uint32_t mk[H];
    dv2 xv[H][3], dg[H][3], eq[H];
    PairFix fx[H][3];
    double xe, de = 1.0;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int64_t row = r0 + 128 * h + 2 * lane;
        mk[h] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(mask + row));   // padded slices
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int64_t row = r0 + 128 * h + 2 * lane;
        int g = 0;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j == JM1 || j == JP1) continue;   // from the d = 0 pair (own lane and neighbours)
            xv[h][g] = diag_pair_x(dd, n, row, dd.d[j], x, fx[h][g]);
            if (JX) dg[h][g] = diag_pair_x(dd, n, row, dd.d[j], aux_d, fx[h][g]);
            ++g;
        }
        eq[h] = dv2{0.0, 0.0};
        if (EQ) eq[h] = ldu2(aux_q + (row + 1 < n ? row : (n >= 2 ? n - 2 : 0)));   // n >= 2 (host check)
    }
    {   // the wave's edge columns: lane 0 x[first row - 1], lane 63 x[last row + 1]; the other lanes re-read
        // their own x[row] (one load instruction, no branch)
        const int64_t er = lane == 0 ? r0 - 1 : (lane == 63 ? r0 + 128 * H : r0 + 2 * lane);
        const int64_t c = diag_col_off(dd, n, er, 0);
        xe = x[c];
        if (JX) de = aux_d[c];
    }
    constexpr bool PUB = MODE != kSpmvPlain && MODE != kSpmvAdd;
    const bool pub = PUB && spmv_publishes<MODE>(gs);
    // the slice's ticket (drawn after the loads: drawn before them, its return held the loads' consumption back —
    // in-loop SpMV 0.049 -> 0.060 ms at N = 10M, profiles/r6_diagp_epilogue_ab.txt)
    uint32_t ticket = 0;
    if (pub && tv && gs.grp_log2 >= 0 && lane == 0)
        ticket = gridsum_draw(gridsum_counter(gs, gridsum_group_of(tl, gs.grp_log2)));
    if (__builtin_amdgcn_readfirstlane(dnv) != 0) {   // uniform: the solve has stopped; tickets handed back
#pragma unroll
        for (int h = 0; h < H; ++h) {
            __asm__ volatile("" ::"v"(mk[h]));
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                __asm__ volatile("" ::"v"(xv[h][g].x), "v"(xv[h][g].y));
                if (JX) __asm__ volatile("" ::"v"(dg[h][g].x), "v"(dg[h][g].y));
            }
            if (EQ) __asm__ volatile("" ::"v"(eq[h].x), "v"(eq[h].y));
        }
        __asm__ volatile("" ::"v"(xe), "v"(de));
        if (pub && tv && gs.grp_log2 >= 0 && lane == 0)
            __hip_atomic_fetch_sub(gridsum_counter(gs, gridsum_group_of(tl, gs.grp_log2)), 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if constexpr (FL) {   // the grid against the prepared one: the stencil octets only
        const SpmvFlush &fl = spmv_flush_arg(flush...);
        const uint32_t ot = gridDim.x >> 3;
        if (pub && threadIdx.x == 0 && sidx == 0 &&
            ((gridDim.x & 7) != 0 || (scnt + 7) / 8 != (int64_t)(ot - spmv_flush_octets_before(fl, ot))))
            atomicOr(gs.err, 2);
    } else {
        if (pub && threadIdx.x == 0 && blockIdx.x == 0 && (gs.nt + TPB - 1) / TPB != gridDim.x) atomicOr(gs.err, 2);
    }
    // the rare pairs that are not one 16-B load, then (DInv*q)[c] products (JX), all after every load was issued
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            diag_pair_fix(xv[h][g], fx[h][g], x);
            if (JX) {
                diag_pair_fix(dg[h][g], fx[h][g], aux_d);
                xv[h][g].x = dg[h][g].x * xv[h][g].x;   // (DInv*q)[c], rounded
                xv[h][g].y = dg[h][g].y * xv[h][g].y;
            }
        }
    if (JX) xe = de * xe;
    // the +-1 neighbours: g = GD is the d = 0 pair (x[row], x[row + 1]) of every lane
    double xl[H], xr[H];   // x[row - 1] of the lane's first row, x[row + 2] of its second
    const double a63 = lane_f64(xv[0][GD].y, 63), b0 = lane_f64(xv[1][GD].x, 0);
    xl[0] = wave_shift1<true>(xv[0][GD].y, xe);      // lane 0: the loaded x[r0 - 1]
    xr[0] = wave_shift1<false>(xv[0][GD].x, b0);     // lane 63: row 128 = half 1's lane 0
    xl[1] = wave_shift1<true>(xv[1][GD].y, a63);     // lane 0: row 127 = half 0's lane 63
    xr[1] = wave_shift1<false>(xv[1][GD].x, xe);     // lane 63: the loaded x[r0 + 256]
    double acc[H];
    dv2 yv[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int64_t row = r0 + 128 * h + 2 * lane;
        // the five diagonals' x of each row in j order (stored order)
        double c0[KM], c1[KM];
        int g = 0;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j == JM1) {
                c0[j] = xl[h];
                c1[j] = xv[h][GD].x;
            } else if (j == JP1) {
                c0[j] = xv[h][GD].y;
                c1[j] = xr[h];
            } else {
                c0[j] = xv[h][g].x;
                c1[j] = xv[h][g].y;
                ++g;
            }
        }
        const uint32_t m0 = mk[h] & 0xffu, m1 = mk[h] >> 8;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int j = 0; j < KM; ++j) {   // stored order, rounded product; absent diagonals by a select
            const double u0 = s0 + dd.v[j] * c0[j], u1 = s1 + dd.v[j] * c1[j];
            s0 = ((m0 >> j) & 1u) ? u0 : s0;
            s1 = ((m1 >> j) & 1u) ? u1 : s1;
        }
        const bool has0 = tv && row < n, has1 = tv && row + 1 < n;
        double e0 = eq[h].x, e1 = eq[h].y;
        if (EQ && row + 1 >= n) {   // the last pair of an odd n: aux_q was loaded one row early
            e0 = eq[h].y;
            e1 = 0.0;
        }
        if (MODE == kSpmvDot) {   // x[row]: the d = 0 gather when the row stores its diagonal
            const bool f0 = (m0 >> JD) & 1u, f1 = (m1 >> JD) & 1u;
            e0 = f0 ? c0[JD] : 0.0;
            e1 = f1 ? c1[JD] : 0.0;
            if (!f0 && has0) e0 = x[row];   // rare: a row without its diagonal
            if (!f1 && has1) e1 = x[row + 1];
        }
        double a0, a1;
        yv[h].x = spmv_row_value<MODE>(has0, s0, e0, a0);
        yv[h].y = spmv_row_value<MODE>(has1, s1, e1, a1);
        acc[h] = a0 + a1;   // wave_total's first level
    }
    if (pub && tv) {
        double w[2 * H];
#pragma unroll
        for (int h = 0; h < H; ++h) diag_pair_totals(acc[h], w[2 * h], w[2 * h + 1]);
        // the wave is the tile
        const double s = ((w[0] + w[1]) + w[2]) + w[3];
        const uint32_t tk = __builtin_amdgcn_readfirstlane(ticket);
        if (gs.grp_log2 < 0) {
            if (lane == 0) gridsum_put(gs.gslots + tl, s);
            gridsum_final_wave<1>(gs);
        } else {
            if (lane == 0) gridsum_put(gs.slots + gridsum_slot(gs, tl), s);
            const int64_t g = gridsum_group_of(tl, gs.grp_log2);
            int64_t base;
            const int64_t cnt = gridsum_members(gs, g, base);
            if (tk == (uint32_t)(cnt - 1)) {
                double r[1];
                gridsum_take<1, 64>(gs.slots, g << gs.grp_log2, cnt, gs.err, nullptr, r);
                if (lane == 0) {
                    gridsum_reset(gridsum_counter(gs, g));
                    gridsum_put(gs.gslots + g, r[0]);
                }
                gridsum_final_wave<1>(gs);
            }
        }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {   // y after the dot epilogue (spmv_row_value)
        const int64_t row = r0 + 128 * h + 2 * lane;
        if (!tv || row >= n) continue;
        if (row + 1 < n) {
            if (MODE == kSpmvResid || MODE == kSpmvAdd) stu2(y + row, yv[h]);
            else stu2nt(y + row, yv[h]);
        } else {
            spmv_store_row<MODE>(true, row, yv[h].x, y);
        }
    }
}

// ---- the PCG init fused into the first SpMV (round 5; diagonal layout in a DPP order, unsharded, Jacobi with one
// DInv value or none): p_0 = M b (PCGSolver.py:98) computed where this SpMV gathers it (xs * b[c]: xs = the DInv
// value, or 1.0), Ap_0 = A p_0 (:111) and the three sums [p_0.Ap_0, b.b, u.r] (:113, :86, :102) through the
// SpMV's tile epilogue; the wave that finishes them runs the init's state logic (PcgInitFin, sums 1 and 2), and
// p_0 is stored for K3. One launch instead of pcg_init_kernel + the SpMV of iteration 0 (b read once, not b and
// then p_0). b.b and u.r have pcg_init_kernel's bits (same 256-row tiles, same per-row products, wave totals in
// wave order), p_0.Ap_0 and Ap_0 the SpMV's (p_0 = xs * b is the product pcg_init_kernel stores).
template <int NB>
__global__ __launch_bounds__(kBlock) void pcg_init_diag_kernel(int64_t n, const uint8_t *__restrict__ mask, DiagDesc dd,
                                                               const double *__restrict__ b, double xs,
                                                               double *__restrict__ p, double *__restrict__ y,
                                                               GridSum gs, PcgInitFin fin, TileMap tm, int64_t ntiles) {
    constexpr int TPW = kDiagTpw, KM = 5;
    static_assert(NB == 1 || NB == 2, "the DPP orders of spmv_diag_kernel");
    constexpr int JD = NB == 1 ? 0 : 2, JM1 = NB == 1 ? 3 : 1, JP1 = NB == 1 ? 4 : 3;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t grp = tile_of_block(tm);
    int64_t tl[TPW];
    bool tv[TPW];
    uint32_t mk[TPW];
    double xv[TPW][KM], xe[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t t = grp * TPW + q;
        tv[q] = t < ntiles;
        tl[q] = tv[q] ? t : ntiles - 1;
        mk[q] = __builtin_nontemporal_load(mask + tl[q] * kSlice + tid);
    }
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t row = tl[q] * kSlice + tid;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j == JM1 || j == JP1) continue;
            xv[q][j] = b[diag_col(dd, n, row, j)];
        }
        xe[q] = b[diag_col_off(dd, n, row, lane == 0 ? -1 : (lane == 63 ? 1 : 0))];
    }
    uint32_t ticket[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        ticket[q] = 0;
        if (tv[q] && gs.grp_log2 >= 0 && tid == 0)
            ticket[q] = gridsum_draw(gridsum_counter(gs, gridsum_group_of(tl[q], gs.grp_log2)));
    }
    __shared__ GridSumTile<3> gsl[TPW];
    if (tid < TPW) gsl[tid].cnt = 0;
    if (tid == 0 && blockIdx.x == 0 && (gs.nt + TPW - 1) / TPW != gridDim.x) atomicOr(gs.err, 2);
    __syncthreads();
    double acc[TPW][3], yv[TPW], pv[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t row = tl[q] * kSlice + tid;
        const bool has = tv[q] && row < n;
        const double braw = xv[q][JD];   // b[row] (the d = 0 column of a row < n is the row itself)
#pragma unroll
        for (int j = 0; j < KM; ++j)
            if (j != JM1 && j != JP1) xv[q][j] = xs * xv[q][j];   // u = precond.applyRight(r)  :98
        xe[q] = xs * xe[q];
        xv[q][JM1] = wave_shift1<true>(xv[q][JD], xe[q]);
        xv[q][JP1] = wave_shift1<false>(xv[q][JD], xe[q]);
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < KM; ++j) {   // stored order, rounded product (spmv_diag_kernel)
            const double t = sum + dd.v[j] * xv[q][j];
            sum = ((mk[q] >> j) & 1u) ? t : sum;
        }
        pv[q] = xv[q][JD];
        yv[q] = sum;
        acc[q][0] = has ? pv[q] * sum : 0.0;    // np.dot(p, Ap)  :113 (spmv_row_value's eq * sum)
        acc[q][1] = has ? braw * braw : 0.0;    // self.norm(b)   :86
        acc[q][2] = has ? pv[q] * braw : 0.0;   // np.dot(u, r)   :102
    }
    gridsum_tiles_publish<TPW, 3>(gs, gsl, acc, ticket, tl, tv, fin);
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t row = tl[q] * kSlice + tid;
        if (tv[q] && row < n) {
            __builtin_nontemporal_store(yv[q], y + row);
            p[row] = pv[q];
        }
    }
}

// (Round 5 also built K3 fused into the next SpMV — pcg_fused_kernel, 33 B/row in one launch instead of 24 + 17 in
// two, bit-identical — and a persistent form of spmv_diag_kernel; both measured no faster (profiles/
// r5_pcg_fused_ab.txt, r5_diag_tpw_ab.txt) and were removed from the product library in round 6.)


// Diagonal-layout detection: row `row`'s stored entries must be, in order, entries of strictly increasing
// diagonals j with column diag_col's mapping and value v_j; the presence byte is written (0 past n) and
// any violation sets *bad.
__global__ __launch_bounds__(kBlock) void diag_detect_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ colidx,
                                                             const double *__restrict__ vals, DiagDesc dd,
                                                             uint8_t *__restrict__ mask, int64_t npad,
                                                             int32_t *__restrict__ bad) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= npad) return;
    uint32_t mk = 0;
    if (row < n) {
        int j = 0;
        bool ok = true;
        for (int32_t e = rowptr[row]; e < rowptr[row + 1] && ok; ++e) {
            const int64_t c = colidx[e];
            const double v = vals[e];
            while (j < dd.K) {
                int64_t cj = row + dd.d[j];
                cj += cj < 0 ? dd.lo : (cj >= n ? dd.hi : 0);
                if (cj == c && same_bits(v, dd.v[j])) break;
                ++j;
            }
            if (j == dd.K) ok = false;
            else mk |= 1u << j++;
        }
        if (!ok) atomicOr(bad, 1);
    }
    mask[row] = (uint8_t)mk;
}

void diag_free(psk_csr *A) {
    if (A->dg_mask) (void)hipFree(A->dg_mask);
    A->dg_mask = nullptr;
    A->dg_K = 0;
    A->dg_jd = -1;
}

static DiagDesc diag_desc(const psk_csr *A) {
    DiagDesc dd{};
    for (int j = 0; j < kDiagMax; ++j) {
        dd.d[j] = A->dg_d[j];
        dd.v[j] = A->dg_v[j];
    }
    dd.lo = A->dg_lo;
    dd.hi = A->dg_hi;
    dd.ncols = A->ncols;
    dd.K = A->dg_K;
    dd.jd = A->dg_jd;
    return dd;
}

// The diagonal layout of A when it has one (see spmv_diag_kernel): the diagonals and their values are
// read off one full-width row of owned columns, the halo mapping of a shard from its column count, and then
// EVERY row is checked against them on the device. Quietly leaves A alone when the rule does not hold
// (force: fails with PSK_ERR_UNSUPPORTED).
int diag_build(psk_csr *A, hipStream_t s, bool force) {
    auto no = [&](const char *why) { return force ? fail(PSK_ERR_UNSUPPORTED, std::string("diagonal layout: ") + why) : PSK_OK; };
    const int64_t n = A->n, nt = (n + kSlice - 1) / kSlice;
    if (n == 0 || A->nnz == 0) return no("empty matrix");
    if (nt > INT32_MAX) return no("too many slices");
    DevBuf tmp;
    DevBufRelease rel{tmp};
    PSK_TRY(tmp.ensure((size_t)nt * 2 * sizeof(int32_t) + 64));
    int32_t *dw = tmp.as<int32_t>(), *dspan = dw + nt;
    int32_t *dbad = dw + 2 * nt;
    PSK_TRY(sliced_shape(A, s, dw, dspan));
    std::vector<int32_t> wd((size_t)nt);
    PSK_HIP(hipMemcpyAsync(wd.data(), dw, (size_t)nt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    const int32_t K = *std::max_element(wd.begin(), wd.end());
    if (K < 1 || K > kDiagMax) return no("rows wider than 8 entries");
    // the template row: a row of K entries, all in owned columns, from slices taken from the middle out
    // (a shard's first and last lines reach into its halo)
    std::vector<int32_t> rp(kSlice + 1), cols(K);
    std::vector<double> vals(K);
    int64_t trow = -1;
    for (int64_t tries = 0, i = 0; i < nt && tries < 64 && trow < 0; ++i) {
        const int64_t t = (nt / 2 + i) % nt;
        if (wd[(size_t)t] != K) continue;
        ++tries;
        const int64_t r0 = t * kSlice, nr = std::min<int64_t>(kSlice, n - r0);
        PSK_HIP(hipMemcpy(rp.data(), A->rowptr + r0, (size_t)(nr + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < nr && trow < 0; ++r) {
            if (rp[(size_t)r + 1] - rp[(size_t)r] != K) continue;
            PSK_HIP(hipMemcpy(cols.data(), A->colidx + rp[(size_t)r], (size_t)K * 4, hipMemcpyDeviceToHost));
            bool owned = true;
            for (int j = 0; j < K; ++j) owned = owned && cols[(size_t)j] >= 0 && cols[(size_t)j] < n;
            if (!owned) continue;
            PSK_HIP(hipMemcpy(vals.data(), A->vals + rp[(size_t)r], (size_t)K * 8, hipMemcpyDeviceToHost));
            trow = r0 + r;
        }
    }
    if (trow < 0) return no("no full-width row of owned columns");
    DiagDesc dd{};
    dd.K = K;
    dd.jd = -1;
    int64_t dmin = 0;
    for (int j = 0; j < K; ++j) {
        const int64_t d = (int64_t)cols[(size_t)j] - trow;
        for (int i = 0; i < j; ++i)
            if (dd.d[i] == d) return no("repeated column in a row");
        dd.d[j] = (int32_t)d;
        dd.v[j] = vals[(size_t)j];
        if (d == 0) dd.jd = j;
        dmin = std::min(dmin, d);
    }
    // halo mapping of a row-block shard with columns [owned | below | above] (psk_csr_create_fd2d_dist):
    // the lines below hold -dmin columns; a shard with one halo has it right after the owned block
    const int64_t halo = A->ncols - n;
    dd.lo = halo > 0 ? n - dmin : 0;
    dd.hi = halo > 0 && halo == -2 * dmin ? -dmin : 0;
    dd.ncols = A->ncols;
    uint8_t *mask = nullptr;
    if (hipMalloc(&mask, (size_t)nt * kSlice) != hipSuccess) {
        (void)hipGetLastError();
        return force ? fail(PSK_ERR_ALLOC, "diagonal layout: hipMalloc") : PSK_OK;
    }
    PSK_HIP(hipMemsetAsync(dbad, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(diag_detect_kernel, dim3((unsigned)nt), dim3(kBlock), 0, s, n, A->rowptr, A->colidx, A->vals, dd,
                       mask, nt * kSlice, dbad);
    int32_t bad = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, dbad, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess || bad) {
        (void)hipFree(mask);
        if (e != hipSuccess) return fail(PSK_ERR_HIP, std::string("diagonal layout: ") + hipGetErrorString(e));
        return no("an entry off the diagonals or with another value");
    }
    sliced_free(A);
    diag_free(A);
    A->dg_mask = mask;
    A->dg_K = K;
    A->dg_jd = dd.jd;
    for (int j = 0; j < kDiagMax; ++j) {
        A->dg_d[j] = j < K ? dd.d[j] : 0;
        A->dg_v[j] = j < K ? dd.v[j] : 0.0;
    }
    A->dg_lo = dd.lo;
    A->dg_hi = dd.hi;
    return PSK_OK;
}

// the DPP neighbour order of a 5-diagonal layout (spmv_diag_kernel's NB): 1 FD stored, 2 sorted, 0 neither
static int diag_nb(const psk_csr *A) {
    if (!A->dg_mask || A->dg_K != 5) return 0;
    if (A->dg_d[0] == 0 && A->dg_d[3] == -1 && A->dg_d[4] == 1) return 1;
    if (A->dg_d[2] == 0 && A->dg_d[1] == -1 && A->dg_d[3] == 1) return 2;
    return 0;
}

// the pair-row kernel's matrices: a DPP order with at least one whole pair of rows and of columns (the others,
// and every other diagonal pattern, run spmv_diag_kernel)
static bool diag_pair_rows(const psk_csr *A) { return diag_nb(A) != 0 && A->n >= 2 && A->ncols >= 2; }

bool pcg_init_diag_eligible(const psk_csr *A) { return !A->comm && A->n > 0 && diag_nb(A) != 0; }
// launch_spmv_diag's choice of spmv_diagp_kernel<kSpmvDot, NB>, unsharded
bool spmv_flush_eligible(const psk_csr *A) { return !A->comm && diag_pair_rows(A); }

// sizes the flush role of launch fl.k (fl.k, fl.nv set) beside nwgp stencil workgroups: fl.nfl = the K3 tiles of
// block k mod S (0: the block owns none), the octet counts and the interleave step; returns the launch's grid, a
// multiple of 8 whose stencil octets are exactly those nwgp needs (0: too large for one launch)
static uint32_t spmv_flush_grid(SpmvFlush &fl, int64_t nwgp) {
    constexpr int S = kPcgStagger > 0 ? kPcgStagger : 1;
    const int64_t per = pcg_block_tiles(fl.nv, S), t0 = (fl.k % S) * per;
    const int64_t nf = std::min(fl.nv, t0 + per) - t0;
    fl.nfl = nf > 0 ? (uint32_t)nf : 0;
    if (fl.nfl == 0) return 0;
    const int64_t ost = (nwgp + 7) / 8, ofl = (nf + 7) / 8;
    if ((ost + ofl + 2) * 8 > (int64_t)INT32_MAX) return 0;
    fl.ost = (uint32_t)ost;
    fl.ofl = (uint32_t)ofl;
    uint32_t ot = (uint32_t)(ost + ofl);
    const int64_t mul = (ofl * 65536 + ot - 1) / ot;   // >= ofl / ot, so the first ost + ofl octets hold ofl
    fl.mul = (uint32_t)std::min<int64_t>(std::max<int64_t>(mul, 1), 65535);
    while (ot < (uint32_t)(ost + ofl + 2) * 2 &&
           (spmv_flush_octets_before(fl, ot) < fl.ofl || ot - spmv_flush_octets_before(fl, ot) < fl.ost))
        ++ot;   // at most one stencil octet joins per step: the loop stops at exactly ost of them
    if (spmv_flush_octets_before(fl, ot) < fl.ofl || ot - spmv_flush_octets_before(fl, ot) != fl.ost) {
        fl.mul = 0;   // a ratio the 16-bit step cannot express: the flush octets after the stencil octets
        ot = (uint32_t)(ost + ofl);
    }
    return ot * 8;
}

// Tiles in XCD bands, as the sliced layouts (psk_internal.hpp). The two DPP orders run the pair-row kernel, a
// wave per slice; everything else the one-row kernel, kDiagTpw slices per workgroup.
int launch_spmv_diag(const psk_csr *A, int mode, const SpmvLaunch &L, const SpmvFlush *flush) {
    const DiagDesc dd = diag_desc(A);
    const dim3 bd(kBlock);
    const int nb = diag_nb(A);
    if (diag_pair_rows(A)) {
        const int64_t nwgp = (L.nwg + kWaves - 1) / kWaves;
        const dim3 gdp((unsigned)nwgp);
        const TileMap tmp = tile_map_for(nwgp, true, L.rev);
        // the PCG loop's launch with the flush role (pcg_state.hpp): one flush workgroup per K3 tile of block
        // k mod kPcgStagger, dealt among the stencil workgroups (spmv_flush_grid); a block that owns no tile
        // launches the kernel without the role
#if PSK_PCG_STAGGER_ON
        if (flush) {
            SpmvFlush fl = *flush;
            const uint32_t grid = spmv_flush_grid(fl, nwgp);
            if (fl.nfl > 0) {
                if (grid == 0) return fail(PSK_ERR_UNSUPPORTED, "launch_spmv: grid too large for the flush role");
                if (nb == 1)
                    hipExtLaunchKernelGGL((spmv_diagp_kernel<kSpmvDot, 1, SpmvFlush>), dim3(grid), bd, 0, L.s, L.ev0,
                                          L.ev1, 0, A->n, A->dg_mask, dd, L.x, L.y, L.aux_d, L.aux_q, L.gs, L.done, tmp,
                                          L.nwg, fl);
                else
                    hipExtLaunchKernelGGL((spmv_diagp_kernel<kSpmvDot, 2, SpmvFlush>), dim3(grid), bd, 0, L.s, L.ev0,
                                          L.ev1, 0, A->n, A->dg_mask, dd, L.x, L.y, L.aux_d, L.aux_q, L.gs, L.done, tmp,
                                          L.nwg, fl);
                PSK_HIP(hipGetLastError());
                return PSK_OK;
            }
        }
#endif
        return spmv_for_mode(mode, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (nb == 1)
                hipExtLaunchKernelGGL((spmv_diagp_kernel<M, 1>), gdp, bd, 0, L.s, L.ev0, L.ev1, 0, A->n, A->dg_mask, dd,
                                      L.x, L.y, L.aux_d, L.aux_q, L.gs, L.done, tmp, L.nwg);
            else
                hipExtLaunchKernelGGL((spmv_diagp_kernel<M, 2>), gdp, bd, 0, L.s, L.ev0, L.ev1, 0, A->n, A->dg_mask, dd,
                                      L.x, L.y, L.aux_d, L.aux_q, L.gs, L.done, tmp, L.nwg);
        });
    }
    const int64_t nwgd = (L.nwg + kDiagTpw - 1) / kDiagTpw;
    const dim3 gdd((unsigned)(nwgd > 0 ? nwgd : 1));
    const TileMap tmd = tile_map_for(nwgd, true, L.rev);
    return spmv_for_mode(mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        auto one_row = [&](auto kmc, auto nbc) {
            hipExtLaunchKernelGGL((spmv_diag_kernel<M, decltype(kmc)::value, kDiagTpw, decltype(nbc)::value>), gdd, bd,
                                  0, L.s, L.ev0, L.ev1, 0, A->n, A->dg_mask, dd, L.x, L.y, L.aux_d, L.aux_q, L.gs,
                                  L.done, tmd, L.nwg);
        };
        // a DPP order too small for whole pairs (n < 2 or ncols < 2) keeps its neighbour form
        if (nb == 1) one_row(SpmvInt<5>{}, SpmvInt<1>{});
        else if (nb == 2) one_row(SpmvInt<5>{}, SpmvInt<2>{});
        else if (A->dg_K <= 3) one_row(SpmvInt<3>{}, SpmvInt<0>{});
        else if (A->dg_K <= 5) one_row(SpmvInt<5>{}, SpmvInt<0>{});
        else one_row(SpmvInt<8>{}, SpmvInt<0>{});
    });
}

int launch_pcg_init_diag(const psk_csr *A, const double *b, double xs, double *p, double *Ap, double *out3,
                         const PcgInitFin &fin, hipStream_t s) {
    if (!pcg_init_diag_eligible(A)) return fail(PSK_ERR_ARG, "launch_pcg_init_diag: not eligible");
    Context *c;
    PSK_TRY(ctx(&c));
    const int64_t nwg = (A->n + kSlice - 1) / kSlice, nwgd = (nwg + kDiagTpw - 1) / kDiagTpw;
    GridSum gs;
    PSK_TRY(gridsum_prepare(c, nwg, 3, out3, &gs));
    const DiagDesc dd = diag_desc(A);
    const TileMap tmd = tile_map_for(nwgd, true);
    if (diag_nb(A) == 1)
        hipLaunchKernelGGL(pcg_init_diag_kernel<1>, dim3((unsigned)nwgd), dim3(kBlock), 0, s, A->n, A->dg_mask, dd, b, xs,
                           p, Ap, gs, fin, tmd, nwg);
    else
        hipLaunchKernelGGL(pcg_init_diag_kernel<2>, dim3((unsigned)nwgd), dim3(kBlock), 0, s, A->n, A->dg_mask, dd, b, xs,
                           p, Ap, gs, fin, tmd, nwg);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

}  // namespace psk
