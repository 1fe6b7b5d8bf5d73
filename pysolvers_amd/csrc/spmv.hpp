// spmv.hpp — what the SpMV files (spmv.hip, spmv_csr.hip, spmv_sliced.hip, spmv_diag.hip; csr.hip for the
// layout builders) share: the stream loads, the row value / dot epilogue every layout's kernel ends with, one
// launch function per layout and the mode dispatcher. launch_spmv itself, which every solver calls, is declared
// in psk_internal.hpp.
#pragma once
#include "psk_internal.hpp"

#include <hip/hip_ext.h>

#include <type_traits>

namespace psk {

constexpr int kSlice = kBlock;   // rows of a slice (sliced and diagonal layouts): one gridsum tile

__device__ __forceinline__ bool same_bits(double a, double b) {
    return __double_as_longlong(a) == __double_as_longlong(b);
}

// What launch_spmv hands a layout's launcher: the operands, the prepared grid sum, the dispatch's events and
// nwg = the matrix's tiles (256-row slices; tile_rows rows in the CSR layout).
struct SpmvLaunch {
    const double *x;
    double *y;
    const double *aux_d, *aux_q;
    GridSum gs;
    const int32_t *done;
    hipStream_t s;
    hipEvent_t ev0, ev1;
    bool rev;   // each XCD walks its band backwards (the PCG loop alternates directions, PSK_K23_BANDS=2)
    int64_t nwg;
};
struct SpmvFlush;
int launch_spmv_csr(const psk_csr *A, int mode, const SpmvLaunch &L);      // spmv_csr.hip
int launch_spmv_sliced(const psk_csr *A, int mode, const SpmvLaunch &L);   // spmv_sliced.hip
// flush: the launch also carries the PCG loop's x flush role (pcg_state.hpp)
int launch_spmv_diag(const psk_csr *A, int mode, const SpmvLaunch &L, const SpmvFlush *flush);   // spmv_diag.hip

// the layouts' builders (csr_choose_layout, psk_csr_layout) and their release
int sliced_build(psk_csr *A, hipStream_t s, bool force, bool pack, bool use_dict, bool force_dict);
void sliced_free(psk_csr *A);
// per 256-row slice: the widest row, and the largest |column - row| of its entries (saturated to int32)
int sliced_shape(const psk_csr *A, hipStream_t s, int32_t *width, int32_t *span);
int diag_build(psk_csr *A, hipStream_t s, bool force);
void diag_free(psk_csr *A);

// The SpMV mode as a compile-time constant: f(std::integral_constant<int, MODE>) for the mode's kernel
// instantiation, written once for every layout's launcher.
template <int V>
using SpmvInt = std::integral_constant<int, V>;
template <class F>
int spmv_for_mode(int mode, F &&f) {
    switch (mode) {
    case kSpmvPlain: f(SpmvInt<kSpmvPlain>{}); break;
    case kSpmvDot: f(SpmvInt<kSpmvDot>{}); break;
    case kSpmvJacobiDot: f(SpmvInt<kSpmvJacobiDot>{}); break;
    case kSpmvPlainDot: f(SpmvInt<kSpmvPlainDot>{}); break;
    case kSpmvResid: f(SpmvInt<kSpmvResid>{}); break;
    case kSpmvAdd: f(SpmvInt<kSpmvAdd>{}); break;
    default:
        return fail(PSK_ERR_ARG, "unknown spmv mode");
    }
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// (The done flag that is never set, g_spmv_never_done, is a static copy in each file whose kernels read it: the
// library is built without relocatable device code, so a __device__ global cannot be shared across files.)

// Stream loads of colidx/vals (read once per SpMV) are non-temporal; the x gathers keep the default
// policy so neighbouring grid lines are served from L2 / Infinity Cache (tools/spmv_lab.hip A/B:
// nt on the stream +9-12% at n = 10M / 16.7M).
__device__ __forceinline__ int32_t ld_stream(const int32_t *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ double ld_stream(const double *p) { return __builtin_nontemporal_load(p); }

// The dot epilogue of every SpMV kernel (p.Ap, q_0.u, ||b-Ax||^2): one DPP total per WAVE, the
// tile's wave totals added in LDS in wave order and published as one gridsum slot per tile
// (gridsum_tile_*, psk_internal.hpp) — no workgroup barrier at the end of a slice. Both layouts sum
// 64 rows per wave in the same lanes over the same 256-row tiles, so their grid sums are
// bit-identical.
template <int MODE>
__device__ __forceinline__ bool spmv_publishes(const GridSum &gs) {
    return MODE != kSpmvPlain && MODE != kSpmvAdd && (MODE != kSpmvResid || gs.out != nullptr);
}
template <int MODE>
__device__ __forceinline__ uint32_t spmv_begin(const GridSum &gs, GridSumTile<1> &L, int64_t t) {
    return spmv_publishes<MODE>(gs) ? gridsum_tile_begin<1>(gs, L, t) : 0u;
}
__device__ __forceinline__ void spmv_publish(const GridSum &gs, GridSumTile<1> &L, double acc, uint32_t ticket,
                                             int64_t t) {
    const double ws = wave_total(acc);
    gridsum_tile_publish<1>(gs, L, &ws, ticket, t);
}

// The row's y value and dot partial first, the y store after the
// dot epilogue (gridsum publish). On gfx950 the registers holding a store's data may not be reused
// until the store has left (a vmcnt wait that also waits for its HBM write): with the y store ahead
// of the epilogue, every wave waited for it there (kSpmvDot at N = 10M: ~9.5 us over a plain SpMV).
template <int MODE>
__device__ __forceinline__ double spmv_row_value(bool has, double sum, double eq, double &acc) {
    const double yv = MODE == kSpmvResid ? eq - sum : MODE == kSpmvAdd ? eq + sum : sum;   // :163 / VCycleManager.py:55
    acc = 0.0;
    if (has && MODE != kSpmvPlain && MODE != kSpmvAdd) acc = MODE == kSpmvResid ? yv * yv : eq * sum;
    return yv;
}
template <int MODE>
__device__ __forceinline__ void spmv_store_row(bool has, int64_t row, double yv, double *__restrict__ y) {
    if (!has) return;
    if (MODE == kSpmvResid || MODE == kSpmvAdd) y[row] = yv;
    else __builtin_nontemporal_store(yv, y + row);
}

// The dot epilogue of a workgroup holding TPW gridsum tiles: first every tile's slot is combined in LDS
// and stored (no wait of any kind), only then does a wave that published a tile holding its group's
// last ticket reduce that group. Storing every slot before any reduction keeps the protocol's
// guarantee: a reducer only waits on tiles that drew their tickets earlier, and those store all their
// slots without waiting — a wave reducing tile 0's group while tile 1's slot were still unstored could
// otherwise close a cycle of reducers across workgroups.
template <int TPW>
__device__ __forceinline__ void spmv_publish_multi(const GridSum &gs, GridSumTile<1> *L, const double *acc,
                                                   const uint32_t *ticket, const int64_t *tl, const bool *tv) {
    const bool lane0 = (threadIdx.x & 63) == 0;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bool mine[TPW];
    uint32_t tk[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        mine[q] = false;
        tk[q] = 0;
        if (!tv[q]) continue;   // uniform: the last workgroup's missing slice
        const double ws = wave_total(acc[q]);
        uint32_t old = 0;
        if (lane0) {
            L[q].part[wave] = ws;
            if (threadIdx.x == 0) L[q].ticket = ticket[q];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            old = atomicAdd(&L[q].cnt, 1u);
        }
        if (__builtin_amdgcn_readfirstlane(old) != kWaves - 1) continue;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        double sum = L[q].part[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) sum += L[q].part[w];   // wave order
        tk[q] = L[q].ticket;
        if (lane0)
            gridsum_put(gs.grp_log2 < 0 ? gs.gslots + tl[q] : gs.slots + gridsum_slot(gs, tl[q]), sum);
        mine[q] = true;
    }
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        if (!mine[q]) continue;
        if (gs.grp_log2 < 0) {
            gridsum_final_wave<1>(gs);
            continue;
        }
        const int64_t g = gridsum_group_of(tl[q], gs.grp_log2);
        int64_t base;
        const int64_t cnt = gridsum_members(gs, g, base);
        if (tk[q] != (uint32_t)(cnt - 1)) continue;
        double r[1];
        gridsum_take<1, 64>(gs.slots, g << gs.grp_log2, cnt, gs.err, nullptr, r);
        if (lane0) {
            gridsum_reset(gridsum_counter(gs, g));
            gridsum_put(gs.gslots + g, r[0]);
        }
        gridsum_final_wave<1>(gs);
    }
}

}  // namespace psk
