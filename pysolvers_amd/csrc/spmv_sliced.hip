// spmv_sliced.hip — the sliced layouts (SELL-256): the general kernel (spmv_sliced_kernel), the uniform-width
// kernel (spmv_uniform_kernel) and the compact two-slices-per-workgroup kernel (spmv_uniform_multi_kernel),
// the value dictionary, the shape / fill kernels and host builder of the sliced copy, and the launcher.
#include "spmv.hpp"

#include <algorithm>
#include <climits>

namespace psk {

// Sliced layout (SELL-256): the same entries regrouped so that one workgroup owns a slice of
// kSlice = 256 rows, ONE ROW PER LANE, and slot j of the slice's rows is contiguous (slot-major).
// The stream loads stay coalesced, and each x gather instruction of a wave now reads the j-th
// entries of 64 consecutive rows: for the 5-point matrix 512 contiguous bytes of x per slot, where
// a CSR tile's gather instruction mixes the 5 neighbour offsets of ~13 rows (more cache lines and
// address work per load). Each lane still sums ITS row in stored order from 0.0 with rounded
// products, so y is bit-identical to csr_matvec and to spmv_kernel. Padding slots (rows shorter
// than the slice's widest row) are skipped. No rowptr stream, no LDS staging.
// Storage of a slice of width w (slot offset o = sl_off[t], all arrays indexed from o):
//  * values in slot PAIRS: slots 2p, 2p+1 of lane l adjacent at o + 2p*256 + 2l (one 16-B load per
//    pair); an odd last slot at o + (w-1)*256 + l;
//  * columns, by sl_fmt[t]: a "packed" slice (every column within +-32767 of its row) stores the
//    int16 deltas c - row of slots 2p, 2p+1 in ONE int32 word at word wo + p*256 + l of the word
//    stream sl_pcol (wo = sl_woff[t]; kPad16 = padding), i.e. 2 B per slot in full 256-B wave
//    loads; any other slice int32 columns at o + j*256 + l of sl_col (-1 = padding). FD: 10.4 B per
//    slot instead of 12 (every slice but a shard's halo lines).
//  * values, when the whole matrix holds at most kDictMax distinct values (bit patterns; stencils,
//    graph Laplacians, FEM on uniform meshes): a value DICTIONARY (sl_dict) and one byte per slot,
//    the indices of slots 4q..4q+3 of lane l in one 32-bit word of the word stream, after the
//    slice's column words (word wo + ceil(w/2)*256 + q*256 + l; wo + q*256 + l in a wide slice), so
//    a slice's whole stream is one contiguous run; 3 B per slot with packed columns instead of 10
//    (no sl_val then). The kernel keeps the dictionary in scalar registers and picks a
//    slot's value with a select tree (no memory instruction per slot: tools/dict_lab.hip, FD
//    16384^2: doubles 2.96 ms, indices + dict[idx] loads 2.24 ms, indices + selects 1.70 ms). The
//    dictionary entries are the matrix's own doubles, so every product, and y, is unchanged bit for
//    bit (Kourtis et al., "CSR-VI" value compression).
// tools/sell_lab.hip, tools/sell_pack_lab.hip (16384^2, back to back): CSR 3.61 ms, int32 columns
// 3.20-3.39 ms, 16-bit pairs + paired values 2.87 ms; all bit-identical.
constexpr int kDictMax = 8;     // distinct values a dictionary may hold (held in scalar registers)
constexpr int kDictCand = 64;    // candidates one detection pass collects
constexpr int kSliceRegs = 8;             // slots held in registers; wider slices take the loop below
constexpr int16_t kPad16 = INT16_MIN;     // padding slot of a packed slice
constexpr int64_t kMaxDelta16 = 32767;

// value of slot j (of w) of lane l in a slice at slot offset o
__device__ __forceinline__ int64_t sliced_vpos(int64_t o, int j, int w, int l) {
    return (j | 1) < w ? o + (int64_t)(j & ~1) * kSlice + 2 * l + (j & 1) : o + (int64_t)j * kSlice + l;
}

__device__ __forceinline__ int32_t unpack_delta(int32_t row, int16_t d) { return d == kPad16 ? -1 : row + (int32_t)d; }

// the dictionary as named scalars (an array here was promoted to per-thread LDS copies)
struct DictRegs {
    double d0, d1, d2, d3, d4, d5, d6, d7;
};

// dictionary entry idx (< DK) by selects on the index bits; the entries live in scalar registers
template <int DK>
__device__ __forceinline__ double dict_pick(const DictRegs dv, uint32_t idx) {
    if (DK == 2) return (idx & 1) ? dv.d1 : dv.d0;
    const double a0 = (idx & 1) ? dv.d1 : dv.d0, a1 = (idx & 1) ? dv.d3 : dv.d2;
    const double b0 = (idx & 2) ? a1 : a0;
    if (DK == 4) return b0;
    const double a2 = (idx & 1) ? dv.d5 : dv.d4, a3 = (idx & 1) ? dv.d7 : dv.d6;
    const double b1 = (idx & 2) ? a3 : a2;
    return (idx & 4) ? b1 : b0;
}

// a done flag that is never set, for launches without one (the kernel reads the flag without a
// branch on the pointer, so its load goes out with the slice header); this file's copy (spmv.hpp)
static __device__ int32_t g_spmv_never_done = 0;

// The dictionary entries DK needs, as scalar loads (the buffer is padded to kDictMax entries).
template <int DK>
__device__ __forceinline__ DictRegs load_dict(const double *__restrict__ sdict) {
    DictRegs dv{};
    if (DK >= 2) {
        dv.d0 = sdict[0];
        dv.d1 = sdict[1];
    }
    if (DK >= 4) {
        dv.d2 = sdict[2];
        dv.d3 = sdict[3];
    }
    if (DK >= 8) {
        dv.d4 = sdict[4];
        dv.d5 = sdict[5];
        dv.d6 = sdict[6];
        dv.d7 = sdict[7];
    }
    return dv;
}

// x[row] for the PCG dot p.Ap (kSpmvDot): the gathered value of the row's diagonal slot when it
// stores one (every 5-point row does: x[c] with c == row is the same double), else a load (rare:
// the branch is taken by the lanes whose row has no stored diagonal). Loading x[row] up front with
// the stream cost 7% of the in-loop SpMV at FD 16384^2 (one more load in the first round trip).
template <int NS>
__device__ __forceinline__ double diag_x(const int32_t *cc, const double *xv, int32_t row, const double *__restrict__ x,
                                         bool has) {
    double d = 0.0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < NS; ++j)
        if (cc[j] == row) {
            d = xv[j];
            found = true;
        }
    if (!found && has) d = x[row];
    return d;
}

// Uniform layout (every slice UW wide and packed — FD and other constant-width banded matrices):
// the width is a template parameter, so the slice's whole stream is issued as one batch of
// unconditional loads (a runtime width put a branch between consecutive loads and the compiler
// then waited on each one: four memory round trips per slice instead of two), the offsets are
// computed from the slice index, and every slot's gather is issued unconditionally (padding slots
// gather x[0], and their product is skipped). DK: dictionary size class (0 = double values in slot
// pairs, 2 / 4 / 8 entries).
template <int MODE, int DK, int UW>
__global__ __launch_bounds__(kBlock) void spmv_uniform_kernel(
    int64_t n, const int32_t *__restrict__ spcol, const double *__restrict__ sval, const double *__restrict__ sdict,
    const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ aux_d,
    const double *__restrict__ aux_q, GridSum gs, const int32_t *__restrict__ done, TileMap tm) {
    constexpr int NP = (UW + 1) / 2;                 // packed column words per lane
    constexpr int NI = DK > 0 ? (UW + 3) / 4 : 0;    // dictionary index words per lane
    const int32_t dn = *(done ? done : &g_spmv_never_done);   // tested once the stream is in flight
    const int tid = threadIdx.x;
    const int64_t t = tile_of_block(tm), row = t * kSlice + tid;
    const bool has = row < n;
    const int32_t *pword = spcol + t * (int64_t)((NP + NI) * kSlice) + tid;
    uint32_t cw[NP], iw[NI > 0 ? NI : 1];
    double vv[UW];
#pragma unroll
    for (int p = 0; p < NP; ++p) cw[p] = (uint32_t)ld_stream(pword + p * kSlice);
    if (DK > 0) {
#pragma unroll
        for (int q = 0; q < NI; ++q) iw[q] = (uint32_t)ld_stream(pword + (NP + q) * kSlice);
    } else {
        const double *v0 = sval + t * (int64_t)(UW * kSlice);
#pragma unroll
        for (int p = 0; p < UW / 2; ++p) {
            const dv2 v2 = __builtin_nontemporal_load(reinterpret_cast<const dv2 *>(v0 + 2 * p * kSlice) + tid);
            vv[2 * p] = v2.x;
            vv[2 * p + 1] = v2.y;
        }
        if (UW & 1) vv[UW - 1] = ld_stream(v0 + (UW - 1) * kSlice + tid);
    }
    const int64_t rowc = has ? row : 0;
    double eq = 0.0;
    // kSpmvDot's x[row] is not loaded here: a row that stores its diagonal gathers it below
    if (MODE == kSpmvResid || MODE == kSpmvAdd || MODE == kSpmvJacobiDot || MODE == kSpmvPlainDot) eq = aux_q[rowc];
    const DictRegs dv = load_dict<DK>(sdict);
    if (dn != 0) {   // uniform over the launch: no barrier has been passed
        // the stream loads are consumed on this path too, so the compiler issues them ahead of the
        // test instead of sinking them below it (every slice would wait on the flag first)
#pragma unroll
        for (int p = 0; p < NP; ++p) __asm__ volatile("" ::"v"(cw[p]));
        if (DK > 0) {
#pragma unroll
            for (int q = 0; q < NI; ++q) __asm__ volatile("" ::"v"(iw[q]));
        } else {
#pragma unroll
            for (int j = 0; j < UW; ++j) __asm__ volatile("" ::"v"(vv[j]));
        }
        return;
    }
    __shared__ GridSumTile<1> gsl;
    const uint32_t ticket = spmv_begin<MODE>(gs, gsl, t);
    const int32_t row32 = (int32_t)row;
    int32_t cc[UW];
    double xv[UW];
#pragma unroll
    for (int j = 0; j < UW; ++j) {
        cc[j] = unpack_delta(row32, (int16_t)((j & 1) ? (cw[j >> 1] >> 16) : (cw[j >> 1] & 0xffff)));
        const int32_t cl = cc[j] >= 0 ? cc[j] : 0;
        xv[j] = x[cl];
        if (MODE == kSpmvJacobiDot) xv[j] = aux_d[cl] * xv[j];   // (DInv*q)[c], rounded
    }
    if (DK > 0) {
#pragma unroll
        for (int j = 0; j < UW; ++j) vv[j] = dict_pick<DK>(dv, (iw[j >> 2] >> (8 * (j & 3))) & 0xff);
    }
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < UW; ++j)
        if (cc[j] >= 0) sum = sum + vv[j] * xv[j];   // stored order, rounded product
    if (MODE == kSpmvDot) eq = diag_x<UW>(cc, xv, row32, x, has);
    double acc;
    const double yv = spmv_row_value<MODE>(has, sum, eq, acc);
    if (spmv_publishes<MODE>(gs)) spmv_publish(gs, gsl, acc, ticket, t);
    spmv_store_row<MODE>(has, row, yv, y);
}

// The uniform kernel with TPW slices per workgroup, one row of each per lane (rows t*256 + lane of the
// TPW consecutive slices t of the workgroup): every stream load of all TPW slices is issued first, then
// every gather, so a wave keeps TPW times the bytes in flight of the one-slice kernel (the in-loop
// SpMV at N = 10M moves ~24 KiB per CU at once with one slice, below what streaming needs). The grid
// sums stay per 256-row slice (one gridsum tile each, its own ticket and LDS combine), so p.Ap has the
// same bits as the one-slice kernel and the CSR layout.
// This is the kernel of the COMPACT stream (odd UW, DK = 2): entry j's 1-bit value index is bit j of the last
// column word's upper half — the half an odd width leaves unused — so no index words are streamed (FD: 12
// instead of 20 B/row of stream). Two slices per workgroup: in-loop SpMV at N = 10M 0.0657 -> 0.0611 ms,
// 16384^2 1.60 -> 1.49 ms, same bits; with double values (the general path) two slices measured 4% slower,
// so the other uniform streams keep the one-slice kernel (profiles/r4_spmv_ab.txt).
template <int MODE, int DK, int UW, int TPW>
__global__ __launch_bounds__(kBlock) void spmv_uniform_multi_kernel(
    int64_t n, const int32_t *__restrict__ spcol, const double *__restrict__ sval, const double *__restrict__ sdict,
    const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ aux_d,
    const double *__restrict__ aux_q, GridSum gs, const int32_t *__restrict__ done, TileMap tm, int64_t ntiles) {
    constexpr int NP = (UW + 1) / 2;
    static_assert(DK == 2 && (UW & 1), "compact stream: odd width, 2-entry dictionary");
    const int32_t dn = *(done ? done : &g_spmv_never_done);
    const int tid = threadIdx.x;
    const int64_t grp = tile_of_block(tm);
    int64_t tl[TPW];     // slice of each part (clamped to a valid slice for the loads)
    bool tv[TPW];        // the part is a real slice
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t t = grp * TPW + q;
        tv[q] = t < ntiles;
        tl[q] = tv[q] ? t : ntiles - 1;
    }
    uint32_t cw[TPW][NP];
    double vv[TPW][UW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int32_t *pword = spcol + tl[q] * (int64_t)(NP * kSlice) + tid;
#pragma unroll
        for (int p = 0; p < NP; ++p) cw[q][p] = (uint32_t)ld_stream(pword + p * kSlice);
    }
    double eq[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t row = tl[q] * kSlice + tid;
        eq[q] = 0.0;
        if (MODE == kSpmvResid || MODE == kSpmvAdd || MODE == kSpmvJacobiDot || MODE == kSpmvPlainDot)
            eq[q] = aux_q[row < n ? row : 0];
    }
    const DictRegs dv = load_dict<DK>(sdict);
    if (dn != 0) {
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
#pragma unroll
            for (int p = 0; p < NP; ++p) __asm__ volatile("" ::"v"(cw[q][p]));
        }
        return;
    }
    constexpr bool PUB = MODE != kSpmvPlain && MODE != kSpmvAdd;
    __shared__ GridSumTile<1> gsl[TPW];
    uint32_t ticket[TPW];
    const bool pub = PUB && spmv_publishes<MODE>(gs);
    if (pub) {
        if (tid < TPW) gsl[tid].cnt = 0;
        if (tid == 0 && blockIdx.x == 0 && (gs.nt + TPW - 1) / TPW != gridDim.x) atomicOr(gs.err, 2);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
            ticket[q] = 0;
            if (tv[q] && gs.grp_log2 >= 0 && tid == 0)
                ticket[q] = gridsum_draw(gridsum_counter(gs, gridsum_group_of(tl[q], gs.grp_log2)));
        }
    }
    int32_t cc[TPW][UW];
    double xv[TPW][UW], acc[TPW], yv[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int32_t row32 = (int32_t)(tl[q] * kSlice + tid);
#pragma unroll
        for (int j = 0; j < UW; ++j) {
            cc[q][j] = unpack_delta(row32, (int16_t)((j & 1) ? (cw[q][j >> 1] >> 16) : (cw[q][j >> 1] & 0xffff)));
            const int32_t cl = cc[q][j] >= 0 ? cc[q][j] : 0;
            xv[q][j] = x[cl];
            if (MODE == kSpmvJacobiDot) xv[q][j] = aux_d[cl] * xv[q][j];
        }
    }
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t row = tl[q] * kSlice + tid;
        const bool has = tv[q] && row < n;
#pragma unroll
        for (int j = 0; j < UW; ++j) vv[q][j] = dict_pick<DK>(dv, (cw[q][NP - 1] >> (16 + j)) & 1u);
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < UW; ++j)
            if (cc[q][j] >= 0) sum = sum + vv[q][j] * xv[q][j];   // stored order, rounded product
        if (MODE == kSpmvDot) eq[q] = diag_x<UW>(cc[q], xv[q], (int32_t)row, x, has);
        // y stored after the dot epilogue (spmv_row_value)
        yv[q] = spmv_row_value<MODE>(has, sum, eq[q], acc[q]);
    }
    if (pub) spmv_publish_multi<TPW>(gs, gsl, acc, ticket, tl, tv);
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int64_t row = tl[q] * kSlice + tid;
        spmv_store_row<MODE>(tv[q] && row < n, row, yv[q], y);
    }
}

// General sliced layout (per-slice widths, offsets and formats loaded from the slice header).
// DK: dictionary size class (0 = double values, 2 / 4 / 8 entries).
template <int MODE, int DK>
__global__ __launch_bounds__(kBlock) void spmv_sliced_kernel(
    int64_t n, const int64_t *__restrict__ soff, const int64_t *__restrict__ swoff, const int8_t *__restrict__ sfmt,
    const int32_t *__restrict__ scol, const int32_t *__restrict__ spcol, const double *__restrict__ sval,
    const double *__restrict__ sdict,
    const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ aux_d,
    const double *__restrict__ aux_q, GridSum gs, const int32_t *__restrict__ done, TileMap tm) {
    if (done != nullptr && *done != 0) return;
    const int tid = threadIdx.x;
    const int64_t t = tile_of_block(tm), row = t * kSlice + tid;
    const bool has = row < n;
    const int64_t o = soff[t];
    const int w = (int)((soff[t + 1] - o) / kSlice);
    const bool packed = sfmt[t] != 0;   // uniform across the workgroup
    const int64_t wo = swoff[t];
    const int32_t *pword = spcol + wo;                                         // packed column words
    const int32_t *vword = pword + (packed ? (int64_t)((w + 1) / 2) * kSlice : 0);   // dictionary indices
    const DictRegs dv = load_dict<DK>(sdict);
    __shared__ GridSumTile<1> gsl;
    const uint32_t ticket = spmv_begin<MODE>(gs, gsl, t);
    const int32_t row32 = (int32_t)row;
    double eq = 0.0;
    if (has) {
        if (MODE == kSpmvDot && w > kSliceRegs) eq = x[row];   // register path: diag_x below
        if (MODE == kSpmvResid || MODE == kSpmvAdd || MODE == kSpmvJacobiDot || MODE == kSpmvPlainDot)
            eq = aux_q[row];
    }
    double sum = 0.0;
    if (w <= kSliceRegs) {
        int32_t cc[kSliceRegs];
        double vv[kSliceRegs], xv[kSliceRegs];
#pragma unroll
        for (int j = 0; j < kSliceRegs; ++j) {
            cc[j] = -1;
            vv[j] = 0.0;
        }
        // the slice's whole stream first (w and packed are uniform): values by pairs (or dictionary
        // index words), then columns
        int32_t vw[kSliceRegs / 4];
        if (DK > 0) {
#pragma unroll
            for (int q = 0; q < kSliceRegs / 4; ++q) vw[q] = 4 * q < w ? ld_stream(vword + q * kSlice + tid) : 0;
        } else {
#pragma unroll
            for (int p = 0; p < kSliceRegs / 2; ++p) {
                if (2 * p + 1 < w) {
                    const dv2 v2 =
                        __builtin_nontemporal_load(reinterpret_cast<const dv2 *>(sval + o + 2 * p * kSlice) + tid);
                    vv[2 * p] = v2.x;
                    vv[2 * p + 1] = v2.y;
                } else if (2 * p < w) {
                    vv[2 * p] = ld_stream(sval + o + 2 * p * kSlice + tid);
                }
            }
        }
        if (packed) {
#pragma unroll
            for (int p = 0; p < kSliceRegs / 2; ++p)
                if (2 * p < w) {
                    const int32_t word = ld_stream(pword + p * kSlice + tid);
                    cc[2 * p] = unpack_delta(row32, (int16_t)(word & 0xffff));
                    cc[2 * p + 1] = unpack_delta(row32, (int16_t)(word >> 16));
                }
        } else {
#pragma unroll
            for (int j = 0; j < kSliceRegs; ++j)
                if (j < w) cc[j] = ld_stream(scol + o + j * kSlice + tid);
        }
        if (DK > 0) {
#pragma unroll
            for (int j = 0; j < kSliceRegs; ++j)
                if (j < w) vv[j] = dict_pick<DK>(dv, ((uint32_t)vw[j >> 2] >> (8 * (j & 3))) & 0xff);
        }
#pragma unroll
        for (int j = 0; j < kSliceRegs; ++j) {   // then every gather
            xv[j] = 0.0;
            if (cc[j] >= 0) {
                xv[j] = x[cc[j]];
                if (MODE == kSpmvJacobiDot) xv[j] = aux_d[cc[j]] * xv[j];   // (DInv*q)[c], rounded
            }
        }
#pragma unroll
        for (int j = 0; j < kSliceRegs; ++j)
            if (cc[j] >= 0) sum = sum + vv[j] * xv[j];   // stored order, rounded product
        if (MODE == kSpmvDot) eq = diag_x<kSliceRegs>(cc, xv, row32, x, has);
    } else {
        for (int j = 0; j < w; ++j) {
            int32_t c;
            if (packed) {
                const int32_t word = ld_stream(pword + (int64_t)(j >> 1) * kSlice + tid);
                c = unpack_delta(row32, (int16_t)((j & 1) ? (word >> 16) : (word & 0xffff)));
            } else {
                c = ld_stream(scol + o + (int64_t)j * kSlice + tid);
            }
            if (c < 0) break;   // only padding follows a row's last entry
            double xx = x[c];
            if (MODE == kSpmvJacobiDot) xx = aux_d[c] * xx;
            const double v =
                DK > 0 ? dict_pick<DK>(dv, ((uint32_t)ld_stream(vword + (int64_t)(j >> 2) * kSlice + tid) >> (8 * (j & 3))) &
                                               0xff)
                       : ld_stream(sval + sliced_vpos(o, j, w, tid));
            sum = sum + v * xx;
        }
    }
    double acc;
    const double yv = spmv_row_value<MODE>(has, sum, eq, acc);
    if (spmv_publishes<MODE>(gs)) spmv_publish(gs, gsl, acc, ticket, t);
    spmv_store_row<MODE>(has, row, yv, y);
}

// per slice: widest row, and the largest |column - row| of its entries (saturated to int32)
__global__ __launch_bounds__(kBlock) void sliced_shape_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                              const int32_t *__restrict__ colidx,
                                                              int32_t *__restrict__ width, int32_t *__restrict__ span) {
    __shared__ int32_t sh[2 * kWaves];
    const int64_t row = (int64_t)blockIdx.x * kSlice + threadIdx.x;
    int32_t len = 0, dmax = 0;
    if (row < n) {
        const int32_t a = rowptr[row], b = rowptr[row + 1];
        len = b - a;
        for (int32_t e = a; e < b; ++e) {
            int64_t d = (int64_t)colidx[e] - row;
            d = d < 0 ? -d : d;
            const int32_t ds = d > INT32_MAX ? INT32_MAX : (int32_t)d;
            dmax = ds > dmax ? ds : dmax;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t v = __shfl_xor(len, o, 64), u = __shfl_xor(dmax, o, 64);
        len = v > len ? v : len;
        dmax = u > dmax ? u : dmax;
    }
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6] = len;
        sh[kWaves + (threadIdx.x >> 6)] = dmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t m = sh[0], dm = sh[kWaves];
        for (int i = 1; i < kWaves; ++i) {
            m = sh[i] > m ? sh[i] : m;
            dm = sh[kWaves + i] > dm ? sh[kWaves + i] : dm;
        }
        width[blockIdx.x] = m;
        span[blockIdx.x] = dm;
    }
}

int sliced_shape(const psk_csr *A, hipStream_t s, int32_t *width, int32_t *span) {
    const int64_t nt = (A->n + kSlice - 1) / kSlice;
    hipLaunchKernelGGL(sliced_shape_kernel, dim3((unsigned)nt), dim3(kBlock), 0, s, A->n, A->rowptr, A->colidx, width,
                       span);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// One detection pass for the value dictionary: every wave that meets a value (bit pattern) not in
// dict[0, nd) offers its first such value; the first kDictCand offers land in cand. No offers =
// the dictionary is complete.
__global__ __launch_bounds__(kBlock) void dict_scan_kernel(int64_t nnz, const double *__restrict__ vals,
                                                           const double *__restrict__ dict, int nd,
                                                           int32_t *__restrict__ ncand, double *__restrict__ cand) {
    __shared__ double dl[kDictMax];
    if (threadIdx.x < nd) dl[threadIdx.x] = dict[threadIdx.x];
    __syncthreads();
    double mine = 0.0;
    bool has = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * kBlock) {
        const double v = vals[i];
        bool found = false;
        for (int k = 0; k < nd && !found; ++k) found = same_bits(v, dl[k]);
        if (!found) {
            mine = v;
            has = true;
            break;
        }
    }
    const uint64_t m = __ballot(has);
    if (m != 0 && (threadIdx.x & 63) == __builtin_ctzll(m)) {
        const int32_t slot = atomicAdd(ncand, 1);
        if (slot < kDictCand) cand[slot] = mine;
    }
}

// one workgroup per slice, one lane per row (lanes past n write padding): coalesced stores
__global__ __launch_bounds__(kBlock) void sliced_fill_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ colidx,
                                                             const double *__restrict__ vals,
                                                             const int64_t *__restrict__ soff,
                                                             const int64_t *__restrict__ swoff,
                                                             const int8_t *__restrict__ sfmt, int32_t *__restrict__ scol,
                                                             int32_t *__restrict__ spcol, double *__restrict__ sval,
                                                             const double *__restrict__ sdict, int nd,
                                                             int compact) {
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x, row = t * kSlice + tid;
    const int64_t o = soff[t];
    const int w = (int)((soff[t + 1] - o) / kSlice);
    const bool packed = sfmt[t] != 0;
    const int64_t a = row < n ? rowptr[row] : 0;
    const int64_t len = row < n ? rowptr[row + 1] - a : 0;
    for (int j = 0; j < w; ++j) {
        if (!sdict) sval[sliced_vpos(o, j, w, tid)] = j < len ? vals[a + j] : 0.0;
        if (!packed) scol[o + (int64_t)j * kSlice + tid] = j < len ? colidx[a + j] : -1;
    }
    if (sdict && !compact) {   // index words; padding slots index entry 0 (never read: their column is padding)
        int32_t *vword = spcol + swoff[t] + (packed ? (int64_t)((w + 1) / 2) * kSlice : 0);
        for (int q = 0; 4 * q < w; ++q) {
            uint32_t word = 0;
            for (int b = 0; b < 4; ++b) {
                const int j = 4 * q + b;
                uint32_t k = 0;
                if (j < len)
                    while (k + 1 < (uint32_t)nd && !same_bits(sdict[k], vals[a + j])) ++k;
                word |= k << (8 * b);
            }
            vword[(int64_t)q * kSlice + tid] = (int32_t)word;
        }
    }
    if (packed)
        for (int p = 0; 2 * p < w; ++p) {
            const int j0 = 2 * p, j1 = 2 * p + 1;
            const int16_t d0 = j0 < len ? (int16_t)(colidx[a + j0] - row) : kPad16;
            const int16_t d1 = j1 < len ? (int16_t)(colidx[a + j1] - row) : kPad16;
            uint32_t hi = (uint16_t)d1;
            if (compact && j1 == w) {   // the free half: bit j = entry j's dictionary index (nd <= 2)
                hi = 0;
                for (int j = 0; j < w && j < len; ++j)
                    if (nd > 1 && !same_bits(sdict[0], vals[a + j])) hi |= 1u << j;   // the index word's k
            }
            spcol[swoff[t] + (int64_t)p * kSlice + tid] = (int32_t)((uint32_t)(uint16_t)d0 | (hi << 16));
        }
}

void sliced_free(psk_csr *A) {
    void *ptrs[] = {A->sl_off, A->sl_woff, A->sl_fmt, A->sl_col, A->sl_pcol, A->sl_val, A->sl_dict};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    A->sl_off = nullptr;
    A->sl_woff = nullptr;
    A->sl_fmt = nullptr;
    A->sl_col = nullptr;
    A->sl_pcol = nullptr;
    A->sl_val = nullptr;
    A->sl_dict = nullptr;
    A->sl_dict_n = 0;
    A->sl_uniform_w = 0;
    A->sl_compact = 0;
    A->sl_slots = 0;
    A->sl_packed_slots = 0;
    A->sl_stream_bytes = 0;
}

// The distinct values of A (bit patterns) when there are at most kDictMax of them, else empty:
// detection passes over A->vals, each adding every new value it was offered (<= kDictMax + 1 passes,
// one for a matrix of arbitrary values).
static int find_value_dict(const psk_csr *A, hipStream_t s, std::vector<double> &dict) {
    dict.clear();
    if (A->nnz == 0) return PSK_OK;
    DevBuf tmp;
    DevBufRelease rel{tmp};
    PSK_TRY(tmp.ensure((size_t)(kDictMax + kDictCand + 1) * sizeof(double)));
    double *ddict = tmp.as<double>(), *dcand = ddict + kDictMax;
    int32_t *dn = reinterpret_cast<int32_t *>(dcand + kDictCand);
    const int64_t blocks = std::min<int64_t>((A->nnz + kBlock - 1) / kBlock, 2048);
    std::vector<double> cand(kDictCand);
    for (int pass = 0; pass <= kDictMax; ++pass) {
        if (!dict.empty())
            PSK_HIP(hipMemcpyAsync(ddict, dict.data(), dict.size() * sizeof(double), hipMemcpyHostToDevice, s));
        PSK_HIP(hipMemsetAsync(dn, 0, sizeof(int32_t), s));
        hipLaunchKernelGGL(dict_scan_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, A->nnz, A->vals, ddict,
                           (int)dict.size(), dn, dcand);
        PSK_HIP(hipGetLastError());
        int32_t nc = 0;
        PSK_HIP(hipMemcpyAsync(&nc, dn, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipMemcpyAsync(cand.data(), dcand, kDictCand * sizeof(double), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipStreamSynchronize(s));
        if (nc == 0) return PSK_OK;   // every value is in the dictionary
        for (int i = 0; i < std::min(nc, kDictCand); ++i) {
            bool seen = false;
            for (double d : dict) seen = seen || std::memcmp(&d, &cand[(size_t)i], sizeof(double)) == 0;
            if (!seen) dict.push_back(cand[(size_t)i]);
            if ((int)dict.size() > kDictMax) {
                dict.clear();
                return PSK_OK;
            }
        }
    }
    dict.clear();
    return PSK_OK;
}

// Builds the sliced copy of A (pack = allow int16 column deltas, use_dict = index values through a
// dictionary when A has at most kDictMax distinct values; force_dict fails when it has more).
// Unless `force`, only when its stream is no larger than the CSR stream (12 B per entry + 4 B per
// row), i.e. padding costs nothing, and quietly keeps CSR if HBM cannot hold the copy.
int sliced_build(psk_csr *A, hipStream_t s, bool force, bool pack, bool use_dict, bool force_dict) {
    sliced_free(A);
    diag_free(A);
    std::vector<double> dict;
    if (use_dict) PSK_TRY(find_value_dict(A, s, dict));
    if (force_dict && dict.empty())
        return fail(PSK_ERR_UNSUPPORTED, "sliced layout: more than 8 distinct values, no value dictionary");
    const int64_t nt = (A->n + kSlice - 1) / kSlice;
    if (nt == 0) return PSK_OK;   // nothing to multiply (launch_spmv returns early)
    if (nt > INT32_MAX) return force ? fail(PSK_ERR_UNSUPPORTED, "sliced layout: too many slices") : PSK_OK;
    DevBuf tmp;
    DevBufRelease rel{tmp};
    PSK_TRY(tmp.ensure((size_t)nt * 2 * sizeof(int32_t)));
    int32_t *dw = tmp.as<int32_t>(), *dspan = dw + nt;
    PSK_TRY(sliced_shape(A, s, dw, dspan));
    std::vector<int32_t> wd((size_t)nt * 2);
    PSK_HIP(hipMemcpyAsync(wd.data(), tmp.p, (size_t)nt * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    // uniform: every slice padded to the widest when all pack and that pads at most 1% more slots
    // (FD: only the first and last grid lines are narrower) — the kernel then computes every
    // offset from the slice index (PSK_SPMV_UNIFORM=0 disables)
    int64_t wmax = 0, wsum = 0;
    bool all_pack = pack;
    for (int64_t t = 0; t < nt; ++t) {
        wmax = std::max<int64_t>(wmax, wd[(size_t)t]);
        wsum += wd[(size_t)t];
        all_pack = all_pack && wd[(size_t)(nt + t)] <= kMaxDelta16;
    }
    const bool uniform = all_pack && wmax > 0 && wmax <= kSliceRegs && wmax * nt * 100 <= wsum * 101;
    if (uniform)
        for (int64_t t = 0; t < nt; ++t) wd[(size_t)t] = (int32_t)wmax;
    // compact stream: uniform, odd width, a 1-bit value index
    const bool compact = uniform && !dict.empty() && dict.size() <= 2 && (wmax & 1) && wmax <= 15;
    std::vector<int64_t> off((size_t)nt + 1), woff((size_t)nt + 1);
    std::vector<int8_t> fmt((size_t)nt);
    off[0] = 0;
    woff[0] = 0;
    int64_t packed_slots = 0, col_bytes = 0, val_bytes = 0;
    for (int64_t t = 0; t < nt; ++t) {
        const int64_t w = wd[(size_t)t];
        off[(size_t)t + 1] = off[(size_t)t] + w * kSlice;
        fmt[(size_t)t] = (pack && wd[(size_t)(nt + t)] <= kMaxDelta16) ? 1 : 0;
        if (fmt[(size_t)t]) packed_slots += w * kSlice;
        col_bytes += (fmt[(size_t)t] ? 4 * ((w + 1) / 2) : 4 * w) * kSlice;
        val_bytes += (dict.empty() ? 8 * w : compact ? 0 : 4 * ((w + 3) / 4)) * kSlice;
        // the word stream: packed column words, then dictionary index words
        const int64_t words = (fmt[(size_t)t] ? (w + 1) / 2 : 0) + (dict.empty() || compact ? 0 : (w + 3) / 4);
        woff[(size_t)t + 1] = woff[(size_t)t] + words * kSlice;
    }
    const int64_t slots = off[(size_t)nt], nwords = woff[(size_t)nt];
    const int64_t wide_slots = slots - packed_slots;
    // matrix bytes one SpMV streams: values (or value indices + dictionary), columns, slice offsets
    // (two arrays) and formats
    const int64_t stream = val_bytes + 8 * (int64_t)dict.size() + col_bytes + (uniform ? 0 : 17 * nt + 16);
    if (!force && stream > 12 * A->nnz + 4 * (A->n + 1)) return PSK_OK;
    const size_t ms = slots > 0 ? (size_t)slots : 1;
    bool ok = hipMalloc(&A->sl_off, (size_t)(nt + 1) * 8) == hipSuccess &&
              hipMalloc(&A->sl_woff, (size_t)(nt + 1) * 8) == hipSuccess &&
              hipMalloc(&A->sl_fmt, (size_t)nt) == hipSuccess;
    if (ok && dict.empty()) ok = hipMalloc(&A->sl_val, ms * 8) == hipSuccess;              // indexed by slot
    if (ok && wide_slots > 0) ok = hipMalloc(&A->sl_col, ms * 4) == hipSuccess;            // indexed by slot
    if (ok && nwords > 0) ok = hipMalloc(&A->sl_pcol, (size_t)nwords * 4) == hipSuccess;   // from sl_woff[t]
    if (ok && !dict.empty()) ok = hipMalloc(&A->sl_dict, kDictMax * 8) == hipSuccess;   // padded: the kernel
                                                                                         // reads its size class
    if (!ok) {
        (void)hipGetLastError();
        sliced_free(A);
        return force ? fail(PSK_ERR_ALLOC, "sliced layout: hipMalloc") : PSK_OK;
    }
    PSK_HIP(hipMemcpyAsync(A->sl_off, off.data(), (size_t)(nt + 1) * 8, hipMemcpyHostToDevice, s));
    PSK_HIP(hipMemcpyAsync(A->sl_woff, woff.data(), (size_t)(nt + 1) * 8, hipMemcpyHostToDevice, s));
    PSK_HIP(hipMemcpyAsync(A->sl_fmt, fmt.data(), (size_t)nt, hipMemcpyHostToDevice, s));
    if (!dict.empty()) {
        std::vector<double> padded(dict);
        padded.resize(kDictMax, 0.0);
        PSK_HIP(hipMemcpyAsync(A->sl_dict, padded.data(), kDictMax * 8, hipMemcpyHostToDevice, s));
    }
    A->sl_dict_n = (int32_t)dict.size();
    A->sl_uniform_w = uniform ? (int32_t)wmax : 0;
    A->sl_compact = compact ? 1 : 0;
    hipLaunchKernelGGL(sliced_fill_kernel, dim3((unsigned)nt), dim3(kBlock), 0, s, A->n, A->rowptr, A->colidx, A->vals,
                       A->sl_off, A->sl_woff, A->sl_fmt, A->sl_col, A->sl_pcol, A->sl_val, A->sl_dict,
                       A->sl_dict_n, compact ? 1 : 0);
    PSK_HIP(hipGetLastError());
    PSK_HIP(hipStreamSynchronize(s));
    A->sl_slots = slots;
    A->sl_packed_slots = packed_slots;
    A->sl_stream_bytes = stream;
    (void)wide_slots;
    return PSK_OK;
}

// One workgroup per slice, the tiles in XCD bands (psk_internal.hpp; N = 10M in the loop 0.078 -> 0.072 ms,
// back to back 0.067 -> 0.057 ms); the compact stream two slices per workgroup.
int launch_spmv_sliced(const psk_csr *A, int mode, const SpmvLaunch &L) {
    const dim3 bd(kBlock);
    const int uw = A->sl_uniform_w;   // 0, or the uniform width (<= kSliceRegs)
    if (A->sl_compact) {              // uniform, odd width, 2-entry dictionary
        const int64_t nwg2 = (L.nwg + 1) / 2;
        const dim3 gd2((unsigned)(nwg2 > 0 ? nwg2 : 1));
        const TileMap tm2 = tile_map_for(nwg2, true, L.rev);
        return spmv_for_mode(mode, [&](auto m) {
            auto go = [&](auto w) {
                hipExtLaunchKernelGGL((spmv_uniform_multi_kernel<decltype(m)::value, 2, decltype(w)::value, 2>), gd2,
                                      bd, 0, L.s, L.ev0, L.ev1, 0, A->n, A->sl_pcol, A->sl_val, A->sl_dict, L.x, L.y,
                                      L.aux_d, L.aux_q, L.gs, L.done, tm2, L.nwg);
            };
            switch (uw) {
            case 1: go(SpmvInt<1>{}); break;
            case 3: go(SpmvInt<3>{}); break;
            case 5: go(SpmvInt<5>{}); break;
            default: go(SpmvInt<7>{}); break;
            }
        });
    }
    const dim3 gd((unsigned)L.nwg);
    const TileMap tm = tile_map_for(L.nwg, true, L.rev);
    const int dk = !A->sl_dict ? 0 : A->sl_dict_n <= 2 ? 2 : A->sl_dict_n <= 4 ? 4 : 8;
    return spmv_for_mode(mode, [&](auto m) {
        auto with_dk = [&](auto dkc) {
            constexpr int M = decltype(m)::value, DK = decltype(dkc)::value;
            auto uni = [&](auto w) {
                hipExtLaunchKernelGGL((spmv_uniform_kernel<M, DK, decltype(w)::value>), gd, bd, 0, L.s, L.ev0, L.ev1, 0,
                                      A->n, A->sl_pcol, A->sl_val, A->sl_dict, L.x, L.y, L.aux_d, L.aux_q, L.gs, L.done,
                                      tm);
            };
            switch (uw) {
            case 0:
                hipExtLaunchKernelGGL((spmv_sliced_kernel<M, DK>), gd, bd, 0, L.s, L.ev0, L.ev1, 0, A->n, A->sl_off,
                                      A->sl_woff, A->sl_fmt, A->sl_col, A->sl_pcol, A->sl_val, A->sl_dict, L.x, L.y,
                                      L.aux_d, L.aux_q, L.gs, L.done, tm);
                break;
            case 1: uni(SpmvInt<1>{}); break;
            case 2: uni(SpmvInt<2>{}); break;
            case 3: uni(SpmvInt<3>{}); break;
            case 4: uni(SpmvInt<4>{}); break;
            case 5: uni(SpmvInt<5>{}); break;
            case 6: uni(SpmvInt<6>{}); break;
            case 7: uni(SpmvInt<7>{}); break;
            default: uni(SpmvInt<8>{}); break;
            }
        };
        switch (dk) {
        case 0: with_dk(SpmvInt<0>{}); break;
        case 2: with_dk(SpmvInt<2>{}); break;
        case 4: with_dk(SpmvInt<4>{}); break;
        default: with_dk(SpmvInt<8>{}); break;
        }
    });
}

}  // namespace psk
