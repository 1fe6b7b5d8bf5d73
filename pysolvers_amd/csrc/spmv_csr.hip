// spmv_csr.hip — the CSR tile kernel (spmv_kernel), the layout of every matrix that has neither a sliced nor a
// diagonal copy, with its tile map and launcher.
//
// SpMV replaces mvmult(A, x) (IterativeLinearSolver.py:94-106) = scipy csr_matvec: for each row,
// sum = 0; sum += vals[jj] * x[colidx[jj]] in STORED order, product rounded before the add.
// We reproduce that bit for bit: the products are staged through LDS (so no FMA can form) and each
// row is summed sequentially by one lane in stored order, starting from 0.0.
//
// Layout/schedule (gfx950): one workgroup of 256 threads (4 waves) per tile of `trows` rows (256
// for 5-point rows), grid = tiles (one-shot; see gridsum in psk_internal.hpp for why). The tile's
// nnz range [rowptr[r0], rowptr[r1]) is streamed in 1280-entry chunks with fully coalesced
// non-temporal loads of colidx (4 B/lane) and vals (8 B/lane), the x gather is issued branch-free
// for 5 entries per lane, rounded products land in a 10 KiB LDS slab, and each lane then sums its
// own row from LDS. Rows longer than a chunk keep their running sum across chunks, so ANY row
// length is exact. Optional epilogues fuse the dot products the Krylov loops need next (p.Ap for
// PCG, q_0.u for GMRES, ||b-Ax||^2 for the true residual), reduced deterministically by gridsum.
#include "spmv.hpp"

namespace psk {

template <int MODE>
__global__ __launch_bounds__(kBlock) void spmv_kernel(
    int64_t n, int trows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
    const double *__restrict__ vals, const double *__restrict__ x, double *__restrict__ y,
    const double *__restrict__ aux_d, const double *__restrict__ aux_q, GridSum gs,
    const int32_t *__restrict__ done, int32_t nnz, TileMap tm) {
    if (done != nullptr && *done != 0) return;
    constexpr int KU = kChunk / kBlock;   // staged entries per lane per chunk
    __shared__ double prod[kChunk + kBlock];   // + a dump row for lanes past the chunk's end
    const int tid = threadIdx.x;
    const int64_t t = tile_of_block(tm);
    const int64_t r0 = t * trows;
    const int64_t r1 = (r0 + trows < n) ? r0 + trows : n;
    const int32_t last = nnz > 0 ? nnz - 1 : 0;   // colidx/vals hold at least one (dummy) entry
    const int32_t e0 = rowptr[r0], e1 = rowptr[r1];
    // the first chunk's colidx/vals stream, clamped to valid indices (an empty tile re-reads one
    // valid entry), issued before anything else
    int32_t cc[KU];
    double vv[KU];
    {
        const int32_t c1 = (e1 - e0 > kChunk) ? e0 + kChunk : e1;
        const int32_t base = e0 < last ? e0 : last;
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int32_t e = e0 + k * kBlock + tid;
            const int32_t ee = e < c1 ? e : base;
            cc[k] = ld_stream(colidx + ee);
            vv[k] = ld_stream(vals + ee);
        }
    }
    __shared__ GridSumTile<1> gsl;
    const uint32_t ticket = spmv_begin<MODE>(gs, gsl, t);
    const int64_t row = r0 + tid;
    const bool has = tid < trows && row < r1;
    const int64_t rowc = has ? row : r0;   // a valid row for the unconditional epilogue loads
    const int32_t rs = rowptr[rowc], re = rowptr[rowc + 1];
    double eq = 0.0;
    if (MODE == kSpmvDot) eq = x[rowc];
    if (MODE == kSpmvResid || MODE == kSpmvAdd || MODE == kSpmvJacobiDot || MODE == kSpmvPlainDot)
        eq = aux_q[rowc];
    double sum = 0.0;
    {   // chunk 0
        const int32_t c0 = e0, c1 = (e1 - c0 > kChunk) ? c0 + kChunk : e1;
        double pv[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            double xx = x[cc[k]];
            if (MODE == kSpmvJacobiDot) xx = aux_d[cc[k]] * xx;   // (DInv*q)[c], rounded
            pv[k] = vv[k] * xx;                                   // rounded product
        }
#pragma unroll
        for (int k = 0; k < KU; ++k) {   // lanes past the chunk write the dump row
            const int32_t e = c0 + k * kBlock + tid;
            prod[(e < c1 ? k * kBlock : kChunk) + tid] = pv[k];
        }
        __syncthreads();
        const int32_t a = rs > c0 ? rs : c0;
        const int32_t bnd = re < c1 ? re : c1;
        if (has)
            for (int32_t e = a; e < bnd; ++e) sum = sum + prod[e - c0];   // stored order
        __syncthreads();
    }
    // rare: tile longer than one chunk
    for (int32_t c0 = e0 + kChunk; c0 < e1; c0 += kChunk) {
        const int32_t c1 = (e1 - c0 > kChunk) ? c0 + kChunk : e1;
        double pv[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int32_t e = c0 + k * kBlock + tid;
            const int32_t ee = e < c1 ? e : c0;
            const int32_t c = ld_stream(colidx + ee);
            double xx = x[c];
            if (MODE == kSpmvJacobiDot) xx = aux_d[c] * xx;
            pv[k] = ld_stream(vals + ee) * xx;
        }
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int32_t e = c0 + k * kBlock + tid;
            if (e < c1) prod[k * kBlock + tid] = pv[k];
        }
        __syncthreads();
        const int32_t a = rs > c0 ? rs : c0;
        const int32_t bnd = re < c1 ? re : c1;
        if (has)
            for (int32_t e = a; e < bnd; ++e) sum = sum + prod[e - c0];
        __syncthreads();
    }
    double acc;
    const double yv = spmv_row_value<MODE>(has, sum, eq, acc);
    // only the residual mode may be called without partials (AMG smoothing); kernel-uniform test
    if (spmv_publishes<MODE>(gs)) spmv_publish(gs, gsl, acc, ticket, t);
    spmv_store_row<MODE>(has, row, yv, y);
}

// The CSR tile kernel's tile map (round 6): chunks of kCsrChunk consecutive tiles dealt over the
// XCDs (tile_map_chunked), so the +-m x lines a tile gathers were fetched through the same L2 by its chunk's
// neighbours; in the loop at N = 10M 0.1400 -> 0.1380 ms, back to back 0.1342 -> 0.1292 ms (block order: the x
// line neighbours land on other XCDs; the whole-band map measured 0.145 ms; profiles/r6_csr_tilemap_ab.txt).
constexpr int64_t kCsrChunk = 128;

int launch_spmv_csr(const psk_csr *A, int mode, const SpmvLaunch &L) {
    const dim3 gd((unsigned)L.nwg), bd(kBlock);
    const TileMap tm = tile_map_chunked(L.nwg, kCsrChunk);
    const int tr = A->tile_rows;
    const int32_t nz = (int32_t)A->nnz;
    return spmv_for_mode(mode, [&](auto m) {
        hipExtLaunchKernelGGL(spmv_kernel<decltype(m)::value>, gd, bd, 0, L.s, L.ev0, L.ev1, 0, A->n, tr, A->rowptr,
                              A->colidx, A->vals, L.x, L.y, L.aux_d, L.aux_q, L.gs, L.done, nz, tm);
    });
}

}  // namespace psk
