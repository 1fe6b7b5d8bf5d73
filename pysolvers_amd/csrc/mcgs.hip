// mcgs.hip — multicolour Gauss-Seidel preconditioner / AMG smoother (PSK_PREC_MCGS, psk_prec_create_mcgs).
//
// z = M^-1 v is `sweeps` Gauss-Seidel sweeps for A z = v from z = 0 in a colour ordering of the rows
// (color_plan.hip: first-fit greedy on the structure of A + A^T): rows of one colour do not reference each other, so a
// whole colour updates in ONE streaming launch — no dependency level, no spin wait, no grid sum — and a full sweep
// still reads A exactly once. With PSK_MCGS_SYMMETRIC the colours run 0..C-1 then C-2..0 (symmetric Gauss-Seidel,
// 2C-1 launches per sweep), which makes the operator symmetric positive definite for an SPD A, so PCG and MINRES may
// use it. No reference counterpart: the reference's Gauss-Seidel smoother is spsolve(triu(A), .)
// (ClassicSmoothers.py:22-36), a triangular solve with a dependency chain.
//
// The arithmetic, to the bit (include/psk.h states the same; tests/mcgs_oracle.py restates it in numpy): all f64,
// every operation rounded once, a product rounded before its add (the library is built with -ffp-contract=off).
//   z = 0;  repeat `sweeps` times: for colour k in ORDER, for every row i of colour k independently:
//       acc = 0.0;  acc = acc + a_ij * z_j over every stored entry of row i (diagonal included) in stored order;
//       z_i = z_i + DInv_i * (v_i - acc)
// DInv_i = 1.0 / (the sum of row i's stored col == row entries in stored order), as the Jacobi preconditioner's.
// A launch reads z_j of other colours and its rows' own z_i and writes only its own rows' z_i, so updating z in place is
// race-free and the result does not depend on the launch geometry.
//
// Layout: a colour-grouped copy of A on the device — rows of colour 0 first, then colour 1, ...; ascending row index
// inside a colour; every row's entries in their original stored order — with the original row index of each grouped
// row beside it and DInv in grouped order. Each colour's slice of it is a contiguous CSR stream.
//
// Kernels (gfx950, wave64; no floating-point atomics, no wait of a workgroup on another):
//  * mcgs_group_kernel (setup): one lane per grouped row copies the row's entries and forms DInv; the smallest row
//    with a zero, missing or non-finite diagonal goes to one device word by an integer atomic min.
//  * mcgs_color_kernel: one launch per colour — the CSR SpMV's tile schedule (spmv_csr.hip: a workgroup per tile of
//    rows of the colour's slice, the tile's colidx/vals streamed non-temporally and coalesced, rounded products
//    staged through LDS, each lane summing its own row in stored order from 0.0; rows longer than a chunk keep their
//    running sum across chunks) with the update in the epilogue: the row's index, DInv, and through the index v_i and
//    z_i are loaded before the reduction (their latency hides behind it), then one scattered 8-byte store of z_i.
//    The only reader of z_i during the launch is the workgroup that holds row i (its diagonal entry), and its store
//    comes after the last barrier of its last chunk, so every gather of the old z_i has been consumed.
//    Bytes per colour launch: 12 B per entry + 4 B per row of the slice, the row index 4, DInv 8, v 8, z_i 8 + 8, and
//    the gathers of z (other colours' lines, served by L2 / Infinity Cache beyond the first touch). Per symmetric
//    sweep on C colours: (2C-1)/C streams of A (1.5 on red/black) plus those vectors.
//  * z = 0 is a hipMemsetAsync of the caller's out. Colour 0 of the first sweep is NOT special-cased as
//    DInv_i * v_i: the stated arithmetic gives 0.0 + DInv_i * (v_i - 0.0), which differs from the bare product in the
//    sign of a zero and when a row holds a non-finite entry.
#include "psk_internal.hpp"

#include <climits>
#include <cmath>
#include <vector>

namespace psk {

struct Mcgs {
    int64_t n = 0, nnz = 0;
    int32_t ncolors = 0, sweeps = 0, flags = 0;
    int tile_rows = kBlock;
    std::vector<int64_t> cstart;   // [ncolors + 1]: grouped position of each colour's first row
    // the colour-grouped copy (owned)
    int32_t *rowptr = nullptr, *colidx = nullptr, *rows = nullptr;
    double *vals = nullptr, *dinv = nullptr;
};

void mcgs_free(Mcgs *m) {
    if (!m) return;
    void *ptrs[] = {m->rowptr, m->colidx, m->rows, m->vals, m->dinv};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete m;
}

int64_t mcgs_nnz(const Mcgs *m) { return m ? m->nnz : 0; }
int64_t mcgs_ncolors(const Mcgs *m) { return m ? m->ncolors : 0; }

namespace {

__device__ __forceinline__ int32_t ld_stream(const int32_t *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ double ld_stream(const double *p) { return __builtin_nontemporal_load(p); }

// grouped row p = row rows[p] of A: its entries in stored order to [grp[p], grp[p + 1]), DInv to dinv[p]
__global__ __launch_bounds__(kBlock) void mcgs_group_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ colidx,
                                                            const double *__restrict__ vals,
                                                            const int32_t *__restrict__ rows,
                                                            const int32_t *__restrict__ grp, int32_t *__restrict__ gcol,
                                                            double *__restrict__ gval, double *__restrict__ dinv,
                                                            int32_t *bad) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rows[p];
    const int32_t a0 = rowptr[i], a1 = rowptr[i + 1], g0 = grp[p];
    double d = 0.0;
    for (int32_t e = a0; e < a1; ++e) {
        const int32_t c = colidx[e];
        const double v = vals[e];
        gcol[g0 + (e - a0)] = c;
        gval[g0 + (e - a0)] = v;
        if (c == i) d = d + v;   // jacobi_dinv_kernel's rule
    }
    dinv[p] = 1.0 / d;
    if (!(d != 0.0) || !isfinite(d)) atomicMin(bad, i);
}

// One colour: the grouped rows [p0, p1), a tile of `trows` of them per workgroup.
//   acc = sum_j a_ij z_j (rounded products, stored order, from 0.0);  z_i = z_i + DInv_i * (v_i - acc)
// (compiled with -ffp-contract=off: every operation rounds as written). z is read and written in place: see the
// file comment for why that is race-free.
__global__ __launch_bounds__(kBlock) void mcgs_color_kernel(
    int64_t p0, int64_t p1, int trows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
    const double *__restrict__ vals, const int32_t *__restrict__ rows, const double *__restrict__ dinv,
    const double *__restrict__ v, double *z, int32_t nnz, TileMap tm) {
    constexpr int KU = kChunk / kBlock;   // staged entries per lane per chunk
    __shared__ double prod[kChunk + kBlock];   // + a dump row for lanes past the chunk's end
    const int tid = threadIdx.x;
    const int64_t t = tile_of_block(tm);
    const int64_t r0 = p0 + t * trows;
    const int64_t r1 = (r0 + trows < p1) ? r0 + trows : p1;
    const int32_t last = nnz > 0 ? nnz - 1 : 0;   // colidx/vals hold at least one (dummy) entry
    const int32_t e0 = rowptr[r0], e1 = rowptr[r1];
    // the first chunk's colidx/vals stream, clamped to valid indices (an empty tile re-reads one valid entry),
    // issued before anything else
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
    const int64_t row = r0 + tid;
    const bool has = tid < trows && row < r1;
    const int64_t rowc = has ? row : r0;   // a valid row for the unconditional epilogue loads
    const int32_t rs = rowptr[rowc], re = rowptr[rowc + 1];
    // the row's own operands, in flight during the reduction
    const int32_t i = rows[rowc];
    const double di = dinv[rowc], vi = v[i], zi = z[i];
    double sum = 0.0;
    {   // chunk 0
        const int32_t c0 = e0, c1 = (e1 - c0 > kChunk) ? c0 + kChunk : e1;
        double pv[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) pv[k] = vv[k] * z[cc[k]];   // rounded product
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
    // rare: tile longer than one chunk (a row keeps its running sum across chunks)
    for (int32_t c0 = e0 + kChunk; c0 < e1; c0 += kChunk) {
        const int32_t c1 = (e1 - c0 > kChunk) ? c0 + kChunk : e1;
        double pv[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int32_t e = c0 + k * kBlock + tid;
            const int32_t ee = e < c1 ? e : c0;
            pv[k] = ld_stream(vals + ee) * z[ld_stream(colidx + ee)];
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
    const double res = vi - sum;
    const double zn = zi + di * res;
    if (has) z[i] = zn;   // the store last, after every gather of this workgroup was consumed
}

// the colour kernel's tiles in chunks of consecutive tiles per XCD, as the CSR SpMV's (spmv_csr.hip, kCsrChunk)
constexpr int64_t kMcgsChunk = 128;

}  // namespace

int mcgs_apply(const psk_prec *M, const double *v, double *out, hipStream_t s) {
    const Mcgs *m = M->mcgs;
    const int64_t n = M->n;
    if (n == 0) return PSK_OK;
    PSK_HIP(hipMemsetAsync(out, 0, (size_t)n * sizeof(double), s));
    const int C = m->ncolors, tr = m->tile_rows;
    const int steps = (m->flags & PSK_MCGS_SYMMETRIC) ? 2 * C - 1 : C;
    for (int sw = 0; sw < m->sweeps; ++sw)
        for (int q = 0; q < steps; ++q) {
            const int k = q < C ? q : 2 * C - 2 - q;   // 0..C-1, then C-2..0
            const int64_t p0 = m->cstart[(size_t)k], p1 = m->cstart[(size_t)k + 1];
            const int64_t nt = (p1 - p0 + tr - 1) / tr;
            const TileMap tm = tile_map_chunked(nt, kMcgsChunk);
            hipLaunchKernelGGL(mcgs_color_kernel, dim3((unsigned)nt), dim3(kBlock), 0, s, p0, p1, tr,
                               (const int32_t *)m->rowptr, (const int32_t *)m->colidx, (const double *)m->vals,
                               (const int32_t *)m->rows, (const double *)m->dinv, v, out, (int32_t)m->nnz, tm);
            PSK_HIP(hipGetLastError());
        }
    return PSK_OK;
}

}  // namespace psk

using namespace psk;

extern "C" {

int psk_prec_create_mcgs(const psk_csr *A, int32_t sweeps, int32_t flags, psk_prec **out) {
    if (!A || !out) return fail(PSK_ERR_ARG, "psk_prec_create_mcgs: NULL argument");
    if (sweeps < 1) return fail(PSK_ERR_ARG, "psk_prec_create_mcgs: sweeps must be >= 1");
    if (flags & ~PSK_MCGS_SYMMETRIC) return fail(PSK_ERR_ARG, "psk_prec_create_mcgs: unknown flag");
    if (A->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_prec_create_mcgs: sharded matrices are not supported");
    if (A->n != A->ncols) return fail(PSK_ERR_ARG, "psk_prec_create_mcgs: the matrix is not square");
    if (A->n < 1) return fail(PSK_ERR_ARG, "psk_prec_create_mcgs: the matrix has no rows");
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    const int64_t n = A->n, nnz = A->nnz;
    // the structure on the host, its colouring, and the grouped order
    std::vector<int32_t> rp((size_t)n + 1), ci((size_t)(nnz > 0 ? nnz : 1)), color((size_t)n);
    PSK_HIP(hipMemcpyAsync(rp.data(), A->rowptr, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (nnz > 0) PSK_HIP(hipMemcpyAsync(ci.data(), A->colidx, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    if (rp[0] != 0 || rp[(size_t)n] != nnz) return fail(PSK_ERR_ARG, "psk_prec_create_mcgs: inconsistent row pointers");
    int32_t C = 0;
    PSK_TRY(psk_color_plan(n, rp.data(), ci.data(), color.data(), &C));
    if (C > PSK_MCGS_MAX_COLORS)
        return fail(PSK_ERR_UNSUPPORTED, "psk_prec_create_mcgs: the colouring needs " + std::to_string(C) +
                                             " colours, more than " + std::to_string(PSK_MCGS_MAX_COLORS));
    Mcgs *m = new Mcgs();
    struct Guard {   // released on every early return
        Mcgs *&p;
        ~Guard() { mcgs_free(p); }
    } guard{m};
    m->n = n;
    m->nnz = nnz;
    m->ncolors = C;
    m->sweeps = sweeps;
    m->flags = flags;
    m->tile_rows = tile_rows_for(n, nnz);
    m->cstart.assign((size_t)C + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++m->cstart[(size_t)color[(size_t)i] + 1];
    for (int k = 0; k < C; ++k) m->cstart[(size_t)k + 1] += m->cstart[(size_t)k];
    std::vector<int32_t> rows((size_t)n), grp((size_t)n + 1);
    {
        std::vector<int64_t> fill(m->cstart.begin(), m->cstart.end() - 1);
        for (int64_t i = 0; i < n; ++i) rows[(size_t)fill[(size_t)color[(size_t)i]]++] = (int32_t)i;   // ascending inside a colour
    }
    grp[0] = 0;
    for (int64_t p = 0; p < n; ++p) {
        const int32_t i = rows[(size_t)p];
        grp[(size_t)p + 1] = grp[(size_t)p] + (rp[(size_t)i + 1] - rp[(size_t)i]);
    }
    const size_t ne = (size_t)(nnz > 0 ? nnz : 1);
    hipError_t e = hipMalloc(&m->rowptr, ((size_t)n + 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&m->rows, (size_t)n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&m->colidx, ne * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&m->vals, ne * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&m->dinv, (size_t)n * sizeof(double));
    if (e != hipSuccess) return fail(PSK_ERR_ALLOC, "psk_prec_create_mcgs: hipMalloc");
    DevBuf word;
    DevBufRelease rel{word};
    PSK_TRY(word.ensure(sizeof(int32_t)));
    int32_t bad = INT32_MAX;
    PSK_HIP(hipMemcpyAsync(word.p, &bad, sizeof(int32_t), hipMemcpyHostToDevice, s));
    PSK_HIP(hipMemcpyAsync(m->rowptr, grp.data(), ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    PSK_HIP(hipMemcpyAsync(m->rows, rows.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (nnz == 0) {   // the dummy entry the colour kernel's clamped loads may touch
        PSK_HIP(hipMemsetAsync(m->colidx, 0, sizeof(int32_t), s));
        PSK_HIP(hipMemsetAsync(m->vals, 0, sizeof(double), s));
    }
    hipLaunchKernelGGL(mcgs_group_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n,
                       (const int32_t *)A->rowptr, (const int32_t *)A->colidx, (const double *)A->vals,
                       (const int32_t *)m->rows, (const int32_t *)m->rowptr, m->colidx, m->vals, m->dinv,
                       word.as<int32_t>());
    PSK_HIP(hipGetLastError());
    PSK_HIP(hipMemcpyAsync(&bad, word.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));   // also: the host vectors above are free to go
    if (bad != INT32_MAX)
        return fail(PSK_ERR_ARG, "psk_prec_create_mcgs: the diagonal entry of row " + std::to_string(bad) +
                                     " is zero, missing or not finite");
    psk_prec *M = new psk_prec();
    M->kind = PSK_PREC_MCGS;
    M->n = n;
    M->mcgs = m;
    m = nullptr;   // owned by M now
    *out = M;
    return PSK_OK;
}

int psk_prec_mcgs_info(const psk_prec *M, int32_t *ncolors, int32_t *sweeps, int32_t *flags, int64_t *color_rows) {
    if (!M || M->kind != PSK_PREC_MCGS || !M->mcgs)
        return fail(PSK_ERR_ARG, "psk_prec_mcgs_info: not a multicolour Gauss-Seidel preconditioner");
    const Mcgs *m = M->mcgs;
    if (ncolors) *ncolors = m->ncolors;
    if (sweeps) *sweeps = m->sweeps;
    if (flags) *flags = m->flags;
    if (color_rows)
        for (int k = 0; k < m->ncolors; ++k) color_rows[k] = m->cstart[(size_t)k + 1] - m->cstart[(size_t)k];
    return PSK_OK;
}

}  // extern "C"
