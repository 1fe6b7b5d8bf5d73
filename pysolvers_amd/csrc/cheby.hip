// cheby.hip — Chebyshev polynomial preconditioner / AMG smoother (PSK_PREC_CHEBYSHEV, psk_prec_create_chebyshev).
//
// z = M^-1 v is the degree-`degree` Chebyshev iteration for D^-1 A z = D^-1 v from z = 0, D = diag(A), on the
// interval [lmax/ratio, lmax] of D^-1 A (include/psk.h states the recurrence and its roundings). No reference
// counterpart: the reference smooths with Jacobi and Gauss-Seidel only (ClassicSmoothers.py:5-36); this is the
// smoother without a triangular solve, one bandwidth-bound pass over A per degree and no dependency chain.
//
// Kernels (gfx950, wave64):
//  * cheby_setup_kernel + cheby_max_kernel: DInv (as jacobi_dinv_kernel) and the Gershgorin bound of D^-1 A in one
//    pass over A at creation.
//  * cheby_first_kernel: step 0, elementwise.
//  * cheby_step_kernel: steps k >= 1, ONE launch each — the CSR SpMV's tile schedule (spmv_csr.hip: a workgroup per
//    tile of rows, the tile's colidx/vals streamed non-temporally, rounded products staged through LDS, each lane
//    summing its own row in stored order from 0.0) with the whole update in the epilogue. The row's v, DInv, d
//    and z_in loads are issued before the reduction (their latency hides behind it), the d and z_out stores come
//    last (a store's data registers are held until it has left). z ping-pongs between two buffers because other
//    rows gather z_in while this row writes; the last step writes the caller's out.
//    Bytes per row and step: 12 nnz/n + 4 of matrix, v 8, DInv 8, d 8 + 8, z_in 8 (its gathers are served by
//    L2 / Infinity Cache beyond the first touch), z_out 8 = 12 nnz/n + 52. The unfused composition (residual
//    SpMV, scale, two axpys) moves 12 nnz/n + 4 + 24 (SpMV: x, b, r) + 24 (scale) + 24 + 24 (axpys) = 12 nnz/n + 100
//    in four launches.
#include "psk_internal.hpp"

#include <cmath>
#include <vector>

namespace psk {

struct Chebyshev {
    const psk_csr *A = nullptr;   // borrowed
    int32_t degree = 0;
    double lmax = 0.0, lmin = 0.0;
    std::vector<double> coef;     // c0, then (alpha_k, beta_k), k = 1..degree-1
    double *dinv = nullptr, *d = nullptr;
    double *z[2] = {nullptr, nullptr};   // z[0]: degree >= 2, z[1]: degree >= 3
};

void cheby_free(Chebyshev *ch) {
    if (!ch) return;
    void *ptrs[] = {ch->dinv, ch->d, ch->z[0], ch->z[1]};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete ch;
}

// the step kernel's tiles in chunks of consecutive tiles per XCD, as the CSR SpMV's (spmv_csr.hip, kCsrChunk)
constexpr int64_t kChebyChunk = 128;

__device__ __forceinline__ int32_t ld_stream(const int32_t *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ double ld_stream(const double *p) { return __builtin_nontemporal_load(p); }

// DInv_i = 1 / (sum of row i's col == row entries in stored order) (jacobi_dinv_kernel), g_i = (sum_j |a_ij| in
// stored order) * |DInv_i|; part[block] = max of the block's g_i; *bad = 1 when a diagonal is zero, missing or
// not finite. The maximum does not depend on the order it is taken in.
__global__ __launch_bounds__(kBlock) void cheby_setup_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ colidx,
                                                             const double *__restrict__ vals, double *__restrict__ dinv,
                                                             double *__restrict__ part, int32_t *bad) {
    __shared__ double sh[kWaves];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double g = 0.0;
    if (i < n) {
        double d = 0.0, a = 0.0;
        for (int32_t jj = rowptr[i]; jj < rowptr[i + 1]; ++jj) {
            const double v = vals[jj];
            if (colidx[jj] == (int32_t)i) d = d + v;
            a = a + fabs(v);
        }
        const double di = 1.0 / d;   // np.reciprocal
        if (!(d != 0.0) || !isfinite(d)) *bad = 1;
        dinv[i] = di;
        g = a * fabs(di);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) g = fmax(g, __shfl_xor(g, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = g;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = sh[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) r = fmax(r, sh[w]);
        part[blockIdx.x] = r;
    }
}

// out[0] = max of np partials (one workgroup)
__global__ __launch_bounds__(kBlock) void cheby_max_kernel(const double *__restrict__ part, int64_t np, double *out) {
    __shared__ double sh[kWaves];
    double g = 0.0;
    for (int64_t i = threadIdx.x; i < np; i += kBlock) g = fmax(g, part[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) g = fmax(g, __shfl_xor(g, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = g;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = sh[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) r = fmax(r, sh[w]);
        out[0] = r;
    }
}

// step 0: d = c0 (DInv v), z = d
__global__ __launch_bounds__(kBlock) void cheby_first_kernel(int64_t n, double c0, const double *__restrict__ dinv,
                                                             const double *__restrict__ v, double *__restrict__ d,
                                                             double *__restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double t = c0 * (dinv[i] * v[i]);
    d[i] = t;
    z[i] = t;
}

// step k >= 1 for the tile of `trows` rows this workgroup holds:
//   s = sum_j a_ij z_in[j] (rounded products, stored order, from 0.0), res = v_i - s,
//   d_i = alpha d_i + beta (DInv_i res), z_out_i = z_in_i + d_i
// (compiled with -ffp-contract=off: every operation rounds as written). z_out must not alias z_in.
__global__ __launch_bounds__(kBlock) void cheby_step_kernel(
    int64_t n, int trows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
    const double *__restrict__ vals, const double *__restrict__ zin, double *__restrict__ zout,
    const double *__restrict__ v, const double *__restrict__ dinv, double *__restrict__ d, double alpha, double beta,
    int32_t nnz, TileMap tm) {
    constexpr int KU = kChunk / kBlock;   // staged entries per lane per chunk
    __shared__ double prod[kChunk + kBlock];   // + a dump row for lanes past the chunk's end
    const int tid = threadIdx.x;
    const int64_t t = tile_of_block(tm);
    const int64_t r0 = t * trows;
    const int64_t r1 = (r0 + trows < n) ? r0 + trows : n;
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
    const double vi = v[rowc], di = dinv[rowc], dd = d[rowc], zi = zin[rowc];
    double sum = 0.0;
    {   // chunk 0
        const int32_t c0 = e0, c1 = (e1 - c0 > kChunk) ? c0 + kChunk : e1;
        double pv[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) pv[k] = vv[k] * zin[cc[k]];   // rounded product
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
            pv[k] = ld_stream(vals + ee) * zin[ld_stream(colidx + ee)];
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
    const double dn = alpha * dd + beta * (di * res);
    const double zn = zi + dn;
    if (has) {   // the stores last
        d[row] = dn;
        zout[row] = zn;
    }
}

int cheby_apply(const psk_prec *M, const double *v, double *out, hipStream_t s) {
    const Chebyshev *ch = M->cheb;
    const psk_csr *A = ch->A;
    const int64_t n = M->n;
    if (n == 0) return PSK_OK;
    const dim3 bd(kBlock), gv((unsigned)((n + kBlock - 1) / kBlock));
    const int K = ch->degree;
    double *z = K == 1 ? out : ch->z[0];
    hipLaunchKernelGGL(cheby_first_kernel, gv, bd, 0, s, n, ch->coef[0], ch->dinv, v, ch->d, z);
    PSK_HIP(hipGetLastError());
    const int tr = A->tile_rows;
    const int64_t nt = (n + tr - 1) / tr;
    const TileMap tm = tile_map_chunked(nt, kChebyChunk);
    for (int k = 1; k < K; ++k) {
        double *zo = k == K - 1 ? out : ch->z[k & 1];
        hipLaunchKernelGGL(cheby_step_kernel, dim3((unsigned)nt), bd, 0, s, n, tr, A->rowptr, A->colidx, A->vals, z, zo,
                           v, ch->dinv, ch->d, ch->coef[2 * k - 1], ch->coef[2 * k], (int32_t)A->nnz, tm);
        PSK_HIP(hipGetLastError());
        z = zo;
    }
    return PSK_OK;
}

// ---- measurement (libpsk_lab's psk_lab_cheby_ab, tools/cheby_ab.py): one step as the fused launch against the same
// step composed of the launches the library had before it — the residual SpMV in A's own layout (kSpmvResid), the
// DInv scale, the d update and the z update. Same values up to the in-place z.
__global__ void cheby_ab_scale_kernel(int64_t n, const double *__restrict__ d, const double *__restrict__ v,
                                      double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = d[i] * v[i];
}
__global__ void cheby_ab_axpby_kernel(int64_t n, double alpha, double beta, const double *__restrict__ x,
                                      double *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = alpha * y[i] + beta * x[i];
}
__global__ void cheby_ab_add_kernel(int64_t n, const double *__restrict__ x, double *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = y[i] + x[i];
}

int cheby_ab(const psk_prec *M, const double *v, int reps, double *fused_ms, double *pieces_ms) {
    if (!M || M->kind != PSK_PREC_CHEBYSHEV || !M->cheb || !v || reps < 1 || !fused_ms || !pieces_ms)
        return fail(PSK_ERR_ARG, "cheby_ab: bad arguments");
    const Chebyshev *ch = M->cheb;
    if (ch->degree < 3) return fail(PSK_ERR_ARG, "cheby_ab: needs a degree >= 3 handle (both z buffers)");
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    const psk_csr *A = ch->A;
    const int64_t n = M->n;
    const dim3 bd(kBlock), gv((unsigned)((n + kBlock - 1) / kBlock));
    const int tr = A->tile_rows;
    const int64_t nt = (n + tr - 1) / tr;
    const TileMap tm = tile_map_chunked(nt, kChebyChunk);
    const double al = ch->coef[1], be = ch->coef[2];
    DevBuf tmp;
    DevBufRelease rel{tmp};
    PSK_TRY(tmp.ensure((size_t)2 * n * sizeof(double)));
    double *r = tmp.as<double>(), *t = r + n;
    hipEvent_t e0, e1;
    PSK_HIP(hipEventCreate(&e0));
    PSK_HIP(hipEventCreate(&e1));
    int rc = PSK_OK;
    float ms = 0.f;
    for (int pass = 0; pass < 2 && rc == PSK_OK; ++pass) {   // 0: fused, 1: pieces; one untimed step first
        hipLaunchKernelGGL(cheby_first_kernel, gv, bd, 0, s, n, ch->coef[0], ch->dinv, v, ch->d, ch->z[0]);
        for (int i = -1; i < reps && rc == PSK_OK; ++i) {
            if (i == 0 && hipEventRecord(e0, s) != hipSuccess) rc = fail(PSK_ERR_HIP, "cheby_ab: event");
            if (pass == 0) {
                double *zi = ch->z[(i + 1) & 1], *zo = ch->z[i & 1];
                hipLaunchKernelGGL(cheby_step_kernel, dim3((unsigned)nt), bd, 0, s, n, tr, A->rowptr, A->colidx, A->vals,
                                   zi, zo, v, ch->dinv, ch->d, al, be, (int32_t)A->nnz, tm);
            } else {
                rc = launch_spmv(A, kSpmvResid, ch->z[0], r, nullptr, v, nullptr, nullptr, s);
                hipLaunchKernelGGL(cheby_ab_scale_kernel, gv, bd, 0, s, n, ch->dinv, r, t);
                hipLaunchKernelGGL(cheby_ab_axpby_kernel, gv, bd, 0, s, n, al, be, t, ch->d);
                hipLaunchKernelGGL(cheby_ab_add_kernel, gv, bd, 0, s, n, ch->d, ch->z[0]);
            }
        }
        if (rc == PSK_OK && (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                             hipEventElapsedTime(&ms, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess))
            rc = fail(PSK_ERR_HIP, "cheby_ab: timing");
        (pass == 0 ? *fused_ms : *pieces_ms) = ms / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

}  // namespace psk

using namespace psk;

extern "C" {

int psk_prec_create_chebyshev(const psk_csr *A, int32_t degree, double lmax, double ratio, psk_prec **out) {
    if (!A || !out) return fail(PSK_ERR_ARG, "psk_prec_create_chebyshev: NULL argument");
    if (degree < 1) return fail(PSK_ERR_ARG, "psk_prec_create_chebyshev: degree must be >= 1");
    if (!(ratio > 1.0) || !std::isfinite(ratio)) return fail(PSK_ERR_ARG, "psk_prec_create_chebyshev: ratio must be > 1");
    if (std::isnan(lmax) || std::isinf(lmax)) return fail(PSK_ERR_ARG, "psk_prec_create_chebyshev: lmax is not finite");
    if (A->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_prec_create_chebyshev: sharded matrices are not supported");
    if (A->n != A->ncols) return fail(PSK_ERR_ARG, "psk_prec_create_chebyshev: the matrix is not square");
    if (A->n < 1) return fail(PSK_ERR_ARG, "psk_prec_create_chebyshev: the matrix has no rows");
    Context *c;
    PSK_TRY(ctx(&c));
    const int64_t n = A->n;
    Chebyshev *ch = new Chebyshev();
    ch->A = A;
    ch->degree = degree;
    struct Guard {   // released on every early return
        Chebyshev *&p;
        ~Guard() { cheby_free(p); }
    } guard{ch};
    const size_t vec = (size_t)n * sizeof(double);
    hipError_t e = hipMalloc(&ch->dinv, vec);
    if (e == hipSuccess) e = hipMalloc(&ch->d, vec);
    if (e == hipSuccess && degree >= 2) e = hipMalloc(&ch->z[0], vec);
    if (e == hipSuccess && degree >= 3) e = hipMalloc(&ch->z[1], vec);
    if (e != hipSuccess) return fail(PSK_ERR_ALLOC, "psk_prec_create_chebyshev: hipMalloc");
    // DInv and the Gershgorin bound: the per-block maxima go to d (nb <= n doubles; d is rewritten by every
    // apply), their maximum to scal[0], the bad-diagonal flag to the word behind it
    const int64_t nb = (n + kBlock - 1) / kBlock;
    DevBuf scal;
    DevBufRelease rel{scal};
    PSK_TRY(scal.ensure(2 * sizeof(double)));
    double *gmax = scal.as<double>();
    int32_t *bad = reinterpret_cast<int32_t *>(gmax + 1);
    PSK_HIP(hipMemsetAsync(scal.p, 0, 2 * sizeof(double), c->stream));
    hipLaunchKernelGGL(cheby_setup_kernel, dim3((unsigned)nb), dim3(kBlock), 0, c->stream, n, A->rowptr, A->colidx,
                       A->vals, ch->dinv, ch->d, bad);
    PSK_HIP(hipGetLastError());
    hipLaunchKernelGGL(cheby_max_kernel, dim3(1), dim3(kBlock), 0, c->stream, ch->d, nb, gmax);
    PSK_HIP(hipGetLastError());
    double hg[2] = {0.0, 0.0};
    PSK_HIP(hipMemcpyAsync(hg, scal.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PSK_HIP(hipStreamSynchronize(c->stream));
    int32_t hbad;
    std::memcpy(&hbad, &hg[1], sizeof(int32_t));
    if (hbad != 0)
        return fail(PSK_ERR_ARG, "psk_prec_create_chebyshev: a row's diagonal entry is zero, missing or not finite");
    ch->lmax = lmax > 0.0 ? lmax : hg[0];
    if (!(ch->lmax > 0.0) || !std::isfinite(ch->lmax))
        return fail(PSK_ERR_ARG, "psk_prec_create_chebyshev: no finite positive spectrum bound");
    // the scalars, in plain double arithmetic (this file is compiled with -ffp-contract=off)
    ch->lmin = ch->lmax / ratio;
    const double theta = (ch->lmax + ch->lmin) / 2.0, delta = (ch->lmax - ch->lmin) / 2.0;
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    ch->coef.assign((size_t)2 * degree - 1, 0.0);
    ch->coef[0] = 1.0 / theta;
    for (int k = 1; k < degree; ++k) {
        const double rk = 1.0 / (2.0 * sigma - rho);
        ch->coef[2 * k - 1] = rk * rho;
        ch->coef[2 * k] = 2.0 * rk / delta;
        rho = rk;
    }
    psk_prec *M = new psk_prec();
    M->kind = PSK_PREC_CHEBYSHEV;
    M->n = n;
    M->cheb = ch;
    ch = nullptr;   // owned by M now
    *out = M;
    return PSK_OK;
}

int psk_prec_chebyshev_info(const psk_prec *M, int32_t *degree, double *lmax, double *lmin, double *coeffs) {
    if (!M || M->kind != PSK_PREC_CHEBYSHEV || !M->cheb)
        return fail(PSK_ERR_ARG, "psk_prec_chebyshev_info: not a Chebyshev preconditioner");
    const Chebyshev *ch = M->cheb;
    if (degree) *degree = ch->degree;
    if (lmax) *lmax = ch->lmax;
    if (lmin) *lmin = ch->lmin;
    if (coeffs)
        for (size_t i = 0; i < ch->coef.size(); ++i) coeffs[i] = ch->coef[i];
    return PSK_OK;
}

}  // extern "C"
