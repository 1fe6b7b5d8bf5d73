// spgemm.hip — sparse operators built on the device: C = A B (psk_csr_matmat), A^T (psk_csr_transpose) and the
// smoothed-aggregation prolongator (psk_sa_prolongator).
//
// Replaces, bit for bit and in the same stored entry order, the scipy calls of the AMG host setup:
//   psk_csr_matmat      scipy's csr_matmat behind `A * B` / `S.dot(Phat)` (MLHierarchy.py _setUpdate,
//                       SmoothedAggregation.py SmoothProlongator; the reference's MLHierarchy.py:283-292)
//   psk_csr_transpose   I_up.transpose().tocsr() (makeRestrictionOp, MLHierarchy.py:304-322)
//   psk_sa_prolongator  SmoothProlongator's numpy lines and its product (SmoothedAggregation.py:185-205)
// Every SpMV of the library sums a row in stored order, so the entry order of these operators is part of the
// V-cycle's bits; the kernels reproduce scipy's, not merely its values.
//
// csr_matmat's contract, for output row i: enumerate the products t = 0, 1, ... — the entries jj of A's row i in
// stored order and, for each, the entries kk of B's row A.col[jj] in stored order; product t is the rounded
// A.val[jj] * B.val[kk] (no FMA: the library is built with -ffp-contract=off) on column B.col[kk]; a column's
// value is ((0.0 + p_a) + p_b) + ... over its products in ascending t; the columns come out in DESCENDING order of
// their first t (scipy's linked list hands them back last-touched-first) and a column whose sum == 0.0 is dropped.
//
// Kernels (gfx950, wave64; no floating-point atomics, no workgroup waits on another, every loop bounded by a row
// length, a product count or a tile count):
//  * spgemm_row_kernel<CAP, FILL>: ONE WAVE PER OUTPUT ROW. The wave stages the row's products in LDS as
//    (column, value) at index t (an exclusive wave scan of the B row lengths gives each A entry its offset), then
//    lane l owns the products t = l, l + 64, ...: one pass over the staged columns tells it whether its product is
//    the first of its column and, if so, sums that column's later products in ascending t. Ballots of the
//    surviving columns give the row's count (FILL = false) or each survivor's position from the end (FILL = true).
//    Work per row is P^2 / 64 LDS reads per lane for P products (P = 14..150 in SA hierarchies: at most 3 products
//    per lane), which is what a 256-wide LDS sort costs as well, without its barriers. Rows are binned by P: CAP =
//    256 (3 KiB of LDS per wave) takes P <= 256, CAP = 1024 (12 KiB) the rest up to the cap kSpgemmCap = 1024, and
//    is only launched when such a row exists. A row over the cap makes the call return PSK_ERR_UNSUPPORTED.
//    Two passes: count, scan, fill — the count is numeric because of the zero drop.
//    Bytes: each pass reads A's row (12 B/entry) and the B rows it names (12 B per product, served by L2 /
//    Infinity Cache for stencil-like operands); the fill writes 12 B per result entry.
//  * scan_*: exclusive scan of int32 counts into rowptr in three launches (tile sums, one workgroup over the tile
//    sums, tiles again) — no look-back, no spin.
//  * transpose_*: integer column counts (atomic adds on int32: their result does not depend on the order), the
//    scan, a fill that drops every entry's (source entry index, source row) key into some slot of its column's
//    segment, and one wave per output row that ranks the segment's keys: the source entry index is monotone in
//    (source row, stored position), so the ranked order is ascending source row and stored order inside one — the
//    order of scipy's csr_tocsc. Ranking is quadratic in the column length (transfer operators: 5..30).
//  * sa_smooth_kernel: per row d = sum of the stored diagonal entries from 0.0, then per entry s = omega * af,
//    v = s / d, value = col == row ? 1 - v : -v (each rounded once; IEEE division).
#include "psk_internal.hpp"

namespace psk {

constexpr int kSpgemmCap = 1024;    // products of one output row (documented in include/psk.h)
constexpr int kSpgemmSmall = 256;   // rows up to here run in the small bin

struct CsrView {
    int64_t m, ncols;
    const int32_t *rowptr, *colidx;
    const double *vals;
};

// device temporaries of one call, freed on every way out
struct Tmp {
    std::vector<void *> p;
    ~Tmp() {
        for (void *q : p)
            if (q) (void)hipFree(q);
    }
    template <class T> int get(int64_t count, T **out) {
        void *q = nullptr;
        if (hipMalloc(&q, (size_t)(count > 0 ? count : 1) * sizeof(T)) != hipSuccess)
            return fail(PSK_ERR_ALLOC, "spgemm: hipMalloc of a temporary failed");
        p.push_back(q);
        *out = static_cast<T *>(q);
        return PSK_OK;
    }
};

// One wave per row: kWaves rows per workgroup. HIP refuses a grid dimension of 2^32 threads or more (2^24
// workgroups of 256), which 2^26 rows reach, so the workgroups are laid out in two dimensions.
constexpr int64_t kRowGridX = (int64_t)1 << 20;
static dim3 wave_row_grid(int64_t rows) {
    const int64_t nb = (rows + kWaves - 1) / kWaves;
    return nb <= kRowGridX ? dim3((unsigned)(nb > 0 ? nb : 1)) : dim3((unsigned)kRowGridX, (unsigned)((nb + kRowGridX - 1) / kRowGridX));
}
__device__ __forceinline__ int64_t wave_row_index() {
    return ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kWaves + (threadIdx.x >> 6);
}

// flag bits of the count pass
constexpr int32_t kFlagOverCap = 1, kFlagLarge = 2;

template <int CAP, bool FILL>
__global__ __launch_bounds__(kBlock) void spgemm_row_kernel(CsrView A, CsrView B, int32_t *__restrict__ counts,
                                                            const int32_t *__restrict__ crowptr,
                                                            int32_t *__restrict__ ccol, double *__restrict__ cval,
                                                            int32_t *flag) {
    constexpr int K = CAP / 64;
    __shared__ int32_t s_col[kWaves][CAP];
    __shared__ double s_val[kWaves][CAP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = wave_row_index();
    const bool live = i < A.m;   // wave-uniform
    int64_t P = 0;               // products of the row (wave-uniform)
    if (live) {
        const int32_t a0 = A.rowptr[i], a1 = A.rowptr[i + 1];
        for (int32_t base = a0; base < a1; base += 64) {
            const int32_t jj = base + lane;
            int32_t b0 = 0, blen = 0;
            double av = 0.0;
            if (jj < a1) {
                const int32_t j = A.colidx[jj];
                b0 = B.rowptr[j];
                blen = B.rowptr[j + 1] - b0;
                av = A.vals[jj];
            }
            int64_t inc = blen;   // inclusive wave scan (64-bit: 64 row lengths may pass 2^31)
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int64_t up = __shfl_up(inc, o, 64);
                if (lane >= o) inc += up;
            }
            const int64_t off = P + inc - blen;
            if (off + blen <= CAP)   // staged only while the row fits this bin; P decides below
                for (int32_t kk = 0; kk < blen; ++kk) {
                    s_col[wave][off + kk] = B.colidx[b0 + kk];
                    s_val[wave][off + kk] = av * B.vals[b0 + kk];
                }
            P += __shfl(inc, 63, 64);
        }
    }
    __syncthreads();   // the only barrier: every wave reaches it, LDS is read-only afterwards
    if (!live) return;
    const bool mine = CAP == kSpgemmSmall ? P <= kSpgemmSmall : (P > kSpgemmSmall && P <= CAP);
    if (!mine) {
        if (!FILL && CAP == kSpgemmSmall && lane == 0) {
            counts[i] = 0;   // the large bin's count pass overwrites it
            const int32_t bit = P > kSpgemmCap ? kFlagOverCap : kFlagLarge;
            if (!(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(flag, bit);
        }
        return;
    }
    const int np = (int)P;
    int32_t c[K];
    double sum[K];
    bool first[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int t = lane + 64 * k;
        c[k] = t < np ? s_col[wave][t] : -1;   // stored columns are >= 0: -1 never matches
        sum[k] = 0.0;
        first[k] = t < np;
    }
    for (int tp = 0; tp < np; ++tp) {
        const int32_t cc = s_col[wave][tp];   // the same address in every lane: a broadcast read
        const double v = s_val[wave][tp];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (cc == c[k]) {
                if (tp < lane + 64 * k) first[k] = false;
                else sum[k] += v;   // ascending t, from 0.0
            }
        }
    }
    unsigned long long mask[K];
    int total = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        mask[k] = __ballot(first[k] && sum[k] != 0.0);
        total += __popcll(mask[k]);
    }
    if (!FILL) {
        if (lane == 0) counts[i] = total;
        return;
    }
    // descending first t: a survivor's position is the number of survivors with a larger t
    const int64_t out0 = crowptr[i];
    const unsigned long long above = lane == 63 ? 0ull : ~0ull << (lane + 1);
    int after = 0;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
        if ((mask[k] >> lane) & 1ull) {
            const int64_t pos = out0 + after + __popcll(mask[k] & above);
            ccol[pos] = c[k];
            cval[pos] = sum[k];
        }
        after += __popcll(mask[k]);
    }
}

// ---- exclusive scan of int32 counts -----------------------------------------------------------------------------
// every thread; returns the exclusive prefix of v over the workgroup and the workgroup total
__device__ __forceinline__ int64_t block_exscan(int64_t v, int64_t *sh, int64_t &total) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        const int64_t add = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    total = sh[kBlock - 1];
    return sh[t] - v;
}

__global__ __launch_bounds__(kBlock) void scan_tile_sums_kernel(int64_t n, const int32_t *__restrict__ counts,
                                                                int64_t *__restrict__ tile_sums) {
    __shared__ int64_t sh[kBlock];
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + 4 * (int64_t)threadIdx.x;
    int64_t v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (i0 + q < n) v += counts[i0 + q];
    int64_t total;
    (void)block_exscan(v, sh, total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one workgroup: tile_sums[0..nt) -> exclusive prefixes in place, the grand total to tile_sums[nt]
__global__ __launch_bounds__(kBlock) void scan_tiles_kernel(int64_t nt, int64_t *tile_sums) {
    __shared__ int64_t sh[kBlock];
    int64_t carry = 0;
    for (int64_t base = 0; base < nt; base += kBlock) {
        const int64_t q = base + threadIdx.x;
        const int64_t v = q < nt ? tile_sums[q] : 0;
        int64_t total;
        const int64_t ex = block_exscan(v, sh, total);
        if (q < nt) tile_sums[q] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tile_sums[nt] = carry;
}

__global__ __launch_bounds__(kBlock) void scan_finish_kernel(int64_t n, const int32_t *__restrict__ counts,
                                                             const int64_t *__restrict__ tile_sums, int64_t nt,
                                                             int32_t *__restrict__ rowptr) {
    __shared__ int64_t sh[kBlock];
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + 4 * (int64_t)threadIdx.x;
    int32_t cnt[4];
    int64_t v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        cnt[q] = i0 + q < n ? counts[i0 + q] : 0;
        v += cnt[q];
    }
    int64_t total;
    int64_t run = tile_sums[blockIdx.x] + block_exscan(v, sh, total);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (i0 + q < n) rowptr[i0 + q] = (int32_t)run;
        run += cnt[q];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) rowptr[n] = (int32_t)tile_sums[nt];
}

// counts[n] -> *total (host), leaving the tile prefixes in `tiles` for exscan_finish
// (declared in psk_internal.hpp: fsai.hip sizes its result the same way)
int exscan_total(int64_t n, const int32_t *counts, int64_t *tiles, int64_t nt, hipStream_t s, int64_t *total) {
    if (nt > 0)
        hipLaunchKernelGGL(scan_tile_sums_kernel, dim3((unsigned)nt), dim3(kBlock), 0, s, n, counts, tiles);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kBlock), 0, s, nt, tiles);
    PSK_HIP(hipGetLastError());
    PSK_HIP(hipMemcpyAsync(total, tiles + nt, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    return PSK_OK;
}
int exscan_finish(int64_t n, const int32_t *counts, const int64_t *tiles, int64_t nt, int32_t *rowptr,
                       hipStream_t s) {
    if (nt > 0) {
        hipLaunchKernelGGL(scan_finish_kernel, dim3((unsigned)nt), dim3(kBlock), 0, s, n, counts, tiles, nt, rowptr);
        PSK_HIP(hipGetLastError());
    } else {
        PSK_HIP(hipMemsetAsync(rowptr, 0, sizeof(int32_t), s));
    }
    return PSK_OK;
}

// C = A B for device views; *out is written only on success
static int matmat_views(const CsrView &A, const CsrView &B, psk_csr **out) {
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    const int64_t m = A.m, nt = (m + kScanTile - 1) / kScanTile;
    if (m >= INT32_MAX || B.ncols >= INT32_MAX || nt > INT32_MAX)
        return fail(PSK_ERR_UNSUPPORTED, "psk_csr_matmat: int32 CSR indices required");
    Tmp tmp;
    int32_t *counts, *flag;
    int64_t *tiles;
    PSK_TRY(tmp.get(m, &counts));
    PSK_TRY(tmp.get(1, &flag));
    PSK_TRY(tmp.get(nt + 1, &tiles));
    PSK_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    const dim3 grid = wave_row_grid(m);
    int32_t hflag = 0;
    if (m > 0) {
        hipLaunchKernelGGL((spgemm_row_kernel<kSpgemmSmall, false>), grid, dim3(kBlock), 0, s, A, B, counts,
                           (const int32_t *)nullptr, (int32_t *)nullptr, (double *)nullptr, flag);
        PSK_HIP(hipGetLastError());
        PSK_HIP(hipMemcpyAsync(&hflag, flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipStreamSynchronize(s));
        if (hflag & kFlagOverCap)
            return fail(PSK_ERR_UNSUPPORTED, "psk_csr_matmat: a row has more than 1024 products");
        if (hflag & kFlagLarge) {
            hipLaunchKernelGGL((spgemm_row_kernel<kSpgemmCap, false>), grid, dim3(kBlock), 0, s, A, B, counts,
                               (const int32_t *)nullptr, (int32_t *)nullptr, (double *)nullptr, flag);
            PSK_HIP(hipGetLastError());
        }
    }
    int64_t nnz = 0;
    PSK_TRY(exscan_total(m, counts, tiles, nt, s, &nnz));
    if (nnz > kMaxNnz) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_matmat: the result exceeds the int32 nnz limit");
    psk_csr *C = nullptr;
    PSK_TRY(csr_new_device(m, B.ncols, nnz, &C));
    int rc = exscan_finish(m, counts, tiles, nt, C->rowptr, s);
    if (rc == PSK_OK && m > 0) {
        hipLaunchKernelGGL((spgemm_row_kernel<kSpgemmSmall, true>), grid, dim3(kBlock), 0, s, A, B,
                           (int32_t *)nullptr, (const int32_t *)C->rowptr, C->colidx, C->vals, flag);
        if (hflag & kFlagLarge)
            hipLaunchKernelGGL((spgemm_row_kernel<kSpgemmCap, true>), grid, dim3(kBlock), 0, s, A, B,
                               (int32_t *)nullptr, (const int32_t *)C->rowptr, C->colidx, C->vals, flag);
        if (hipGetLastError() != hipSuccess) rc = fail(PSK_ERR_HIP, "psk_csr_matmat: launch failed");
    }
    if (rc == PSK_OK) rc = csr_finish_device(C, s);
    if (rc != PSK_OK) {
        (void)hipStreamSynchronize(s);
        csr_discard(C);
        return rc;
    }
    *out = C;
    return PSK_OK;
}

// ---- transpose --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void transpose_count_kernel(int64_t nnz, const int32_t *__restrict__ colidx,
                                                                 int32_t *cnt) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < nnz) atomicAdd(cnt + colidx[e], 1);
}

// every entry into SOME slot of its column's segment (the ranking kernel orders them): cnt counts down to zero
__global__ __launch_bounds__(kBlock) void transpose_scatter_kernel(int64_t m, const int32_t *__restrict__ rowptr,
                                                                   const int32_t *__restrict__ colidx,
                                                                   const int32_t *__restrict__ trowptr, int32_t *cnt,
                                                                   uint64_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int32_t e1 = rowptr[i + 1];
    for (int32_t e = rowptr[i]; e < e1; ++e) {
        const int32_t j = colidx[e];
        const int32_t slot = atomicSub(cnt + j, 1) - 1;
        keys[(int64_t)trowptr[j] + slot] = ((uint64_t)(uint32_t)e << 32) | (uint32_t)i;
    }
}

// one wave per output row: rank its keys (distinct), write (source row, value) at the rank
__global__ __launch_bounds__(kBlock) void transpose_rank_kernel(int64_t nrows, const int32_t *__restrict__ trowptr,
                                                                const uint64_t *__restrict__ keys,
                                                                const double *__restrict__ vals,
                                                                int32_t *__restrict__ tcol, double *__restrict__ tval) {
    const int lane = threadIdx.x & 63;
    const int64_t j = wave_row_index();
    if (j >= nrows) return;
    const int64_t s0 = trowptr[j];
    const int32_t L = trowptr[j + 1] - trowptr[j];
    for (int32_t q = lane; q < L; q += 64) {
        const uint64_t key = keys[s0 + q];
        int32_t rank = 0;
        for (int32_t r = 0; r < L; ++r) rank += keys[s0 + r] < key ? 1 : 0;
        tcol[s0 + rank] = (int32_t)(uint32_t)key;
        tval[s0 + rank] = vals[key >> 32];
    }
}

// ---- prolongator smoothing ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sa_smooth_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ colidx,
                                                           const double *__restrict__ vals,
                                                           const double *__restrict__ af, double omega,
                                                           double *__restrict__ sv) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t e0 = rowptr[i], e1 = rowptr[i + 1];
    double d = 0.0;   // scipy's diagonal(): the row's col == row entries in stored order
    for (int32_t e = e0; e < e1; ++e)
        if (colidx[e] == i) d += vals[e];
    for (int32_t e = e0; e < e1; ++e) {
        const double sc = omega * af[e];
        const double v = sc / d;
        sv[e] = colidx[e] == i ? 1.0 - v : -v;
    }
}

__global__ __launch_bounds__(kBlock) void sa_phat_kernel(int64_t n, int32_t *__restrict__ rowptr,
                                                         double *__restrict__ ones) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i <= n) rowptr[i] = (int32_t)i;
    if (i < n) ones[i] = 1.0;
}

}  // namespace psk

using namespace psk;

static CsrView view_of(const psk_csr *A) { return CsrView{A->n, A->ncols, A->rowptr, A->colidx, A->vals}; }

extern "C" {

int psk_csr_matmat(const psk_csr *A, const psk_csr *B, psk_csr **C) {
    if (!A || !B || !C) return fail(PSK_ERR_ARG, "psk_csr_matmat: NULL argument");
    if (A->comm || B->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_matmat: sharded operand");
    if (A->ncols != B->n) return fail(PSK_ERR_ARG, "psk_csr_matmat: inner dimensions differ");
    return matmat_views(view_of(A), view_of(B), C);
}

int psk_csr_transpose(const psk_csr *A, psk_csr **At) {
    if (!A || !At) return fail(PSK_ERR_ARG, "psk_csr_transpose: NULL argument");
    if (A->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_transpose: sharded operand");
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    const int64_t m = A->n, nr = A->ncols, nnz = A->nnz, nt = (nr + kScanTile - 1) / kScanTile;
    Tmp tmp;
    int32_t *cnt;
    int64_t *tiles;
    uint64_t *keys;
    PSK_TRY(tmp.get(nr, &cnt));
    PSK_TRY(tmp.get(nt + 1, &tiles));
    PSK_TRY(tmp.get(nnz, &keys));
    psk_csr *T = nullptr;
    PSK_TRY(csr_new_device(nr, m, nnz, &T));
    auto work = [&]() -> int {
        if (nr > 0) PSK_HIP(hipMemsetAsync(cnt, 0, (size_t)nr * sizeof(int32_t), s));
        if (nnz > 0)
            hipLaunchKernelGGL(transpose_count_kernel, dim3((unsigned)((nnz + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                               nnz, (const int32_t *)A->colidx, cnt);
        PSK_HIP(hipGetLastError());
        int64_t total = 0;
        PSK_TRY(exscan_total(nr, cnt, tiles, nt, s, &total));
        PSK_TRY(exscan_finish(nr, cnt, tiles, nt, T->rowptr, s));
        if (nnz > 0) {
            hipLaunchKernelGGL(transpose_scatter_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                               m, (const int32_t *)A->rowptr, (const int32_t *)A->colidx, (const int32_t *)T->rowptr,
                               cnt, keys);
            hipLaunchKernelGGL(transpose_rank_kernel, wave_row_grid(nr), dim3(kBlock), 0, s,
                               nr, (const int32_t *)T->rowptr, (const uint64_t *)keys, (const double *)A->vals,
                               T->colidx, T->vals);
            PSK_HIP(hipGetLastError());
        }
        return csr_finish_device(T, s);
    };
    const int rc = work();
    if (rc != PSK_OK) {
        (void)hipStreamSynchronize(s);
        csr_discard(T);
        return rc;
    }
    *At = T;
    return PSK_OK;
}

int psk_sa_prolongator(const psk_csr *A, const int32_t *agg, int64_t count, const double *af_vals, double omega,
                       int32_t loc, psk_csr **P) {
    if (!A || !agg || !P || (A->nnz > 0 && !af_vals) || count < 0 || (loc != PSK_HOST && loc != PSK_DEVICE))
        return fail(PSK_ERR_ARG, "psk_sa_prolongator: bad arguments");
    if (A->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_sa_prolongator: sharded operand");
    if (A->n != A->ncols) return fail(PSK_ERR_ARG, "psk_sa_prolongator: A must be square");
    if (count >= INT32_MAX) return fail(PSK_ERR_UNSUPPORTED, "psk_sa_prolongator: int32 CSR indices required");
    const int64_t n = A->n, nnz = A->nnz;
    if (loc == PSK_HOST)
        for (int64_t i = 0; i < n; ++i)
            if (agg[i] < 0 || agg[i] >= count) return fail(PSK_ERR_ARG, "psk_sa_prolongator: aggregate out of range");
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    Tmp tmp;
    const int32_t *dagg = agg;
    const double *daf = af_vals;
    if (loc == PSK_HOST) {
        int32_t *ta;
        double *tf;
        PSK_TRY(tmp.get(n, &ta));
        PSK_TRY(tmp.get(nnz, &tf));
        if (n > 0) PSK_HIP(hipMemcpyAsync(ta, agg, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (nnz > 0) PSK_HIP(hipMemcpyAsync(tf, af_vals, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, s));
        dagg = ta;
        daf = tf;
    }
    double *sv, *ones;
    int32_t *iota;
    PSK_TRY(tmp.get(nnz, &sv));
    PSK_TRY(tmp.get(n, &ones));
    PSK_TRY(tmp.get(n + 1, &iota));
    const unsigned grid = (unsigned)((n + 1 + kBlock - 1) / kBlock);
    if (n > 0)
        hipLaunchKernelGGL(sa_smooth_kernel, dim3(grid), dim3(kBlock), 0, s, n, (const int32_t *)A->rowptr,
                           (const int32_t *)A->colidx, (const double *)A->vals, daf, omega, sv);
    hipLaunchKernelGGL(sa_phat_kernel, dim3(grid), dim3(kBlock), 0, s, n, iota, ones);
    PSK_HIP(hipGetLastError());
    const CsrView S{n, n, A->rowptr, A->colidx, sv};
    const CsrView Phat{n, count, iota, dagg, ones};
    const int rc = matmat_views(S, Phat, P);
    (void)hipStreamSynchronize(s);   // the host buffers and the temporaries are free to go
    return rc;
}

}  // extern "C"
