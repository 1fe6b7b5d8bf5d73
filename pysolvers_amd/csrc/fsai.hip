// fsai.hip — factorized sparse approximate inverse (psk_csr_fsai) and the preconditioner M^-1 v = G^T (G v) built on
// it (psk_prec_create_fsai, PSK_PREC_FSAI). Replaces nothing in the reference, whose preconditioners stronger than a
// smoother are SuperLU's incomplete factors: for an SPD A = L L^T this builds a sparse lower-triangular G ~ L^-1 on a
// prescribed pattern from n INDEPENDENT small dense problems, and applies it as two SpMVs: no dependency chain, no
// level schedule, no spin wait and no grid sum, at setup or at apply.
//
// The factor, to the bit (include/psk.h states the same). s = the sign of row 0's stored diagonal entry of A; the
// factorisation runs on s A. Row i: J = the pattern row's columns <= i in ascending order, m = |J| <= PSK_FSAI_ROW_CAP,
// i in J. With every operation rounded once and a product rounded before its add or subtract (the library is built
// with -ffp-contract=off):
//   B[a][b] = s * (A[J[a]][J[b]], or 0.0 when it is not stored)                      0 <= b <= a < m
//   b = 0..m-1, a = b..m-1:  t = B[a][b];  t = t - C[a][k] * C[b][k], k = 0..b-1 ascending;
//                            a == b: t must be > 0 and finite, C[b][b] = sqrt(t);  else C[a][b] = t / C[b][b]
//   g[m-1] = 1 / C[m-1][m-1];  a = m-2..0:  u = 0.0;  u = u + C[b][a] * g[b], b = a+1..m-1 ascending;
//                                           g[a] = (-u) / C[a][a]
//   row i of G = (J, g)
// Every value's update sequence is fixed, so the result does not depend on the launch geometry or on which of the
// two numeric kernels handled the row.
//
// Kernels (gfx950, wave64; no floating-point atomics, no wait of a wave or workgroup on another):
//  * fsai_sort_kernel: ONE WAVE PER ROW ranks a row's entries by column into a working copy (as ilu0.hip's) and
//    flags a duplicate column and a column outside [0, n). Run on A (columns and values) and, when the caller gives
//    one, on the pattern (columns only).
//  * fsai_count_kernel: one lane per row: m_i by a binary search of i in the sorted pattern row; the smallest row
//    without its diagonal, the smallest row over the cap and the largest m into device words by integer atomics.
//    The counts are scanned into G's row pointers (spgemm.hip's exclusive scan).
//  * fsai_wave_kernel, the general kernel: ONE WAVE PER ROW. J is staged in LDS; lane a gathers row a of B by
//    walking the lower part of A's sorted row J[a] and looking each column up in J (binary search in LDS, at most 6
//    steps); the factor overwrites B in a packed lower triangle stored COLUMN-major (element (a, k) at
//    off(k) + a - k), so that in column b the lanes a = b..m-1 read consecutive LDS words for C[a][k] and one
//    broadcast word for C[b][k]: each lane runs its own ascending-k chain. The pivot goes round by a register
//    shuffle. The back substitution keeps g[a] in lane a: step a forms the products C[b][a] g[b] in parallel, puts
//    them in LDS and every lane adds them in ascending b (the chain of adds is the definition's; it cannot be a
//    tree). LDS per wave: m_max (m_max + 1) / 2 + 96 doubles, sized from the matrix's longest row at launch: 17 KiB at
//    the cap (then one wave per workgroup), 2.6 KiB at m_max = 21 (four). Every loop is bounded by m <= 64 or by the
//    length of one row of A.
//  * fsai_small_kernel, for matrices whose longest J is <= 4 (the 5- and 7-point stencils on their own pattern, where
//    a wave per row would idle 60 lanes over 10^7 rows): ONE LANE PER ROW, B, C and g in registers, every loop
//    unrolled to 4 and guarded by m, the same operations in the same order. PSK_FSAI_WAVE_ONLY bypasses it.
//  * a failed pivot: the smallest such row into one device word by an integer atomic min (as ilu0.hip); the row
//    finishes with NaNs, which are harmless, and the host reads the word once after the launch.
//
// The apply is two launches of the library's SpMV (launch_spmv, plain mode) on the apply's stream, t = G v then
// out = Gt t with Gt = s G^T stored explicitly: the bits of two psk_spmv calls in whatever layout the two matrices
// took. Bytes per apply: the two matrix streams (12 B per entry + 4 B per row each in CSR, less in a sliced
// layout) plus v, t (written, then gathered) and out.
#include "psk_internal.hpp"

#include <climits>
#include <cmath>

namespace psk {

struct Fsai {
    psk_csr *G = nullptr, *Gt = nullptr;   // owned
    double *t = nullptr;                   // n: G v
    int32_t sign = 0, max_row = 0;
};

void fsai_free(Fsai *f) {
    if (!f) return;
    if (f->G) (void)psk_csr_destroy(f->G);
    if (f->Gt) (void)psk_csr_destroy(f->Gt);
    if (f->t) (void)hipFree(f->t);
    delete f;
}

int64_t fsai_nnz(const Fsai *f) { return f && f->G ? f->G->nnz : 0; }

int fsai_apply(const psk_prec *M, const double *v, double *out, hipStream_t s) {
    const Fsai *f = M->fsai;
    if (M->n == 0) return PSK_OK;
    PSK_TRY(launch_spmv(f->G, kSpmvPlain, v, f->t, nullptr, nullptr, nullptr, nullptr, s));
    return launch_spmv(f->Gt, kSpmvPlain, f->t, out, nullptr, nullptr, nullptr, nullptr, s);
}

namespace {

constexpr int kCap = PSK_FSAI_ROW_CAP;
constexpr int kSmall = 4;   // longest J the one-lane-per-row kernel takes
constexpr int32_t kFlagDup = 1, kFlagRange = 2;
// device words of one call
constexpr int kWordFlags = 0, kWordOverCap = 1, kWordBadPivot = 2, kWordMaxRow = 3, kWordNoDiag = 4, kWords = 5;
// LDS of one wave of the general kernel besides the triangle: 64 products, then J (64 int32 = 32 doubles)
constexpr int kWaveExtra = 64 + 32;
constexpr size_t kWaveLdsBudget = 32768;   // per workgroup: the waves per workgroup are cut to stay under it

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
            return fail(PSK_ERR_ALLOC, "fsai: hipMalloc of a temporary failed");
        p.push_back(q);
        *out = static_cast<T *>(q);
        return PSK_OK;
    }
};

// HIP refuses a grid dimension of 2^32 threads or more: workgroups beyond 2^20 go to a second dimension
constexpr int64_t kGridX = (int64_t)1 << 20;
dim3 grid_for_blocks(int64_t nb) {
    return nb <= kGridX ? dim3((unsigned)(nb > 0 ? nb : 1)) : dim3((unsigned)kGridX, (unsigned)((nb + kGridX - 1) / kGridX));
}
__device__ __forceinline__ int64_t block_index() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

// the lanes of one wave hand values to each other through LDS: its LDS accesses before this are done, and seen, before
// those after it
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// VALS: the values travel with the columns (A); otherwise the structure alone (the pattern)
template <bool VALS>
__global__ __launch_bounds__(kBlock) void fsai_sort_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ col,
                                                           const double *__restrict__ val, int32_t *__restrict__ fcol,
                                                           double *__restrict__ fval, int32_t *words) {
    const int lane = threadIdx.x & 63;
    const int64_t i = block_index() * kWaves + (threadIdx.x >> 6);
    if (i >= n) return;   // wave-uniform
    const int32_t s0 = rowptr[i], L = rowptr[i + 1] - s0;
    int32_t bad = 0;
    for (int32_t q = lane; q < L; q += 64) {
        const int32_t c = col[s0 + q];
        if (c < 0 || c >= n) {
            bad |= kFlagRange;
            continue;
        }
        int32_t rank = 0;
        for (int32_t r = 0; r < L; ++r) {
            const int32_t cr = col[s0 + r];
            rank += cr < c ? 1 : 0;
            if (cr == c && r != q) bad |= kFlagDup;
        }
        // rank < L: at most L - 1 other entries are smaller (with a duplicate two entries share a slot; flagged)
        fcol[s0 + rank] = c;
        if (VALS) fval[s0 + rank] = val[s0 + q];
    }
    if (bad) atomicOr(words + kWordFlags, bad);
}

// m_i = the sorted pattern row's entries with column <= i (they come first)
__global__ __launch_bounds__(kBlock) void fsai_count_kernel(int64_t n, const int32_t *__restrict__ prp,
                                                            const int32_t *__restrict__ pcol,
                                                            int32_t *__restrict__ counts, int32_t *words) {
    const int64_t i = block_index() * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t p0 = prp[i], p1 = prp[i + 1];
    int32_t lo = p0, hi = p1;   // first entry with column > i
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (pcol[mid] <= (int32_t)i) lo = mid + 1;
        else hi = mid;
    }
    const int32_t m = lo - p0;
    counts[i] = m;
    if (m == 0 || pcol[lo - 1] != (int32_t)i) atomicMin(words + kWordNoDiag, (int32_t)i);
    if (m > kCap) atomicMin(words + kWordOverCap, (int32_t)i);
    atomicMax(words + kWordMaxRow, m);
}

// The general kernel: one wave per row, blockDim.x / 64 rows per workgroup. tri = m_max (m_max + 1) / 2.
__global__ __launch_bounds__(kBlock) void fsai_wave_kernel(int64_t n, const int32_t *__restrict__ arp,
                                                           const int32_t *__restrict__ acol,
                                                           const double *__restrict__ aval,
                                                           const int32_t *__restrict__ prp,
                                                           const int32_t *__restrict__ pcol,
                                                           const int32_t *__restrict__ grp, int32_t *__restrict__ gcol,
                                                           double *__restrict__ gval, double sd, int32_t tri,
                                                           int32_t *words) {
    extern __shared__ double fsai_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = block_index() * (blockDim.x >> 6) + wave;
    if (i >= n) return;   // wave-uniform; no workgroup barrier below
    double *C = fsai_lds + (size_t)wave * (size_t)(tri + kWaveExtra);
    double *pw = C + tri;
    int32_t *Js = reinterpret_cast<int32_t *>(pw + 64);
    const int32_t g0 = grp[i];
    int32_t m = grp[i + 1] - g0;
    if (m > kCap) m = kCap;   // never (the host refused the matrix): keeps every index below inside the wave's LDS
    if (m * (m + 1) / 2 > tri) return;   // never: tri was sized from the longest row
    const int32_t p0 = prp[i];
    int32_t myJ = 0;
    if (lane < m) {
        myJ = pcol[p0 + lane];
        Js[lane] = myJ;
        gcol[g0 + lane] = myJ;
    }
    wave_lds_sync();
    // element (a, k), k <= a, of the packed column-major triangle: off(k) + a - k, off(k) = k m - k (k - 1) / 2
    if (lane < m) {   // lane a gathers row a of B
        const int a = lane;
        const double zero = sd * 0.0;
        for (int b = 0, off = 0; b <= a; off += m - b, ++b) C[off + a - b] = zero;
        const int32_t e1 = arp[myJ + 1];
        for (int32_t e = arp[myJ]; e < e1; ++e) {   // the lower part of A's sorted row J[a]
            const int32_t c = acol[e];
            if (c > myJ) break;
            int lo = 0, hi = a + 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (Js[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo <= a && Js[lo] == c) C[lo * m - ((lo * (lo - 1)) >> 1) + a - lo] = sd * aval[e];
        }
    }
    wave_lds_sync();
    bool failed = false;
    for (int b = 0, offb = 0; b < m; offb += m - b, ++b) {
        double t = 0.0;
        if (lane >= b && lane < m) {
            t = C[offb + lane - b];
            for (int k = 0, off = 0; k < b; off += m - k, ++k) t = t - C[off + lane - k] * C[off + b - k];
        }
        const double piv = __shfl(t, b, 64);
        if (!(piv > 0.0) || !__builtin_isfinite(piv)) failed = true;
        const double d = sqrt(piv);
        if (lane == b) C[offb] = d;
        else if (lane > b && lane < m) C[offb + lane - b] = t / d;
        wave_lds_sync();
    }
    // back substitution: g[a] in lane a
    double g = 0.0;
    const double cdiag = lane < m ? C[lane * m - ((lane * (lane - 1)) >> 1)] : 1.0;
    if (lane == m - 1) g = 1.0 / cdiag;
    for (int a = m - 2; a >= 0; --a) {
        const int offa = a * m - ((a * (a - 1)) >> 1);
        if (lane > a && lane < m) pw[lane] = C[offa + lane - a] * g;
        wave_lds_sync();
        double u = 0.0;
        for (int b = a + 1; b < m; ++b) u = u + pw[b];
        if (lane == a) g = (-u) / cdiag;
        wave_lds_sync();   // pw is rewritten by the next step
    }
    if (lane < m) gval[g0 + lane] = g;
    if (failed && lane == 0) atomicMin(words + kWordBadPivot, (int32_t)i);
}

// The small-row kernel: one lane per row, m <= kSmall for every row of the matrix.
__global__ __launch_bounds__(kBlock) void fsai_small_kernel(int64_t n, const int32_t *__restrict__ arp,
                                                            const int32_t *__restrict__ acol,
                                                            const double *__restrict__ aval,
                                                            const int32_t *__restrict__ prp,
                                                            const int32_t *__restrict__ pcol,
                                                            const int32_t *__restrict__ grp, int32_t *__restrict__ gcol,
                                                            double *__restrict__ gval, double sd, int32_t *words) {
    const int64_t i = block_index() * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t g0 = grp[i], p0 = prp[i];
    int32_t m = grp[i + 1] - g0;
    if (m > kSmall) m = kSmall;   // never (the host launches this kernel only when the longest row fits)
    int32_t J[kSmall];
#pragma unroll
    for (int a = 0; a < kSmall; ++a) J[a] = a < m ? pcol[p0 + a] : -1;
    double C[kSmall][kSmall];
    const double zero = sd * 0.0;
#pragma unroll
    for (int a = 0; a < kSmall; ++a) {
#pragma unroll
        for (int b = 0; b < kSmall; ++b) C[a][b] = zero;
        if (a < m) {
            const int32_t r = J[a], e1 = arp[r + 1];
            for (int32_t e = arp[r]; e < e1; ++e) {   // the lower part of A's sorted row J[a]
                const int32_t c = acol[e];
                if (c > r) break;
                const double x = sd * aval[e];
#pragma unroll
                for (int b = 0; b <= a; ++b)
                    if (c == J[b]) C[a][b] = x;
            }
        }
    }
    bool failed = false;
#pragma unroll
    for (int b = 0; b < kSmall; ++b) {
#pragma unroll
        for (int a = b; a < kSmall; ++a) {
            if (a < m) {
                double t = C[a][b];
#pragma unroll
                for (int k = 0; k < b; ++k) t = t - C[a][k] * C[b][k];
                if (a == b) {
                    if (!(t > 0.0) || !__builtin_isfinite(t)) failed = true;
                    C[b][b] = sqrt(t);
                } else {
                    C[a][b] = t / C[b][b];
                }
            }
        }
    }
    double g[kSmall] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a = kSmall - 1; a >= 0; --a) {
        if (a == m - 1) {
            g[a] = 1.0 / C[a][a];
        } else if (a < m - 1) {
            double u = 0.0;
#pragma unroll
            for (int b = a + 1; b < kSmall; ++b)
                if (b < m) u = u + C[b][a] * g[b];
            g[a] = (-u) / C[a][a];
        }
    }
#pragma unroll
    for (int a = 0; a < kSmall; ++a)
        if (a < m) {
            gcol[g0 + a] = J[a];
            gval[g0 + a] = g[a];
        }
    if (failed) atomicMin(words + kWordBadPivot, (int32_t)i);
}

__global__ void fsai_negate_kernel(int64_t nnz, const double *__restrict__ in, double *__restrict__ out) {
    const int64_t e = block_index() * kBlock + threadIdx.x;
    if (e < nnz) out[e] = -in[e];
}

// *out and *sign are written only on success
int fsai_factor(const psk_csr *A, const psk_csr *P, int32_t flags, psk_csr **out, int32_t *sign, int32_t *max_row) {
    if (!A || !out || !sign) return fail(PSK_ERR_ARG, "psk_csr_fsai: NULL argument");
    if (flags & ~PSK_FSAI_WAVE_ONLY) return fail(PSK_ERR_ARG, "psk_csr_fsai: unknown flag");
    if (A->comm || (P && P->comm)) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_fsai: sharded matrix");
    if (A->n != A->ncols) return fail(PSK_ERR_ARG, "psk_csr_fsai: A must be square");
    if (A->n == 0 || A->nnz == 0) return fail(PSK_ERR_ARG, "psk_csr_fsai: A is empty");
    if (P && (P->n != A->n || P->ncols != A->n)) return fail(PSK_ERR_ARG, "psk_csr_fsai: the pattern must have A's size");
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    const int64_t n = A->n, nnz = A->nnz, nt = exscan_tiles(n);
    Tmp tmp;
    int32_t *acol, *pcol_own = nullptr, *counts, *words;
    double *aval;
    int64_t *tiles;
    PSK_TRY(tmp.get(nnz, &acol));
    PSK_TRY(tmp.get(nnz, &aval));
    if (P) PSK_TRY(tmp.get(P->nnz, &pcol_own));
    PSK_TRY(tmp.get(n, &counts));
    PSK_TRY(tmp.get(nt + 1, &tiles));
    PSK_TRY(tmp.get(kWords, &words));
    const int32_t *prp = P ? P->rowptr : A->rowptr;
    const int32_t *pcol = P ? pcol_own : acol;
    psk_csr *G = nullptr;
    int32_t sgn = 0;
    int32_t hw[kWords];
    auto work = [&]() -> int {
        const int32_t init[kWords] = {0, INT32_MAX, INT32_MAX, 0, INT32_MAX};
        PSK_HIP(hipMemcpyAsync(words, init, sizeof(init), hipMemcpyHostToDevice, s));
        const dim3 wave_grid = grid_for_blocks((n + kWaves - 1) / kWaves), lane_grid = grid_for_blocks((n + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(fsai_sort_kernel<true>, wave_grid, dim3(kBlock), 0, s, n, (const int32_t *)A->rowptr,
                           (const int32_t *)A->colidx, (const double *)A->vals, acol, aval, words);
        if (P)
            hipLaunchKernelGGL(fsai_sort_kernel<false>, wave_grid, dim3(kBlock), 0, s, n, (const int32_t *)P->rowptr,
                               (const int32_t *)P->colidx, (const double *)nullptr, pcol_own, (double *)nullptr, words);
        PSK_HIP(hipGetLastError());
        int32_t rp01[2] = {0, 0};
        PSK_HIP(hipMemcpyAsync(hw, words, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipMemcpyAsync(rp01, A->rowptr, sizeof(rp01), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipStreamSynchronize(s));
        if (hw[kWordFlags] & kFlagRange) return fail(PSK_ERR_ARG, "psk_csr_fsai: column index out of range");
        if (hw[kWordFlags] & kFlagDup) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_fsai: duplicate column within a row");
        // the sign: row 0's diagonal entry is the first of its sorted row
        int32_t c0 = -1;
        double d0 = 0.0;
        if (rp01[1] > rp01[0]) {
            PSK_HIP(hipMemcpyAsync(&c0, acol + rp01[0], sizeof(int32_t), hipMemcpyDeviceToHost, s));
            PSK_HIP(hipMemcpyAsync(&d0, aval + rp01[0], sizeof(double), hipMemcpyDeviceToHost, s));
            PSK_HIP(hipStreamSynchronize(s));
        }
        if (c0 != 0 || d0 == 0.0 || !std::isfinite(d0))
            return fail(PSK_ERR_ARG, "psk_csr_fsai: row 0's diagonal entry is zero, missing or not finite");
        sgn = d0 > 0.0 ? 1 : -1;
        // row lengths of G and its row pointers
        hipLaunchKernelGGL(fsai_count_kernel, lane_grid, dim3(kBlock), 0, s, n, prp, pcol, counts, words);
        PSK_HIP(hipGetLastError());
        PSK_HIP(hipMemcpyAsync(hw, words, sizeof(hw), hipMemcpyDeviceToHost, s));
        int64_t total = 0;
        PSK_TRY(exscan_total(n, counts, tiles, nt, s, &total));   // syncs
        if (hw[kWordNoDiag] != INT32_MAX)
            return fail(PSK_ERR_ARG, "psk_csr_fsai: pattern row " + std::to_string(hw[kWordNoDiag]) +
                                         " does not hold its diagonal");
        if (hw[kWordOverCap] != INT32_MAX)
            return fail(PSK_ERR_UNSUPPORTED, "psk_csr_fsai: pattern row " + std::to_string(hw[kWordOverCap]) +
                                                 " has more than " + std::to_string(kCap) + " lower entries");
        const int32_t mmax = hw[kWordMaxRow];
        if (mmax < 1 || mmax > kCap) return fail(PSK_ERR_HIP, "psk_csr_fsai: inconsistent row count");
        PSK_TRY(csr_new_device(n, n, total, &G));
        PSK_TRY(exscan_finish(n, counts, tiles, nt, G->rowptr, s));
        const double sd = (double)sgn;
        if (mmax <= kSmall && !(flags & PSK_FSAI_WAVE_ONLY)) {
            hipLaunchKernelGGL(fsai_small_kernel, lane_grid, dim3(kBlock), 0, s, n, (const int32_t *)A->rowptr,
                               (const int32_t *)acol, (const double *)aval, prp, pcol, (const int32_t *)G->rowptr,
                               G->colidx, G->vals, sd, words);
        } else {
            const int32_t tri = mmax * (mmax + 1) / 2;
            const size_t per = (size_t)(tri + kWaveExtra) * sizeof(double);
            int W = kWaves;
            while (W > 1 && W * per > kWaveLdsBudget) W >>= 1;
            hipLaunchKernelGGL(fsai_wave_kernel, grid_for_blocks((n + W - 1) / W), dim3(64 * W), W * per, s, n,
                               (const int32_t *)A->rowptr, (const int32_t *)acol, (const double *)aval, prp, pcol,
                               (const int32_t *)G->rowptr, G->colidx, G->vals, sd, tri, words);
        }
        PSK_HIP(hipGetLastError());
        PSK_HIP(hipMemcpyAsync(hw, words, sizeof(hw), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipStreamSynchronize(s));
        if (hw[kWordBadPivot] != INT32_MAX)
            return fail(PSK_ERR_ARG, "psk_csr_fsai: not positive definite: the pivot of row " +
                                         std::to_string(hw[kWordBadPivot]) + " is not positive and finite");
        if (max_row) *max_row = mmax;
        return csr_finish_device(G, s);
    };
    const int rc = work();
    if (rc != PSK_OK) {
        (void)hipStreamSynchronize(s);
        csr_discard(G);
        return rc;
    }
    *out = G;
    *sign = sgn;
    return PSK_OK;
}

}  // namespace
}  // namespace psk

using namespace psk;

extern "C" {

int psk_csr_fsai(const psk_csr *A, const psk_csr *pattern, int32_t flags, psk_csr **G, int32_t *sign) {
    return fsai_factor(A, pattern, flags, G, sign, nullptr);
}

int psk_prec_create_fsai(const psk_csr *A, const psk_csr *pattern, int32_t flags, psk_prec **out) {
    if (!out) return fail(PSK_ERR_ARG, "psk_prec_create_fsai: NULL argument");
    Fsai *f = new Fsai();
    struct Guard {   // released on every early return
        Fsai *&p;
        ~Guard() { fsai_free(p); }
    } guard{f};
    PSK_TRY(fsai_factor(A, pattern, flags, &f->G, &f->sign, &f->max_row));
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    const int64_t n = f->G->n, nnz = f->G->nnz;
    if (f->sign > 0) {
        PSK_TRY(psk_csr_transpose(f->G, &f->Gt));
    } else {
        // Gt = (-G)^T: the transpose of a view of G with the values flipped, so that Gt's SpMV layout is built
        // from the flipped values
        DevBuf neg;
        DevBufRelease rel{neg};
        PSK_TRY(neg.ensure((size_t)nnz * sizeof(double)));
        hipLaunchKernelGGL(fsai_negate_kernel, grid_for_blocks((nnz + kBlock - 1) / kBlock), dim3(kBlock), 0, s, nnz,
                           (const double *)f->G->vals, neg.as<double>());
        PSK_HIP(hipGetLastError());
        psk_csr view;
        view.n = n;
        view.ncols = n;
        view.nnz = nnz;
        view.rowptr = f->G->rowptr;
        view.colidx = f->G->colidx;
        view.vals = neg.as<double>();
        const int rc = psk_csr_transpose(&view, &f->Gt);
        (void)hipStreamSynchronize(s);   // before the flipped values are freed
        PSK_TRY(rc);
    }
    if (hipMalloc(&f->t, (size_t)n * sizeof(double)) != hipSuccess)
        return fail(PSK_ERR_ALLOC, "psk_prec_create_fsai: hipMalloc");
    psk_prec *M = new psk_prec();
    M->kind = PSK_PREC_FSAI;
    M->n = n;
    M->fsai = f;
    f = nullptr;   // owned by M now
    *out = M;
    return PSK_OK;
}

int psk_prec_fsai_info(const psk_prec *M, int32_t *sign, int64_t *nnz_g, int32_t *max_row) {
    if (!M || M->kind != PSK_PREC_FSAI || !M->fsai)
        return fail(PSK_ERR_ARG, "psk_prec_fsai_info: not an FSAI preconditioner");
    if (sign) *sign = M->fsai->sign;
    if (nnz_g) *nnz_g = M->fsai->G->nnz;
    if (max_row) *max_row = M->fsai->max_row;
    return PSK_OK;
}

}  // extern "C"
