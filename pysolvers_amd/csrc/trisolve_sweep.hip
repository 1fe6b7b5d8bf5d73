// trisolve_sweep.hip — approximate triangular applies by Jacobi sweeps (psk_prec_trisolve_sweeps; Anzt, Chow and
// Dongarra's iterative sparse triangular solves). With T = D + N (off-diagonal entries N, diagonal d; unit: d = 1):
//     x0 = b / d;   x(j) = (b - N x(j-1)) / d,  j = 1..s;   x = x(s)
// Every sweep is one streaming launch over the factor that reads only the previous iterate (ping-pong buffers), so
// there is no dependency chain inside a launch: no sentinel, no scheduling words, no polling, `err` is never
// written, and the kernel boundary is the only synchronisation. The cost is sweeps x bytes instead of levels x
// latency. N is nilpotent (a row at dependency level l is final after l sweeps), so levels - 1 sweeps reproduce the
// exact solve; a fixed s from the fixed start is a fixed linear operator, which is what the Krylov solvers need.
//
// The kernel reads the solve-order CSR copy every TriFactor holds (position k = row order[k], entries
// [rowptr[k], rowptr[k+1]) with natural column indices): G = 1, 4, 16 or 64 lanes per row chosen from the mean
// off-diagonal row length (a 5-point factor has 2 entries per row: a wave per row would idle 62 lanes of a
// bandwidth-bound kernel), lane t taking entries t, t + G, ... of the row in stored order with fma from 0.0, then
// one fixed-order DPP sum over the group. The entry streams (colidx, vals) are read once per sweep and loaded
// non-temporally; the gathers of the previous iterate, the right-hand side and the diagonal go through the caches.
#include "trisolve.hpp"

#include <algorithm>
#include <cstdlib>

namespace psk {

namespace {

constexpr int64_t kSweepMaxGrid = (int64_t)1 << 20;   // workgroups of one launch (then a grid-stride loop)

// x0[i] = rhs[rhs_idx[i]] / diag[i] (diag == nullptr: no division)
__global__ __launch_bounds__(kBlock) void sweep_start_kernel(int64_t n, const double *__restrict__ diag,
                                                             const double *__restrict__ rhs,
                                                             const int32_t *__restrict__ rhs_idx,
                                                             double *__restrict__ x0) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double r = rhs[rhs_idx ? rhs_idx[i] : i];
        if (diag) r = r / diag[i];
        x0[i] = r;
    }
}

// the sum of a group of G lanes (G consecutive lanes, aligned), in a fixed order; valid in the group's first lane
template <int G>
__device__ __forceinline__ double group_total(double v) {
    if (G == 64) return wave_total(v);
    if (G >= 4) {
        v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
        v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
    }
    if (G >= 16) {
        v += dpp_f64<0x124>(v);   // row_ror:4
        v += dpp_f64<0x128>(v);   // row_ror:8
    }
    return v;
}

// one sweep: xout[row] = (rhs[rhs_idx[row]] - sum_e vals[e] xin[colidx[e]]) / diag[row] for every position. xin
// and xout are different buffers: no row reads a value this launch wrote. Every lane stays in the loop (rows past
// the end are clamped and their store dropped), so the DPP steps see whole groups.
template <int G>
__global__ __launch_bounds__(kBlock) void sweep_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                       const int32_t *__restrict__ colidx,
                                                       const double *__restrict__ vals, const double *__restrict__ diag,
                                                       const int32_t *__restrict__ order, const double *__restrict__ rhs,
                                                       const int32_t *__restrict__ rhs_idx,
                                                       const double *__restrict__ xin, double *__restrict__ xout) {
    constexpr int64_t kGroups = kBlock / G;   // rows per workgroup and pass
    const int64_t local = threadIdx.x / G;
    const int t = threadIdx.x % G;
    for (int64_t base = (int64_t)blockIdx.x * kGroups; base < n; base += (int64_t)gridDim.x * kGroups) {
        const bool live = base + local < n;
        const int64_t k = live ? base + local : n - 1;
        const int64_t e0 = rowptr[k], e1 = rowptr[k + 1];   // 64-bit entry offsets
        double acc = 0.0;
        for (int64_t e = e0 + t; e < e1; e += G)   // rows longer than the group: chunks of G
            acc = fma(__builtin_nontemporal_load(vals + e), xin[__builtin_nontemporal_load(colidx + e)], acc);
        const double sum = group_total<G>(acc);
        if (live && t == 0) {
            const int32_t row = order[k];
            double r = rhs[rhs_idx ? rhs_idx[row] : row] - sum;
            if (diag) r = r / diag[row];
            xout[row] = r;
        }
    }
}

template <int G>
int launch_sweep(int64_t n, const TriFactor &T, const double *rhs, const int32_t *rhs_idx, const double *xin,
                 double *xout, hipStream_t s) {
    const int64_t nb = (n + kBlock / G - 1) / (kBlock / G);
    hipLaunchKernelGGL(sweep_kernel<G>, dim3((unsigned)std::min(nb, kSweepMaxGrid)), dim3(kBlock), 0, s, n,
                       (const int32_t *)T.rowptr, (const int32_t *)T.colidx, (const double *)T.vals,
                       (const double *)T.diag, (const int32_t *)T.order, rhs, rhs_idx, xin, xout);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// lanes per row from the factor's mean off-diagonal row length (PSK_TRISWEEP_WIDTH=1|4|16|64, read when the sweep
// count is set, overrides: tests of every width)
int sweep_width(int64_t n, int64_t nnz) {
    if (const char *e = std::getenv("PSK_TRISWEEP_WIDTH")) {
        const int w = std::atoi(e);
        if (w == 1 || w == 4 || w == 16 || w == 64) return w;
    }
    const double mean = n > 0 ? (double)nnz / (double)n : 0.0;
    return mean <= 2.0 ? 1 : mean <= 8.0 ? 4 : mean <= 32.0 ? 16 : 64;
}

}  // namespace

// x = T.sweeps Jacobi sweeps of T x = rhs[rhs_idx] from x0 = rhs / d: 1 + sweeps launches, the iterates in the two
// n-vectors at T.sweep_buf, the last sweep straight into x (which is neither of them)
int launch_sweeps(const Context *, int64_t n, const TriFactor &T, const double *rhs, const int32_t *rhs_idx, double *x,
                  int32_t *, hipStream_t s) {
    if (n == 0) return PSK_OK;
    if (T.sweeps < 1 || !T.sweep_buf) return fail(PSK_ERR_ARG, "triangular sweeps: factor is not in sweep mode");
    double *p[2] = {T.sweep_buf, T.sweep_buf + n};
    const int64_t nb = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(sweep_start_kernel, dim3((unsigned)std::min(nb, kSweepMaxGrid)), dim3(kBlock), 0, s, n,
                       (const double *)T.diag, rhs, rhs_idx, p[0]);
    PSK_HIP(hipGetLastError());
    for (int32_t j = 1; j <= T.sweeps; ++j) {
        const double *xin = p[(j - 1) & 1];
        double *xout = j == T.sweeps ? x : p[j & 1];
        switch (T.sweep_width) {
        case 1: PSK_TRY(launch_sweep<1>(n, T, rhs, rhs_idx, xin, xout, s)); break;
        case 4: PSK_TRY(launch_sweep<4>(n, T, rhs, rhs_idx, xin, xout, s)); break;
        case 16: PSK_TRY(launch_sweep<16>(n, T, rhs, rhs_idx, xin, xout, s)); break;
        default: PSK_TRY(launch_sweep<64>(n, T, rhs, rhs_idx, xin, xout, s)); break;
        }
    }
    return PSK_OK;
}

}  // namespace psk

using namespace psk;

extern "C" int psk_prec_trisolve_sweeps(psk_prec *M, int32_t which, int32_t set, int32_t *sweeps) {
    if (!M || M->kind != PSK_PREC_ILU || (which != 0 && which != 1))
        return fail(PSK_ERR_ARG, "psk_prec_trisolve_sweeps: not a triangular-solve chain / bad factor");
    TriFactor &T = which == 0 ? M->lo : M->up;
    if (!T.present) return fail(PSK_ERR_ARG, "psk_prec_trisolve_sweeps: factor absent");
    if (set < -1 || set > kMaxSweeps) return fail(PSK_ERR_ARG, "psk_prec_trisolve_sweeps: set must be -1 or 0..65536");
    if (set >= 1) {
        if (!M->sweep_work && M->n > 0) {   // two more n-vectors per chain, shared by its factors (they run in turn)
            Context *c;
            PSK_TRY(ctx(&c));
            if (hipMalloc(&M->sweep_work, (size_t)(2 * M->n) * sizeof(double)) != hipSuccess) {
                M->sweep_work = nullptr;
                return fail(PSK_ERR_ALLOC, "psk_prec_trisolve_sweeps: hipMalloc of the sweep vectors failed");
            }
        }
        T.sweep_buf = M->sweep_work;
        T.sweep_width = sweep_width(M->n, T.nnz);
    }
    if (set >= 0) T.sweeps = set;
    if (sweeps) *sweeps = T.sweeps;
    return PSK_OK;
}
