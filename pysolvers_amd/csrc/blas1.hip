// blas1.hip — BLAS-1 for the standalone entry points: psk_dot, psk_nrm2, psk_axpy and their kernels.
#include "psk_internal.hpp"

#include <cmath>

namespace psk {

__global__ __launch_bounds__(kBlock) void dot_partial_kernel(int64_t n, const double *__restrict__ x,
                                                             const double *__restrict__ y,
                                                             double *__restrict__ part) {
    __shared__ double sh[kWaves];
    int64_t t0, t1;
    const int64_t ntiles = (n + kVecTile - 1) / kVecTile;
    block_range(ntiles, t0, t1);
    const int64_t i0 = t0 * kVecTile, i1 = (t1 * kVecTile < n) ? t1 * kVecTile : n;
    double acc = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kBlock) acc = fma(x[i], y[i], acc);
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void reduce_final_kernel(const double *part, int np, double *out,
                                                              int do_sqrt) {
    __shared__ double sh[kWaves];
    const double s = reduce_partials(part, np, 1, sh);
    if (threadIdx.x == 0) out[0] = do_sqrt ? sqrt(s) : s;
}

__global__ void axpy_kernel(int64_t n, double alpha, const double *__restrict__ x, double *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = y[i] + alpha * x[i];   // compiled with -ffp-contract=off: two roundings
}

}  // namespace psk

using namespace psk;

extern "C" {

static int dot_impl(int64_t n, const double *x, const double *y, int32_t loc, double *out, bool nrm) {
    if (!out || n < 0 || !x || (!nrm && !y)) return fail(PSK_ERR_ARG, "psk_dot: bad arguments");
    Context *c;
    PSK_TRY(ctx(&c));
    DevBuf tmp;
    const int grid = grid_for_rows(c, n, kVecTile);
    PSK_TRY(tmp.ensure((size_t)(2 * n + kMaxGrid + 1) * sizeof(double)));
    double *dx = const_cast<double *>(x), *dy = const_cast<double *>(y);
    double *base = tmp.as<double>();
    if (loc == PSK_HOST) {
        dx = base;
        PSK_TRY(to_device_vec(x, loc, n, dx, c->stream));
        if (!nrm) {
            dy = base + n;
            PSK_TRY(to_device_vec(y, loc, n, dy, c->stream));
        }
    }
    if (nrm) dy = dx;
    double *part = base + 2 * n;
    double *res = part + kMaxGrid;
    hipLaunchKernelGGL(dot_partial_kernel, dim3(grid), dim3(kBlock), 0, c->stream, n, dx, dy, part);
    PSK_HIP(hipGetLastError());
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kBlock), 0, c->stream, part, grid, res, nrm ? 1 : 0);
    PSK_HIP(hipGetLastError());
    PSK_HIP(hipMemcpyAsync(out, res, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PSK_HIP(hipStreamSynchronize(c->stream));
    tmp.release();
    return PSK_OK;
}

int psk_dot(int64_t n, const double *x, const double *y, int32_t loc, double *out) {
    return dot_impl(n, x, y, loc, out, false);
}

int psk_nrm2(int64_t n, const double *x, int32_t loc, double *out) {
    return dot_impl(n, x, nullptr, loc, out, true);
}

int psk_axpy(int64_t n, double alpha, const double *x, double *y, int32_t loc) {
    if (n < 0 || !x || !y) return fail(PSK_ERR_ARG, "psk_axpy: bad arguments");
    if (n == 0) return PSK_OK;
    Context *c;
    PSK_TRY(ctx(&c));
    DevBuf tmp;
    const double *dx = x;
    double *dy = y;
    if (loc == PSK_HOST) {
        PSK_TRY(tmp.ensure((size_t)2 * n * sizeof(double)));
        double *b = tmp.as<double>();
        PSK_TRY(to_device_vec(x, loc, n, b, c->stream));
        PSK_TRY(to_device_vec(y, loc, n, b + n, c->stream));
        dx = b;
        dy = b + n;
    }
    hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       c->stream, n, alpha, dx, dy);
    PSK_HIP(hipGetLastError());
    if (loc == PSK_HOST) PSK_TRY(from_device_vec(dy, PSK_HOST, n, y, c->stream));
    PSK_HIP(hipStreamSynchronize(c->stream));
    return PSK_OK;
}

}  // extern "C"
