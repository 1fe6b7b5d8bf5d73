// prec.hip — the preconditioner handle: Jacobi (jacobi_dinv_kernel, scale_kernel), the generic device apply
// every Krylov driver calls (prec_apply_dev, prec_check_error) and the psk_prec_* ABI (create, apply, destroy, info).
#include "amg.hpp"

#include <cstdlib>

namespace psk {

// diagonal (scipy csr_diagonal: sum of col==row entries in stored order) and its reciprocal
__global__ void jacobi_dinv_kernel(int64_t n, const int32_t *rowptr, const int32_t *colidx,
                                   const double *vals, double *dinv) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    for (int32_t jj = rowptr[i]; jj < rowptr[i + 1]; ++jj)
        if (colidx[jj] == (int32_t)i) d = d + vals[jj];
    dinv[i] = 1.0 / d;   // np.reciprocal
}

__global__ void scale_kernel(int64_t n, const double *__restrict__ d, const double *__restrict__ v,
                             double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = d[i] * v[i];
}

int prec_apply_dev(const psk_prec *M, int64_t n, const double *v, double *out, hipStream_t s) {
    if (n == 0) return PSK_OK;
    if (!M || M->kind == PSK_PREC_IDENTITY) {
        PSK_HIP(hipMemcpyAsync(out, v, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
        return PSK_OK;
    }
    if (M->kind == PSK_PREC_JACOBI) {
        hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n,
                           M->dinv, v, out);
        PSK_HIP(hipGetLastError());
        return PSK_OK;
    }
    if (M->kind == PSK_PREC_ILU) return ilu_apply(M, v, out, s);
    if (M->kind == PSK_PREC_AMG) return amg_apply(M, v, out, s);
    if (M->kind == PSK_PREC_DENSE) return dense_apply(M, v, out, s);
    if (M->kind == PSK_PREC_CHEBYSHEV) return cheby_apply(M, v, out, s);
    if (M->kind == PSK_PREC_FSAI) return fsai_apply(M, v, out, s);
    if (M->kind == PSK_PREC_MCGS) return mcgs_apply(M, v, out, s);
    return fail(PSK_ERR_UNSUPPORTED, "unknown preconditioner kind");
}

int prec_check_error(const psk_prec *M, hipStream_t s) {
    if (!M) return PSK_OK;
    if (M->kind == PSK_PREC_ILU) return ilu_check_error(M, s);
    if (M->kind == PSK_PREC_DENSE) return dense_check_error(M, s);
    if (M->kind == PSK_PREC_AMG) {
        const AmgHierarchy *h = M->amg;
        for (psk_prec *S : h->S)
            if (S && S->kind == PSK_PREC_ILU) PSK_TRY(ilu_check_error(S, s));
        if (h->coarse && h->coarse->kind == PSK_PREC_ILU) PSK_TRY(ilu_check_error(h->coarse, s));
        if (h->coarse && h->coarse->kind == PSK_PREC_DENSE) PSK_TRY(dense_check_error(h->coarse, s));
    }
    return PSK_OK;
}

}  // namespace psk

using namespace psk;

extern "C" {

// flag = 1 when some v[i] differs from v[0] bit for bit
__global__ void differs_from_first_kernel(int64_t n, const double *__restrict__ v, int32_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && __double_as_longlong(v[i]) != __double_as_longlong(v[0])) *flag = 1;
}

int psk_prec_create(const psk_csr *A, int32_t kind, psk_prec **out) {
    if (!A || !out) return fail(PSK_ERR_ARG, "psk_prec_create: NULL argument");
    if (kind != PSK_PREC_IDENTITY && kind != PSK_PREC_JACOBI)
        return fail(PSK_ERR_UNSUPPORTED, "psk_prec_create: unknown preconditioner kind");
    Context *c;
    PSK_TRY(ctx(&c));
    psk_prec *M = new psk_prec();
    M->kind = kind;
    M->n = A->n;
    if (kind == PSK_PREC_JACOBI && A->n > 0) {
        hipError_t e = hipMalloc(&M->dinv, (size_t)A->n * sizeof(double));
        if (e != hipSuccess) {
            delete M;
            return fail(PSK_ERR_ALLOC, "hipMalloc dinv");
        }
        hipLaunchKernelGGL(jacobi_dinv_kernel, dim3((unsigned)((A->n + kBlock - 1) / kBlock)), dim3(kBlock),
                           0, c->stream, A->n, A->rowptr, A->colidx, A->vals, M->dinv);
        e = hipGetLastError();
        // a constant diagonal (stencils) gives one DInv value: the PCG kernels then use the scalar
        int32_t *dflag = nullptr;
        if (e == hipSuccess) e = hipMalloc(&dflag, sizeof(int32_t));
        if (e == hipSuccess) e = hipMemsetAsync(dflag, 0, sizeof(int32_t), c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(differs_from_first_kernel, dim3((unsigned)((A->n + kBlock - 1) / kBlock)), dim3(kBlock),
                               0, c->stream, A->n, M->dinv, dflag);
            e = hipGetLastError();
        }
        int32_t differs = 1;
        if (e == hipSuccess) e = hipMemcpyAsync(&differs, dflag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(&M->dinv_value, M->dinv, sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (dflag) (void)hipFree(dflag);
        const char *ue = std::getenv("PSK_JACOBI_UNIFORM");
        M->dinv_uniform = e == hipSuccess && differs == 0 && !(ue && std::atoi(ue) == 0);
        if (e != hipSuccess) {
            (void)hipFree(M->dinv);
            delete M;
            return fail(PSK_ERR_HIP, std::string("jacobi: ") + hipGetErrorString(e));
        }
    }
    *out = M;
    return PSK_OK;
}

int psk_prec_jacobi_uniform(const psk_prec *M, int32_t *uniform, double *value) {
    if (!M || M->kind != PSK_PREC_JACOBI) return fail(PSK_ERR_ARG, "psk_prec_jacobi_uniform: not a Jacobi preconditioner");
    if (uniform) *uniform = M->dinv_uniform ? 1 : 0;
    if (value) *value = M->dinv_uniform ? M->dinv_value : 0.0;
    return PSK_OK;
}

int psk_prec_apply(const psk_prec *M, int64_t n, const double *v, double *outv, int32_t loc) {
    if (!M || !v || !outv || n != M->n) return fail(PSK_ERR_ARG, "psk_prec_apply: bad arguments");
    Context *c;
    PSK_TRY(ctx(&c));
    if (n == 0) return PSK_OK;
    if (M->kind == PSK_PREC_IDENTITY) {
        const hipMemcpyKind k = loc == PSK_HOST ? hipMemcpyHostToHost : hipMemcpyDeviceToDevice;
        if (v != outv) PSK_HIP(hipMemcpyAsync(outv, v, (size_t)n * 8, k, c->stream));
        PSK_HIP(hipStreamSynchronize(c->stream));
        return PSK_OK;
    }
    DevBuf tmp;
    DevBufRelease rel{tmp};
    const double *dv = v;
    double *dout = outv;
    if (loc == PSK_HOST || v == outv) {
        PSK_TRY(tmp.ensure((size_t)2 * n * sizeof(double)));
        double *b = tmp.as<double>();
        PSK_TRY(to_device_vec(v, loc, n, b, c->stream));
        dv = b;
        dout = b + n;
    }
    PSK_TRY(prec_apply_dev(M, n, dv, dout, c->stream));
    if (prec_is_general(M)) PSK_TRY(prec_check_error(M, c->stream));
    if (dout != outv) PSK_TRY(from_device_vec(dout, loc, n, outv, c->stream));
    PSK_HIP(hipStreamSynchronize(c->stream));
    return PSK_OK;
}

int psk_prec_destroy(psk_prec *M) {
    if (!M || lib_shut_down()) return PSK_OK;   // after psk_shutdown: reclaimed with the process
    void *ptrs[] = {M->dinv, M->gather_in, M->gather_out, M->work, M->sweep_work, M->err};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    M->lo.release();
    M->up.release();
    if (M->amg) amg_free(M->amg);
    if (M->dense) dense_free(M->dense);
    if (M->cheb) cheby_free(M->cheb);
    if (M->fsai) fsai_free(M->fsai);
    if (M->mcgs) mcgs_free(M->mcgs);
    delete M;
    return PSK_OK;
}

int psk_prec_info(const psk_prec *M, int32_t *kind, int64_t *n, int64_t *nnz_l, int64_t *nnz_u, int64_t *levels_l,
                  int64_t *levels_u) {
    if (!M) return fail(PSK_ERR_ARG, "psk_prec_info: NULL preconditioner");
    if (kind) *kind = M->kind;
    if (n) *n = M->n;
    // FSAI: both "factors" are G (G and its transpose); multicolour Gauss-Seidel: the grouped copy of A, and its
    // colours as the levels
    const int64_t own = M->fsai ? fsai_nnz(M->fsai) : M->mcgs ? mcgs_nnz(M->mcgs) : -1;
    if (nnz_l) *nnz_l = own >= 0 ? own : M->lo.nnz;
    if (nnz_u) *nnz_u = own >= 0 ? own : M->up.nnz;
    if (levels_l) *levels_l = M->mcgs ? mcgs_ncolors(M->mcgs) : M->lo.levels;
    if (levels_u) *levels_u = M->mcgs ? mcgs_ncolors(M->mcgs) : M->up.levels;
    return PSK_OK;
}

}  // extern "C"
