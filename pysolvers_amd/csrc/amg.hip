// amg.hip — smoothed-aggregation AMG preconditioner apply on the device: the hierarchy, the V-cycle and the
// psk_prec_create_amg ABI. The paired Gauss-Seidel kernel is in amg_gs_pair.hip, the host setup in amg_aggregate.hip.
//
// apply(v) restates AMGPreconditioner.apply (AMGPreconditioner.py:46-51) -> AMGVCycleSolver.solve with
// CommonSolverArgs(maxiter=numIters, failOnMaxiter=False) (VCycleSolver.py:52-95):
//     x = copy(v);  for k < numIters: x = runLevel(v, x, L-1); r = v - A x;  if ||r|| < tau ||v||: return x
// runLevel (VCycleManager.py:31-62): level 0 -> direct solve; else pre-smooth, r = f - A x, f2 = R r,
// x2 = runLevel(f2, 0, lev-1), x = x + P x2, post-smooth. A smoothing sweep is x <- x + S^-1 (f - A x) for both of
// the reference's smoothers (ClassicSmoothers.py:5-36: Jacobi S^-1 = DInv*, Gauss-Seidel S^-1 = spsolve(triu(A), .)).
//
// Everything stays on one stream with no host synchronisation: the early exit is a device flag. After each non-final
// cycle a one-workgroup kernel compares the fused residual norm (SpMV epilogue) with tau ||v|| and, the first time it
// holds, the current x is copied to the output; later cycles still run (their result is discarded), which keeps the
// launch sequence fixed.
#include "amg.hpp"

#include <algorithm>

namespace psk {

void amg_free(AmgHierarchy *h) {
    if (!h) return;
    for (auto &b : h->x) b.release();
    for (auto &b : h->f) b.release();
    for (auto &b : h->r) b.release();
    for (auto &b : h->t) b.release();
    for (auto &g : h->gp) g.pub.release();
    h->scal.release();
    h->loop.release();
    delete h;
}

__global__ void amg_add_kernel(int64_t n, double *__restrict__ x, const double *__restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] + d[i];   // x + dx (ClassicSmoothers.py:14, :34)
}

// ||v||^2 partials, and x = copy(v) (VCycleSolver.py:69) in the same pass
__global__ __launch_bounds__(kBlock) void amg_sqnorm_partial_kernel(int64_t n, const double *__restrict__ v,
                                                                    double *__restrict__ part,
                                                                    double *__restrict__ x) {
    __shared__ double sh[kWaves];
    int64_t t0, t1;
    const int64_t ntiles = (n + kVecTile - 1) / kVecTile;
    block_range(ntiles, t0, t1);
    const int64_t i0 = t0 * kVecTile, i1 = (t1 * kVecTile < n) ? t1 * kVecTile : n;
    double acc = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kBlock) {
        const double vi = v[i];
        x[i] = vi;
        acc = fma(vi, vi, acc);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// scal[0] = sum of np partials (||v||^2); flag = 0
__global__ __launch_bounds__(kBlock) void amg_init_kernel(const double *part, int np, double *scal,
                                                          int64_t *flag) {
    __shared__ double sh[kWaves];
    const double s = reduce_partials(part, np, 1, sh);
    if (threadIdx.x == 0) {
        scal[0] = s;
        *flag = 0;
    }
}

// convergence test after a non-final cycle (VCycleSolver.py:134-142): 0 -> 1 the first time
__global__ __launch_bounds__(kBlock) void amg_check_kernel(const double *part, int np, const double *scal,
                                                           double tau, int64_t *flag) {
    __shared__ double sh[kWaves];
    const double rr = reduce_partials(part, np, 1, sh);
    if (threadIdx.x == 0 && *flag == 0 && sqrt(rr) < tau * sqrt(scal[0])) *flag = 1;
}

// out = x when flag == want (a converged snapshot (1), or the final x when never converged (0))
__global__ void amg_copy_if_kernel(int64_t n, const int64_t *flag, int64_t want, const double *__restrict__ x,
                                   double *__restrict__ out) {
    if (*flag != want) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = x[i];
}

__global__ void amg_promote_kernel(int64_t *flag) {
    if (*flag == 1) *flag = 2;
}

static inline dim3 vgrid(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// nu sweeps of x <- x + S^-1 (f - A x) on level lev
static int amg_smooth(const AmgHierarchy *h, const Context *c, int lev, const double *f, double *x, int nu,
                      hipStream_t s) {
    psk_csr *A = h->A[lev];
    const int64_t n = A->n;
    double *r = h->r[lev].as<double>(), *t = h->t[lev].as<double>();
    int it = 0;
    // two sweeps per launch (gs_pair_kernel), unless the smoother was switched to Jacobi sweeps since the hierarchy
    // was built (psk_prec_trisolve_sweeps): the pair is an exact solve, so it steps aside for ilu_apply_add
    if ((size_t)lev < h->gp.size() && h->gp[lev].on && h->S[lev]->up.sweeps == 0)
        for (; it + 2 <= nu; it += 2) {
            PSK_TRY(launch_spmv(A, kSpmvResid, x, r, nullptr, f, nullptr, nullptr, s));
            PSK_TRY(gs_pair_launch(c, h->gp[lev], h->S[lev], f, r, x, s));
        }
    for (; it < nu; ++it) {
        PSK_TRY(launch_spmv(A, kSpmvResid, x, r, nullptr, f, nullptr, nullptr, s));
        // (round 3: x += U^-1 r fused into the solve's last gather, profiles/r3_amg_fuse_ab.txt)
        if (h->S[lev] && h->S[lev]->kind == PSK_PREC_ILU) {   // Gauss-Seidel: x += U^-1 r in the last gather
            PSK_TRY(ilu_apply_add(h->S[lev], r, x, s));
            continue;
        }
        PSK_TRY(prec_apply_dev(h->S[lev], n, r, t, s));
        hipLaunchKernelGGL(amg_add_kernel, vgrid(n), dim3(kBlock), 0, s, n, x, t);
        PSK_HIP(hipGetLastError());
    }
    return PSK_OK;
}

// x <- runLevel(f, x, lev) (VCycleManager.py:31-62)
static int amg_level(const AmgHierarchy *h, const Context *c, int lev, const double *f, double *x,
                     hipStream_t s) {
    if (lev == 0) return prec_apply_dev(h->coarse, h->A[0]->n, f, x, s);   // spsolve(A_c, f) (:34-37)
    psk_csr *A = h->A[lev];
    PSK_TRY(amg_smooth(h, c, lev, f, x, h->nu_pre, s));                         // :41
    double *r = h->r[lev].as<double>();
    PSK_TRY(launch_spmv(A, kSpmvResid, x, r, nullptr, f, nullptr, nullptr, s));   // :44
    double *f2 = h->f[lev - 1].as<double>(), *x2 = h->x[lev - 1].as<double>();
    psk_csr *R = h->R[lev - 1], *P = h->P[lev - 1];
    PSK_TRY(launch_spmv(R, kSpmvPlain, r, f2, nullptr, nullptr, nullptr, nullptr, s));   // :47
    if (lev - 1 > 0 && h->A[lev - 1]->n > 0)
        PSK_HIP(hipMemsetAsync(x2, 0, (size_t)h->A[lev - 1]->n * sizeof(double), s));   // zeros_like (:50)
    PSK_TRY(amg_level(h, c, lev - 1, f2, x2, s));                                  // :51
    PSK_TRY(launch_spmv(P, kSpmvAdd, x2, x, nullptr, x, nullptr, nullptr, s));   // :54
    return amg_smooth(h, c, lev, f, x, h->nu_post, s);                            // :59
}

// ---- what amg_apply and the standalone solver (vcycle.hip, psk_vcycle) share: the loop's vectors and scalars on the
// finest level, its start, one cycle and the residual with its in-launch sum
int amg_loop_view(const psk_prec *M, AmgLoop *out) {
    if (!M || M->kind != PSK_PREC_AMG || !M->amg) return fail(PSK_ERR_ARG, "amg_loop_view: not an AMG preconditioner");
    AmgHierarchy *h = M->amg;
    const int top = h->L - 1;
    out->A = h->A[top];
    out->x = h->x[top].as<double>();
    out->r = h->r[top].as<double>();
    out->normb2 = h->scal.as<double>();
    out->sum = h->scal.as<double>() + 2;
    out->work = &h->loop;
    return PSK_OK;
}

// scal[0] = ||v||^2, flag = 0, x = copy(v) (VCycleSolver.py:63, :69)
int amg_loop_start(const psk_prec *M, const Context *c, const double *v, hipStream_t s) {
    const AmgHierarchy *h = M->amg;
    const int64_t n = M->n;
    double *x = h->x[h->L - 1].as<double>();
    double *scal = h->scal.as<double>();
    int64_t *flag = reinterpret_cast<int64_t *>(scal + 1);
    double *part = scal + 2;
    const int gv = grid_for_rows(c, n, kVecTile);
    hipLaunchKernelGGL(amg_sqnorm_partial_kernel, dim3(gv), dim3(kBlock), 0, s, n, v, part, x);   // + x = copy(b) (:69)
    PSK_HIP(hipGetLastError());
    hipLaunchKernelGGL(amg_init_kernel, dim3(1), dim3(kBlock), 0, s, part, gv, scal, flag);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// x = runCycle(v, x) on the finest level's x (VCycleSolver.py:81)
int amg_cycle(const psk_prec *M, const Context *c, const double *v, hipStream_t s) {
    const AmgHierarchy *h = M->amg;
    return amg_level(h, c, h->L - 1, v, h->x[h->L - 1].as<double>(), s);
}

// r = v - A x with ||r||^2 finished in the same launch, into scal[2] (VCycleSolver.py:84, :87)
int amg_residual(const psk_prec *M, const double *v, hipStream_t s) {
    const AmgHierarchy *h = M->amg;
    const int top = h->L - 1;
    return launch_spmv(h->A[top], kSpmvResid, h->x[top].as<double>(), h->r[top].as<double>(), nullptr, v,
                       h->scal.as<double>() + 2, nullptr, s);
}

int amg_apply(const psk_prec *M, const double *v, double *out, hipStream_t s) {
    const AmgHierarchy *h = M->amg;
    const int64_t n = M->n;
    if (n == 0) return PSK_OK;
    Context *c;
    PSK_TRY(ctx(&c));
    double *x = h->x[h->L - 1].as<double>();
    double *scal = h->scal.as<double>();
    int64_t *flag = reinterpret_cast<int64_t *>(scal + 1);
    double *part = scal + 2;
    const int ga = 1;   // the residual SpMV's sum: in-launch
    PSK_TRY(amg_loop_start(M, c, v, s));
    for (int k = 0; k < h->num_iters; ++k) {
        PSK_TRY(amg_cycle(M, c, v, s));                                                    // runCycle (:79)
        if (k + 1 < h->num_iters) {
            PSK_TRY(amg_residual(M, v, s));                                                // r = b - A x (:82)
            hipLaunchKernelGGL(amg_check_kernel, dim3(1), dim3(kBlock), 0, s, part, ga, scal, h->tau, flag);
            PSK_HIP(hipGetLastError());
            hipLaunchKernelGGL(amg_copy_if_kernel, vgrid(n), dim3(kBlock), 0, s, n, flag, (int64_t)1, x, out);
            PSK_HIP(hipGetLastError());
            hipLaunchKernelGGL(amg_promote_kernel, dim3(1), dim3(1), 0, s, flag);
            PSK_HIP(hipGetLastError());
        }
    }
    // the last cycle's test does not matter: converged or not (failOnMaxiter=False) x is returned
    hipLaunchKernelGGL(amg_copy_if_kernel, vgrid(n), dim3(kBlock), 0, s, n, flag, (int64_t)0, x, out);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

int amg_gs_pair(psk_prec *M, int set, int *on, int *eligible) {
    if (!M || M->kind != PSK_PREC_AMG) return fail(PSK_ERR_ARG, "amg_gs_pair: not an AMG preconditioner");
    int a = 0, e = 0;
    for (GsPairLevel &g : M->amg->gp) {
        if (set >= 0) g.on = g.eligible && set != 0;
        a += g.on;
        e += g.eligible;
    }
    if (on) *on = a;
    if (eligible) *eligible = e;
    return PSK_OK;
}

}  // namespace psk

using namespace psk;

extern "C" int psk_prec_create_amg(int32_t num_levels, psk_csr *const *A, psk_csr *const *P, psk_csr *const *R,
                                   psk_prec *const *smoother, psk_prec *coarse, int32_t num_iters, int32_t nu_pre,
                                   int32_t nu_post, double tau, psk_prec **out) {
    if (!out || num_levels < 1 || !A || !coarse || num_iters < 0 || nu_pre < 0 || nu_post < 0)
        return fail(PSK_ERR_ARG, "psk_prec_create_amg: bad arguments");
    if (num_levels > 1 && (!P || !R || !smoother)) return fail(PSK_ERR_ARG, "psk_prec_create_amg: NULL level arrays");
    const int L = num_levels;
    for (int k = 0; k < L; ++k) {
        if (!A[k]) return fail(PSK_ERR_ARG, "psk_prec_create_amg: NULL level matrix");
        if (A[k]->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_prec_create_amg: sharded matrices (replicas only)");
        if (A[k]->ncols != A[k]->n) return fail(PSK_ERR_ARG, "psk_prec_create_amg: level matrix not square");
    }
    for (int k = 0; k + 1 < L; ++k) {
        if (!P[k] || !R[k]) return fail(PSK_ERR_ARG, "psk_prec_create_amg: NULL transfer operator");
        if (P[k]->n != A[k + 1]->n || P[k]->ncols != A[k]->n)
            return fail(PSK_ERR_ARG, "psk_prec_create_amg: P[k] must be n_{k+1} x n_k");
        if (R[k]->n != A[k]->n || R[k]->ncols != A[k + 1]->n)
            return fail(PSK_ERR_ARG, "psk_prec_create_amg: R[k] must be n_k x n_{k+1}");
    }
    for (int k = 1; k < L; ++k) {
        psk_prec *S = smoother[k];
        if (!S || S->n != A[k]->n || S->kind == PSK_PREC_AMG)
            return fail(PSK_ERR_ARG, "psk_prec_create_amg: smoother[k] missing, of the wrong size or an AMG");
    }
    if (coarse->n != A[0]->n || coarse->kind == PSK_PREC_AMG)
        return fail(PSK_ERR_ARG, "psk_prec_create_amg: coarse solver of the wrong size");
    Context *c;
    PSK_TRY(ctx(&c));
    AmgHierarchy *h = new AmgHierarchy();
    h->L = L;
    h->num_iters = num_iters;
    h->nu_pre = nu_pre;
    h->nu_post = nu_post;
    h->tau = tau;
    h->A.assign(A, A + L);
    if (L > 1) {
        h->P.assign(P, P + L - 1);
        h->R.assign(R, R + L - 1);
        h->S.assign(smoother, smoother + L);
        h->S[0] = nullptr;   // built but never used by the reference (VCycleManager.py:23-24)
    }
    h->coarse = coarse;
    h->x.resize(L);
    h->f.resize(L);
    h->r.resize(L);
    h->t.resize(L);
    int rc = PSK_OK;
    for (int k = 0; k < L && rc == PSK_OK; ++k) {
        const size_t bytes = (size_t)std::max<int64_t>(A[k]->n, 1) * sizeof(double);
        rc = h->x[k].ensure(bytes);
        if (rc == PSK_OK && k < L - 1) rc = h->f[k].ensure(bytes);
        if (rc == PSK_OK && (k > 0 || L == 1)) rc = h->r[k].ensure(bytes);
        if (rc == PSK_OK && k > 0) rc = h->t[k].ensure(bytes);
    }
    if (rc == PSK_OK) rc = h->r[L - 1].ensure((size_t)std::max<int64_t>(A[L - 1]->n, 1) * sizeof(double));
    if (rc == PSK_OK) rc = h->scal.ensure((size_t)(2 + kMaxGrid) * sizeof(double));
    h->gp.resize(L);
    for (int k = 1; k < L && rc == PSK_OK; ++k) rc = gs_pair_setup(h->A[k], h->S[k], h->gp[k], c->stream);
    if (rc != PSK_OK) {
        amg_free(h);
        return rc;
    }
    psk_prec *M = new psk_prec();
    M->kind = PSK_PREC_AMG;
    M->n = A[L - 1]->n;
    M->amg = h;
    *out = M;
    return PSK_OK;
}
