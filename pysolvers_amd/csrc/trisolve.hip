// trisolve.hip — sparse triangular-solve chains on the device: right-ILUT apply
// (RightILUTPreconditioner.applyRight, ILUTPreconditioner.py:70-78), RightIC apply
// (ICPreconditioner.py:58-63), the Gauss-Seidel smoother's U^-1 (ClassicSmoothers.py:28-36) and the
// AMG coarse-level SuperLU solve (VCycleManager.py:34-37) are all "gather, lower solve, upper solve,
// gather" with some stages absent (psk_prec_create_trisolve).
//
// The reference calls SuperLU's ILU.solve(v) (scipy SuperLU, dgstrs): with Pr A Pc ~= L U,
//     bb[perm_r[i]] = v[i];  y = L^-1 bb (unit lower);  z = U^-1 y;  out[i] = z[perm_c[i]].
// The factors come from the same third-party factorisation on the host (scipy spilu, exactly the
// reference's call, ILUTPreconditioner.py:51-53): they are uploaded once per form() and the two
// triangular solves run on the GPU.
//
// One file per schedule holds its kernel and launch (trisolve_syncfree.hip: sync-free and single-workgroup LDS;
// trisolve_band.hip; trisolve_grid.hip; trisolve_levels.hip; trisolve_part.hip), trisolve_plan.hip the host
// cost models that pick one and pack its layout, trisolve.hpp what they share; trisolve_sweep.hip holds the opt-in
// approximate apply by Jacobi sweeps (psk_prec_trisolve_sweeps). Here: the apply chain, the upload of a plan and
// the C entry points.
#include "trisolve.hpp"

#include <string>

namespace psk {

__global__ void fill_sentinel_kernel(int64_t n, double *x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) reinterpret_cast<uint64_t *>(x)[i] = kSentinel;
}

// out[i] = z[perm[i]] (perm == nullptr: copy)
__global__ void gather_perm_kernel(int64_t n, const double *__restrict__ z, const int32_t *__restrict__ perm,
                                   double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = perm ? z[perm[i]] : z[i];
}

// x[i] = x[i] + z[perm[i]]: the last gather fused with the smoother's x + dx (ClassicSmoothers.py:34),
// the same single rounding as gathering into a temporary and adding it (24 instead of 40 B/row)
__global__ void gather_add_kernel(int64_t n, const double *__restrict__ z, const int32_t *__restrict__ perm,
                                  double *__restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] + (perm ? z[perm[i]] : z[i]);
}

// the output of one factor before its solve: the sentinel where the schedule's waits read it (the grid
// schedule: only its published lines; every other schedule: every row)
static int fill_factor_output(const TriFactor &T, int64_t n, double *x, hipStream_t s) {
    if (T.schedule == kSchedLevel) return PSK_OK;   // nothing polls: one workgroup, dependencies through LDS
    if (T.schedule == kSchedGrid) return launch_grid_fill(T, n, x, nullptr, s);
    hipLaunchKernelGGL(fill_sentinel_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n, x);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// x = T^-1 rhs[rhs_idx] for one factor, with the factor's schedule
static int launch_factor(const Context *c, int64_t n, const TriFactor &T, const double *rhs, const int32_t *rhs_idx,
                         double *x, int32_t *err, hipStream_t s) {
    if (T.sweeps > 0) return launch_sweeps(c, n, T, rhs, rhs_idx, x, err, s);   // opt-in (psk_prec_trisolve_sweeps)
    switch (T.schedule) {
    case kSchedLds: return launch_lds(c, n, T, rhs, rhs_idx, x, err, s);
    case kSchedLevel: return launch_levels(c, n, T, rhs, rhs_idx, x, err, s);
    case kSchedPart: return launch_part(c, n, T, rhs, rhs_idx, x, err, s);
    case kSchedGrid: return launch_grid(c, n, T, rhs, rhs_idx, x, err, s);
    case kSchedBand: return launch_band(c, n, T, rhs, rhs_idx, x, err, s);
    default: return launch_syncfree(c, n, T, rhs, rhs_idx, x, err, s);
    }
}

// out = (U^-1 L^-1 v[gather_in])[gather_out] for a triangular-solve chain (device pointers; out may
// not alias v)
// out = M^-1 v; add: out += M^-1 v (the Gauss-Seidel smoother's update, fused into the last gather)
static int ilu_apply_impl(const psk_prec *M, const double *v, double *out, bool add, hipStream_t s) {
    const int64_t n = M->n;
    if (n == 0) return PSK_OK;
    Context *c;
    PSK_TRY(ctx(&c));
    const unsigned fb = (unsigned)((n + kBlock - 1) / kBlock);
    double *y = M->work, *z = M->work + n;
    const int nbuf = (M->lo.present ? 1 : 0) + (M->up.present ? 1 : 0);
    // factors whose schedule fills (or needs) no sentinel of its own: the grid schedule's published lines only,
    // none for the levels schedule
    // none either for a factor in sweep mode (nothing waits): both swept, no fill at all
    auto own_fill = [](const TriFactor &T) {
        return T.sweeps > 0 || T.schedule == kSchedGrid || T.schedule == kSchedLevel;
    };
    const bool grid_any = (M->lo.present && own_fill(M->lo)) || (M->up.present && own_fill(M->up));
    if (nbuf > 0 && !grid_any) {
        hipLaunchKernelGGL(fill_sentinel_kernel, dim3((unsigned)((nbuf * n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           s, nbuf * n, y);   // y and z are contiguous
        PSK_HIP(hipGetLastError());
    } else if (nbuf > 0) {
        if (M->lo.present && M->lo.sweeps == 0) PSK_TRY(fill_factor_output(M->lo, n, y, s));
        if (M->up.present && M->up.sweeps == 0) PSK_TRY(fill_factor_output(M->up, n, M->lo.present ? z : y, s));
    }
    const double *cur = v;                // current right-hand side
    const int32_t *cur_idx = M->gather_in;
    const TriFactor &first = M->lo.present ? M->lo : M->up;
    if (cur_idx && first.present && first.sweeps == 0 &&
        (first.schedule == kSchedGrid || first.schedule == kSchedPart)) {   // rhs[row]
        hipLaunchKernelGGL(gather_perm_kernel, dim3(fb), dim3(kBlock), 0, s, n, cur, cur_idx, M->work + 2 * n);
        PSK_HIP(hipGetLastError());
        cur = M->work + 2 * n;
        cur_idx = nullptr;
    }
    if (M->lo.present) {
        PSK_TRY(launch_factor(c, n, M->lo, cur, cur_idx, y, M->err, s));
        cur = y;
        cur_idx = nullptr;
    }
    if (M->up.present) {
        double *dst = M->lo.present ? z : y;
        PSK_TRY(launch_factor(c, n, M->up, cur, cur_idx, dst, M->err, s));
        cur = dst;
        cur_idx = nullptr;
    }
    if (cur_idx) {   // no factor at all: out = v[gather_in][gather_out]
        hipLaunchKernelGGL(gather_perm_kernel, dim3(fb), dim3(kBlock), 0, s, n, cur, cur_idx, y);
        PSK_HIP(hipGetLastError());
        cur = y;
    }
    if (add) hipLaunchKernelGGL(gather_add_kernel, dim3(fb), dim3(kBlock), 0, s, n, cur, M->gather_out, out);
    else hipLaunchKernelGGL(gather_perm_kernel, dim3(fb), dim3(kBlock), 0, s, n, cur, M->gather_out, out);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

int ilu_apply(const psk_prec *M, const double *v, double *out, hipStream_t s) {
    return ilu_apply_impl(M, v, out, false, s);
}

int ilu_apply_add(const psk_prec *M, const double *v, double *x, hipStream_t s) {
    return ilu_apply_impl(M, v, x, true, s);
}

int ilu_check_error(const psk_prec *M, hipStream_t s) {
    int32_t h = 0;
    PSK_HIP(hipMemcpyAsync(&h, M->err, 4, hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    if (h) {
        // a launch that stopped waiting may have left its scheduling words armed: re-zero them (and the
        // error word) so that the next apply starts clean
        for (const TriFactor *T : {&M->lo, &M->up})
            if (T->present && T->sched) (void)hipMemsetAsync(T->sched, 0, kSchedWords * sizeof(uint32_t), s);
        (void)hipMemsetAsync(M->err, 0, sizeof(int32_t), s);
        (void)hipStreamSynchronize(s);
        return fail(PSK_ERR_HIP, "triangular solve: dependency wait exceeded its bound, code " + std::to_string(h));
    }
    return PSK_OK;
}

static void free_all(std::initializer_list<void *> ptrs) {
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
}
void TriFactor::Band::release() {
    free_all({rec_row, rec_end, rec_c, rec_v, rec_d});
    *this = Band();
}
void TriFactor::Grid::release() {
    free_all({coef, dict, idx, flag});
    *this = Grid();
}
void TriFactor::Part::release() {
    free_all({seg, rp, code, row, va});
    *this = Part();
}
void TriFactor::Levels::release() {
    free_all({rc, sl, cf, dg, b});
    *this = Levels();
}
void TriFactor::release() {
    band.release();
    grid.release();
    part.release();
    lv.release();
    free_all({rowptr, colidx, vals, diag, order, sched});
    *this = TriFactor();
}

template <class T>
static int upload(T **d, const std::vector<T> &h) {
    if (h.empty()) {
        *d = nullptr;
        return PSK_OK;
    }
    if (hipMalloc(d, h.size() * sizeof(T)) != hipSuccess) return fail(PSK_ERR_ALLOC, "hipMalloc trisolve");
    if (hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
        return fail(PSK_ERR_HIP, "hipMemcpy trisolve");
    return PSK_OK;
}

static int check_perm(int64_t n, const int32_t *p, const char *what) {
    std::vector<char> seen(n, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (p[i] < 0 || p[i] >= n || seen[p[i]]) return fail(PSK_ERR_ARG, std::string(what) + ": not a permutation");
        seen[p[i]] = 1;
    }
    return PSK_OK;
}

// Plan (host only: plan_factor), then upload one factor. The two numbers the plan takes from the device: its
// CU count and the waves of a sync-free launch.
static int make_factor(const Context *c, int64_t n, const int32_t *rp, const int32_t *ci, const double *va, bool upper,
                       bool unit, const std::vector<int32_t> &nat, TriFactor &T) {
    FactorPlan P;
    PSK_TRY(plan_factor(n, rp, ci, va, upper, unit, nat, c->num_cus, (int64_t)syncfree_grid(c) * kWaves, P));
    T = P.T;
    int rc = PSK_OK;
    auto up = [&rc](auto **d, const auto &h) {
        if (rc == PSK_OK) rc = upload(d, h);
    };
    up(&T.rowptr, P.krp);
    up(&T.colidx, P.kci);
    up(&T.vals, P.kva);
    up(&T.diag, P.dg);
    up(&T.order, P.order);
    up(&T.band.rec_row, P.rec_row);
    up(&T.band.rec_end, P.rec_end);
    up(&T.band.rec_c, P.rec_c);
    up(&T.band.rec_v, P.rec_v);
    up(&T.band.rec_d, P.rec_d);
    up(&T.grid.coef, P.gcoef);
    up(&T.grid.idx, P.gidx);
    up(&T.grid.dict, P.gdict);
    up(&T.grid.flag, std::vector<int32_t>(T.grid.dict_n > 0 ? 1 : 0, 0));
    up(&T.sched, std::vector<uint32_t>(kSchedWords, 0u));   // block tickets / enrolment
    up(&T.part.seg, P.pseg);
    up(&T.part.rp, P.prp);
    up(&T.part.code, P.pcode);
    up(&T.part.row, P.prow);
    up(&T.part.va, P.pva);
    up(&T.lv.rc, P.lrc);
    up(&T.lv.sl, P.lsl);
    up(&T.lv.cf, P.lcf);
    up(&T.lv.dg, P.ldg);
    up(&T.lv.b, std::vector<double>(P.lrc.size(), 0.0));
    return rc;
}

}  // namespace psk

using namespace psk;

extern "C" int psk_prec_create_trisolve(int64_t n, const int32_t *l_rowptr, const int32_t *l_colidx,
                                        const double *l_vals, int32_t l_unit, const int32_t *u_rowptr,
                                        const int32_t *u_colidx, const double *u_vals, int32_t u_unit,
                                        const int32_t *gather_in, const int32_t *gather_out, psk_prec **out) {
    if (!out || n < 0) return fail(PSK_ERR_ARG, "psk_prec_create_trisolve: bad arguments");
    if (n >= INT32_MAX) return fail(PSK_ERR_UNSUPPORTED, "psk_prec_create_trisolve: n must fit int32");
    if (l_rowptr && l_rowptr[n] > 0 && (!l_colidx || !l_vals)) return fail(PSK_ERR_ARG, "lower factor: NULL arrays");
    if (u_rowptr && u_rowptr[n] > 0 && (!u_colidx || !u_vals)) return fail(PSK_ERR_ARG, "upper factor: NULL arrays");
    if (gather_in) PSK_TRY(check_perm(n, gather_in, "gather_in"));
    if (gather_out) PSK_TRY(check_perm(n, gather_out, "gather_out"));
    Context *c;
    PSK_TRY(ctx(&c));
    psk_prec *M = new psk_prec();
    M->kind = PSK_PREC_ILU;
    M->n = n;
    int rc = PSK_OK;
    // natural index of every factor row (the partitioned schedule's strips): L row r solves equation
    // gather_in[r]; U row gather_out[i] gives unknown i
    std::vector<int32_t> nat_l, nat_u;
    if (gather_in) nat_l.assign(gather_in, gather_in + n);
    if (gather_out) {
        nat_u.assign(n, 0);
        for (int64_t i = 0; i < n; ++i) nat_u[gather_out[i]] = (int32_t)i;
    }
    if (l_rowptr) rc = make_factor(c, n, l_rowptr, l_colidx, l_vals, false, l_unit != 0, nat_l, M->lo);
    if (rc == PSK_OK && u_rowptr) rc = make_factor(c, n, u_rowptr, u_colidx, u_vals, true, u_unit != 0, nat_u, M->up);
    std::vector<int32_t> gin, gout;
    if (gather_in) gin.assign(gather_in, gather_in + n);
    if (gather_out) gout.assign(gather_out, gather_out + n);
    if (rc == PSK_OK) rc = upload(&M->gather_in, gin);
    if (rc == PSK_OK) rc = upload(&M->gather_out, gout);
    if (rc == PSK_OK && n > 0 && hipMalloc(&M->work, (size_t)(3 * n) * sizeof(double)) != hipSuccess)
        rc = fail(PSK_ERR_ALLOC, "trisolve work");
    if (rc == PSK_OK && hipMalloc(&M->err, sizeof(int32_t)) != hipSuccess) rc = fail(PSK_ERR_ALLOC, "trisolve err");
    if (rc == PSK_OK && hipMemset(M->err, 0, sizeof(int32_t)) != hipSuccess) rc = fail(PSK_ERR_HIP, "trisolve err");
    if (rc != PSK_OK) {
        psk_prec_destroy(M);
        return rc;
    }
    *out = M;
    return PSK_OK;
}

// SuperLU ILU.solve: bb[perm_r[i]] = v[i]  <=>  bb[j] = v[pinv[j]];  out[i] = z[perm_c[i]]
extern "C" int psk_prec_create_ilu(int64_t n, const int32_t *l_rowptr, const int32_t *l_colidx, const double *l_vals,
                                   const int32_t *u_rowptr, const int32_t *u_colidx, const double *u_vals,
                                   const int32_t *perm_r, const int32_t *perm_c, psk_prec **out) {
    if (!out || n < 0 || !l_rowptr || !u_rowptr || !perm_r || !perm_c)
        return fail(PSK_ERR_ARG, "psk_prec_create_ilu: NULL argument");
    PSK_TRY(check_perm(n, perm_r, "ILU perm_r"));
    std::vector<int32_t> pinv(n);
    for (int64_t i = 0; i < n; ++i) pinv[perm_r[i]] = (int32_t)i;
    return psk_prec_create_trisolve(n, l_rowptr, l_colidx, l_vals, 1, u_rowptr, u_colidx, u_vals, 0, pinv.data(),
                                    perm_c, out);
}

extern "C" int psk_trisolve_grid_plan(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                                      int32_t upper, int64_t *out) {
    if (n <= 0 || !rowptr || !colidx || !vals || !out) return fail(PSK_ERR_ARG, "psk_trisolve_grid_plan: bad arguments");
    HostFactor F;
    F.n = n;
    F.upper = upper != 0;
    std::vector<double> ova, dg;
    PSK_TRY(split_factor(n, rowptr, colidx, vals, upper == 0, false, F.rp, F.ci, ova, dg));
    GridPlan gp;
    plan_grid(F, gp);
    if (!gp.ok || n > kGridMaxRows)
        return fail(PSK_ERR_UNSUPPORTED, "psk_trisolve_grid_plan: factor is not a 2-D stencil (grid schedule)");
    const int64_t v[7] = {gp.w, gp.H, gp.sigma2, gp.phase, gp.off,
                          (gp.w - 1) + grid_g(gp.sigma2, gp.phase, kGridLanes - 1) - grid_g(gp.sigma2, gp.phase, 0) + 1,
                          (int64_t)gp.K};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    return PSK_OK;
}

extern "C" int psk_prec_trisolve_grid_info(const psk_prec *M, int32_t which, int64_t *out) {
    if (!M || M->kind != PSK_PREC_ILU || (which != 0 && which != 1) || !out)
        return fail(PSK_ERR_ARG, "psk_prec_trisolve_grid_info: not a triangular-solve chain / bad factor");
    const TriFactor &T = which == 0 ? M->lo : M->up;
    if (!T.present || T.grid.K == 0)
        return fail(PSK_ERR_UNSUPPORTED, "psk_prec_trisolve_grid_info: factor is not a 2-D stencil (grid schedule)");
    const int64_t v[7] = {T.grid.w, T.grid.H, T.grid.sigma, T.grid.phase, T.grid.off, T.grid.S, T.grid.dict_n};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    return PSK_OK;
}

extern "C" int psk_prec_trisolve_schedule(psk_prec *M, int32_t which, int32_t set, int32_t *schedule,
                                          int64_t *blocks, int32_t *ring_words, double *est_syncfree_us,
                                          double *est_band_us) {
    if (!M || M->kind != PSK_PREC_ILU || (which != 0 && which != 1))
        return fail(PSK_ERR_ARG, "psk_prec_trisolve_schedule: not a triangular-solve chain / bad factor");
    TriFactor &T = which == 0 ? M->lo : M->up;
    if (!T.present) return fail(PSK_ERR_ARG, "psk_prec_trisolve_schedule: factor absent");
    if (set == kSchedBand && T.band.K == 0)
        return fail(PSK_ERR_UNSUPPORTED, "psk_prec_trisolve_schedule: factor not eligible for the band schedule "
                                         "(more than 8 entries in a row or a level wider than a chunk)");
    if (set == kSchedLds && (M->n > kLdsMaxRows || M->n == 0))
        return fail(PSK_ERR_UNSUPPORTED, "psk_prec_trisolve_schedule: factor too large for the LDS schedule");
    if (set == kSchedGrid && T.grid.K == 0)
        return fail(PSK_ERR_UNSUPPORTED, "psk_prec_trisolve_schedule: factor is not a 2-D stencil (grid schedule)");
    if (set == kSchedPart && T.part.P == 0)
        return fail(PSK_ERR_UNSUPPORTED, "psk_prec_trisolve_schedule: partitioned layout not built for this factor "
                                         "(built when chosen, or with PSK_TRISOLVE_PART=1 at creation)");
    if (set == kSchedLevel && T.lv.steps == 0)
        return fail(PSK_ERR_UNSUPPORTED, "psk_prec_trisolve_schedule: levels layout not built for this factor "
                                         "(built when chosen, or with PSK_TRISOLVE_LEVELS=1 at creation)");
    if (set >= kSchedSyncFree && set <= kSchedLevel) T.schedule = set;
    else if (set != -1) return fail(PSK_ERR_ARG, "psk_prec_trisolve_schedule: set must be -1 or 0..5");
    if (schedule) *schedule = T.schedule;
    if (blocks) *blocks = T.band.nblocks;
    if (ring_words) *ring_words = T.band.ring_words;
    if (est_syncfree_us) *est_syncfree_us = T.est_us[kSchedSyncFree];
    if (est_band_us) *est_band_us = T.est_us[kSchedBand];
    return PSK_OK;
}
