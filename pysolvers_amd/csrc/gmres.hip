// gmres.hip — device-resident right-preconditioned GMRES (GMRESSolver.solve, GMRESSolver.py:55-180).
//
// Krylov basis Q lives in HBM column-major (each q_j contiguous, n x (K+1)); the Hessenberg
// column, the Givens table and g live in HBM too and are advanced by one lane of workgroup 0.
// Per Arnoldi step k (one-shot launches, one 512-element tile per workgroup). The host only enqueues: in front of
// step k it waits for the event behind step k - 3 and reads the done stamp G3 stores when it raises `done`
// (solve_loop.hpp StampPoll), so at most two steps are enqueued behind the one that ended the cycle, and they
// return at once. It synchronises after the first cycle start (b = 0), at each cycle's end and for the results.
//   G1      u = A M^-1 q_k, with q_0.u finished in-launch (gridsum)      (:107, first MGS dot)
//   G2_j    h_jk (G1's or G2_{j-1}'s grid sum); u -= h_jk q_j; q_{j+1}.u (:110-112, MGS, j=0..k)
//           finished in-launch (for j==k u.u, the norm)
//   G3      h_{k+1,k} = ||u||; breakdown test; q_{k+1} = u / h_{k+1,k};  (:115-125)
//           workgroup 0: old rotations, new rotation, g update, |g_{k+1}|, convergence (:133-158)
// Bytes per step (algorithmic): the SpMV's, then 32n per G2_j (u read + written, q_j, q_{j+1}),
// 24n for G2_k, 16n for G3.
// On convergence the (k+1)^2 triangular-ish least-squares system is solved on the host (it is
// 31x31 at config 3; LU with partial pivoting as LAPACK dgesv, :159), then
//   x = M^-1 (Q[:, :k+1] y) on the device (:160) and the true residual ||b - A x|| (:163-164).
// restart == 0 reproduces the reference (one cycle, Krylov dimension = maxiter). restart = m > 0
// is the restarted GMRES(m) the reference lacks: cycles of m steps from r = b - A x.
// Reference defects: self.precond never set (:71) -> we always form M;
// NameError at maxiter (:180) -> we return the MAXITER status handleMaxiter would have built.
#include "psk_internal.hpp"
#include "dist.hpp"
#include "solve_loop.hpp"

#include <cmath>
#include <cstdio>

namespace psk {

struct GmresState {
    int32_t done;    // 0 running, 1 converged (recursive test or Arnoldi breakdown)
    int32_t brk;     // Arnoldi breakdown flag
    int32_t kconv;   // step k at which `done` was raised
    int32_t zero_b;  // ||b|| == 0
    double normB;
    double tauNormB;
    double rec;      // last |g[k+1]|
    double true_resid;
    int64_t *hdone;  // host-mapped done stamp (solve_loop.hpp): k + 2 for step k of a cycle, 1 for b = 0
    int64_t hgen;    // this solve's generation in the stamp's high bits
};

__global__ __launch_bounds__(kBlock) void gm_selfdot_kernel(int64_t n, const double *__restrict__ v,
                                                            double *__restrict__ part) {
    __shared__ double sh[kWaves];
    int64_t t0, t1;
    block_range((n + kVecTile - 1) / kVecTile, t0, t1);
    const int64_t i0 = t0 * kVecTile, i1 = (t1 * kVecTile < n) ? t1 * kVecTile : n;
    double acc = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kBlock) acc = fma(v[i], v[i], acc);
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// cycle start: beta = ||r0||, q_0 = r0/beta, g = beta e1 (:90-97)
__global__ __launch_bounds__(kBlock) void gm_start_kernel(int64_t n, const double *__restrict__ r0,
                                                          double *__restrict__ q0, const double *__restrict__ part,
                                                          int np, double *__restrict__ g, int Kp1, GmresState *st,
                                                          double tau, int first, double normb_caller,
                                                          int64_t *hdone, int64_t hgen) {
    __shared__ double sh[kWaves];
    const double bb = reduce_partials(part, np, 1, sh);
    const double beta = sqrt(bb);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (first) {
            // self.norm(b)  :66: == npla.norm(r0) since r0 = b, or the caller's norm of b
            const double nb = normb_caller > 0.0 ? normb_caller : beta;
            st->normB = nb;
            st->tauNormB = tau * nb;
            st->zero_b = beta == 0.0;
            st->hdone = hdone;
            st->hgen = hgen;
            if (beta == 0.0) {                 // :67-68
                st->done = 1;
                done_stamp_store(hdone, hgen, 1);
            }
        }
        for (int j = 0; j < Kp1; ++j) g[j] = beta * (j == 0 ? 1.0 : 0.0);   // g = beta*e1
    }
    if (beta == 0.0) return;
    int64_t t0, t1;
    block_range((n + kVecTile - 1) / kVecTile, t0, t1);
    const int64_t i0 = t0 * kVecTile, i1 = (t1 * kVecTile < n) ? t1 * kVecTile : n;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kBlock) q0[i] = r0[i] / beta;   // :91
}

// MGS step j of Arnoldi column k, one-shot (one 512-element tile per workgroup, 16-B accesses):
// h = HBar[j,k] (the previous launch's grid sum), u -= h q_j, and the next dot — q_{j+1}.u, or u.u
// for j == k (the norm of :115) — finished in-launch by gridsum into hout.
__global__ __launch_bounds__(kBlock) void gm_mgs_kernel(int64_t n, double *__restrict__ u,
                                                        const double *__restrict__ qj,
                                                        const double *__restrict__ qnext,
                                                        const double *__restrict__ hin, double *__restrict__ hcol,
                                                        int j, GridSum gs, const GmresState *st) {
    if (st->done) return;
    __shared__ double sh[kWaves];
    const double h = *hin;                                  // HBar[j,k] = np.dot(Q[:,j], u)  :111
    if (blockIdx.x == 0 && threadIdx.x == 0) hcol[j] = h;
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    uint32_t ticket = 0;
    double acc = 0.0;
    if (i + 1 < n) {
        // q_j is not read again this step (non-temporal); u and q_{j+1} are read by the next launch
        dv2 uv = ld2(u + i);
        const dv2 qv = ld2nt(qj + i);
        dv2 nv = uv;
        if (qnext) nv = ld2(qnext + i);
        ticket = gridsum_ticket(gs);
        uv.x = uv.x - h * qv.x;                             // u -= HBar[j,k]*Q[:,j]  :112
        uv.y = uv.y - h * qv.y;
        st2(u + i, uv);
        if (!qnext) nv = uv;
        acc = fma(nv.x, uv.x, acc);
        acc = fma(nv.y, uv.y, acc);
    } else if (i < n) {
        ticket = gridsum_ticket(gs);
        const double ui = u[i] - h * qj[i];
        u[i] = ui;
        acc = (qnext ? qnext[i] : ui) * ui;
    }
    const double v = block_sum(acc, sh);
    gridsum_publish<1>(gs, &v, sh, ticket);
}

__device__ __forceinline__ void givens_apply(double *x, double c, double s, int i) {
    const double xi = x[i], xi1 = x[i + 1];            // Givens.py:30-34
    x[i] = c * xi + s * xi1;
    x[i + 1] = -s * xi + c * xi1;
}

// h_{k+1,k}, breakdown, q_{k+1}, Givens, convergence; one-shot like gm_mgs_kernel (hsq: the grid
// sum u.u of the last MGS launch)
__global__ __launch_bounds__(kBlock) void gm_normalize_kernel(
    int64_t n, const double *__restrict__ u, double *__restrict__ qnext, const double *__restrict__ hsq,
    double *__restrict__ H, double *__restrict__ R, double *__restrict__ CS, double *__restrict__ g, int ld, int k,
    int64_t it, GmresState *st, double *__restrict__ hist) {
    if (st->done) return;
    const double hk = sqrt(*hsq);                                   // npla.norm(u)  :115
    const double *hcol = H + (int64_t)k * ld;
    double hh = 0.0;
    for (int j = 0; j <= k; ++j) hh += hcol[j] * hcol[j];
    const double hlast = sqrt(hh);                                  // npla.norm(HBar[0:k+1,k])  :121
    const bool brk = fabs(hk) <= 1.0e-16 * hlast;                    // :122
    const int64_t i = (int64_t)blockIdx.x * kVecTile + 2 * threadIdx.x;
    if (!brk) {                                                     // Q[:,k+1] = u / HBar[k+1,k]  :125
        if (i + 1 < n) {
            const dv2 uv = ld2nt(u + i);
            dv2 q;
            q.x = uv.x / hk;
            q.y = uv.y / hk;
            st2(qnext + i, q);
        } else if (i < n) {
            qnext[i] = u[i] / hk;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        H[(int64_t)k * ld + k + 1] = hk;
        double *rc = R + (int64_t)k * ld;
        for (int j = 0; j <= k; ++j) rc[j] = hcol[j];
        rc[k + 1] = hk;
        for (int j = 0; j < k; ++j) givens_apply(rc, CS[2 * j], CS[2 * j + 1], j);   // :133-135
        const double hyp = sqrt(rc[k + 1] * rc[k + 1] + rc[k] * rc[k]);          // Givens.py:8-10
        const double s = rc[k + 1] / hyp;
        const double c = rc[k] / hyp;
        CS[2 * k] = c;
        CS[2 * k + 1] = s;
        givens_apply(rc, c, s, k);                                                 // :145
        givens_apply(g, c, s, k);                                                  // :148
        const double nr = fabs(g[k + 1]);                                          // :152
        hist[it] = nr;
        st->rec = nr;
        if (brk || nr <= st->tauNormB) {                                           // :158
            st->brk = brk;
            st->kconv = k;
            st->done = 1;
            done_stamp_store(st->hdone, st->hgen, k + 2);
        }
    }
}

// x (+)= M^-1 (Q[:, :k1] y)   (:160)
__global__ __launch_bounds__(kBlock) void gm_update_x_kernel(int64_t n, const double *__restrict__ Q,
                                                             int64_t ldq, const double *__restrict__ y, int k1,
                                                             const double *__restrict__ dinv,
                                                             double *__restrict__ x, int accumulate) {
    __shared__ double ys[1024];
    for (int j = threadIdx.x; j < k1 && j < 1024; j += kBlock) ys[j] = y[j];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < k1; ++j) s = fma(Q[(int64_t)j * ldq + i], j < 1024 ? ys[j] : y[j], s);
    const double v = dinv ? dinv[i] * s : s;
    x[i] = accumulate ? x[i] + v : v;
}

__global__ __launch_bounds__(kBlock) void gm_add_or_copy_kernel(int64_t n, const double *__restrict__ v,
                                                                double *__restrict__ x, int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) x[i] = accumulate ? x[i] + v[i] : v[i];
}

__global__ __launch_bounds__(kBlock) void gm_true_resid_kernel(const double *part, int np, GmresState *st) {
    __shared__ double sh[kWaves];
    const double rr = reduce_partials(part, np, 1, sh);
    if (threadIdx.x == 0) st->true_resid = sqrt(rr);   // self.norm(resid)  :164
}

// LU with partial pivoting (LAPACK dgesv semantics) on a small dense column-major system.
static bool small_solve(int m, const double *Rcm, int ld, const double *rhs, std::vector<double> &y) {
    std::vector<double> a((size_t)m * m);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) a[(size_t)i * m + j] = Rcm[(size_t)j * ld + i];
    y.assign(rhs, rhs + m);
    std::vector<int> piv(m);
    for (int kk = 0; kk < m; ++kk) {
        int p = kk;
        double best = std::fabs(a[(size_t)kk * m + kk]);
        for (int i = kk + 1; i < m; ++i)
            if (std::fabs(a[(size_t)i * m + kk]) > best) {
                best = std::fabs(a[(size_t)i * m + kk]);
                p = i;
            }
        if (a[(size_t)p * m + kk] == 0.0) return false;
        if (p != kk) {
            for (int j = 0; j < m; ++j) std::swap(a[(size_t)p * m + j], a[(size_t)kk * m + j]);
            std::swap(y[p], y[kk]);
        }
        for (int i = kk + 1; i < m; ++i) {
            const double l = a[(size_t)i * m + kk] / a[(size_t)kk * m + kk];
            a[(size_t)i * m + kk] = l;
            for (int j = kk + 1; j < m; ++j) a[(size_t)i * m + j] -= l * a[(size_t)kk * m + j];
            y[i] -= l * y[kk];
        }
    }
    for (int i = m - 1; i >= 0; --i) {
        double s = y[i];
        for (int j = i + 1; j < m; ++j) s -= a[(size_t)i * m + j] * y[j];
        y[i] = s / a[(size_t)i * m + i];
    }
    return true;
}

// K: the Krylov basis of one cycle (restart, or maxiter when it is 0), at most maxiter, at least 1
static int64_t gm_basis(int64_t maxiter, int64_t restart) {
    const int64_t K = restart > 0 && restart < maxiter ? restart : maxiter;
    return K < 1 ? 1 : K;
}

struct GmresWork {
    double *Q, *u, *x, *bv, *w, *tt;   // w, tt: general (ILU) preconditioner only (M^-1 q_k, scratch)
    GmresState *st;
    double *H, *R, *CS, *g, *pa, *dhist, *dy, *hv;
    int64_t ldq;     // doubles between two columns of Q (a column is padded to 256 bytes)
    size_t hbytes;   // the extent of H, and of R
};
// the layout of A->ws (big) and A->ws_small (sm): run on null-based carvers for the sizes, then on the buffers
static void gm_layout(Carve &big, Carve &sm, int64_t n, int64_t maxiter, int64_t K, bool gen, GmresWork &w) {
    const size_t vec = (size_t)n * 8, ld = (size_t)K + 1;
    const size_t col = (vec + 255) / 256 * 256;
    w.ldq = (int64_t)(col / 8);
    w.Q = big.take<double>(col * ld);
    w.u = big.take<double>(vec);
    w.x = big.take<double>(vec);
    w.bv = big.take<double>(vec);
    w.w = gen ? big.take<double>(vec) : nullptr;
    w.tt = gen ? big.take<double>(vec) : nullptr;
    w.st = sm.take<GmresState>(sizeof(GmresState));
    w.H = sm.take<double>(ld * K * 8);
    const size_t hend = sm.off;
    w.R = sm.take<double>(ld * K * 8);
    w.hbytes = sm.off - hend;
    w.CS = sm.take<double>((size_t)2 * K * 8);
    w.g = sm.take<double>(ld * 8);
    w.pa = sm.take<double>((size_t)kMaxGrid * 8);   // partials of the cycle-start norm / the residual's sum
    w.dhist = sm.take<double>((size_t)(maxiter + 1) * 8);
    w.dy = sm.take<double>(ld * 8);
    w.hv = sm.take<double>((size_t)(K + 2) * 8);    // K + 2 grid sums of a step (gm_mgs_kernel)
}
void gmres_layout_probe(int64_t n, int64_t maxiter, int64_t restart, bool gen, std::vector<int64_t> *log, int64_t *bytes) {
    GmresWork w;
    const int64_t K = gm_basis(maxiter, restart);
    layout_sizes([&](Carve &big, Carve &sm) { gm_layout(big, sm, n, maxiter, K, gen, w); }, 0, log, bytes);
}
// A->ws and A->ws_small carved by gm_layout; need[2]: the bytes of each the layout covers; grow: as workspace_carve
static int gm_workspace(psk_csr *A, int64_t maxiter, int64_t restart, bool gen, bool grow, GmresWork &w, int64_t *need) {
    const int64_t K = gm_basis(maxiter, restart);
    auto layout = [&](Carve &big, Carve &sm) { gm_layout(big, sm, A->n, maxiter, K, gen, w); };
    return workspace_carve(A, 0, grow, layout, need);
}
// the regions psk_gmres(maxiter, restart, gen) carved on this matrix. Host code only (psk_lab_gmres_internals,
// psk_lab_gmres_prefill).
int gmres_work_view(psk_csr *A, int64_t maxiter, int64_t restart, bool gen, bool grow, GmresView *v) {
    if (!A || !v || maxiter < 0 || restart < 0 || A->n < 0) return fail(PSK_ERR_ARG, "gmres_work_view: bad arguments");
    int64_t need[2];
    GmresWork w;
    PSK_TRY(gm_workspace(A, maxiter, restart, gen, grow, w, need));
    v->n = A->n;
    v->K = gm_basis(maxiter, restart);
    v->ldq = w.ldq;
    v->Q = w.Q;
    v->H = w.H;
    v->R = w.R;
    v->CS = w.CS;
    v->g = w.g;
    v->dy = w.dy;
    v->done = &w.st->done;
    v->brk = &w.st->brk;
    v->kconv = &w.st->kconv;
    v->normB = &w.st->normB;
    v->tauNormB = &w.st->tauNormB;
    v->rec = &w.st->rec;
    v->big = A->ws.p;
    v->big_bytes = (size_t)need[0];
    v->small = A->ws_small.p;
    v->small_bytes = (size_t)need[1];
    return PSK_OK;
}

// what the phases share. nv: the one-shot grid of the MGS kernels; gen: M^-1 q_k is materialised in w before the SpMV;
// C = 1: a poll chunk is one step
struct GmresRun : SolveRun {
    int64_t K;               // the basis of a full cycle
    int gv, ld;              // gv: the grid of the cycle start; ld = K + 1, the leading dimension of H and R
    GmresWork w;
    int64_t it, spmvs;       // iterations completed before this cycle; SpMV launches enqueued
    bool hit_maxiter;
    GmresState hs;           // the device state as last read (gm_read_state)
};

// before anything is allocated: the K + 1 basis columns and four more vectors, as the layout pads them, against
// the free HBM
static int gm_fits_hbm(const GmresRun &r) {
    Carve big, sm;
    GmresWork w;
    gm_layout(big, sm, r.n, r.ctl->maxiter, r.K, r.gen, w);
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && (size_t)(r.K + 5) * w.ldq * 8 > fr)
        return fail(PSK_ERR_ALLOC, "psk_gmres: Krylov basis of " + std::to_string(r.K + 1) +
                                       " vectors does not fit in HBM; use restart");
    return PSK_OK;
}

static int gm_read_state(GmresRun &r) {
    PSK_HIP(hipMemcpyAsync(&r.hs, r.w.st, sizeof(r.hs), hipMemcpyDeviceToHost, r.s));
    PSK_HIP(hipStreamSynchronize(r.s));
    return PSK_OK;
}

// cycle start: r0 = b (first cycle, :87) or b - A x (restart); beta = ||r0||, q_0, g
static int gm_cycle_start(GmresRun &r, const StampPoll &poll, bool first) {
    GmresWork &w = r.w;
    const double *r0 = w.bv;
    int np = r.gv;   // partials of ||r0||^2: gm_selfdot_kernel's, one per workgroup
    if (first) {
        hipLaunchKernelGGL(gm_selfdot_kernel, dim3(r.gv), dim3(kBlock), 0, r.s, r.n, w.bv, w.pa);
    } else {
        PSK_TRY(launch_spmv(r.A, kSpmvResid, w.x, w.u, nullptr, w.bv, w.pa, nullptr, r.s));
        ++r.spmvs;
        r0 = w.u;
        np = 1;      // the residual SpMV finishes its sum in-launch (gridsum)
    }
    hipLaunchKernelGGL(gm_start_kernel, dim3(r.gv), dim3(kBlock), 0, r.s, r.n, r0, w.Q, w.pa, np, w.g, r.ld, w.st,
                       r.ctl->tau, first ? 1 : 0, first ? r.ctl->norm_b : 0.0, poll.hdone(), poll.hgen());
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// Arnoldi step k of the cycle: [w = M^-1 q_k], u = A M^-1 q_k with q_0.u, the k + 1 MGS launches, the normalisation
static int gm_step(GmresRun &r, int64_t k) {
    GmresWork &w = r.w;
    hipStream_t s = r.s;
    const int64_t n = r.n;
    const dim3 g((unsigned)r.nv), blk(kBlock);
    const double *qk = w.Q + k * w.ldq;
    if (r.gen) {   // u = A (M^-1 q_k): materialise M^-1 q_k (GMRESSolver.py:107)
        PSK_TRY(prec_apply_dev(r.M, n, qk, w.w, s));
        PSK_TRY(launch_spmv(r.A, kSpmvPlainDot, w.w, w.u, nullptr, w.Q, w.hv, &w.st->done, s));
    } else {
        PSK_TRY(launch_spmv(r.A, r.dinv ? kSpmvJacobiDot : kSpmvPlainDot, qk, w.u, r.dinv, w.Q, w.hv, &w.st->done, s));
    }
    ++r.spmvs;
    // hv[0] = q_0.u (the SpMV's grid sum), hv[j+1] = the dot MGS step j finishes
    double *hcol = w.H + k * r.ld;
    for (int64_t j = 0; j <= k; ++j) {
        const double *qj = w.Q + j * w.ldq;
        const double *qn = j < k ? qj + w.ldq : nullptr;
        GridSum gsj;
        PSK_TRY(gridsum_prepare(r.c, r.nv, 1, w.hv + j + 1, &gsj));
        hipLaunchKernelGGL(gm_mgs_kernel, g, blk, 0, s, n, w.u, qj, qn, w.hv + j, hcol, (int)j, gsj, w.st);
    }
    hipLaunchKernelGGL(gm_normalize_kernel, g, blk, 0, s, n, w.u, w.Q + (k + 1) * w.ldq, w.hv + k + 1, w.H, w.R, w.CS,
                       w.g, r.ld, (int)k, r.it + k, w.st, w.dhist);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// y = solve(R[:kc+1,:kc+1], g[:kc+1]) on the host; x (+)= M^-1 (Q[:, :kc+1] y)   (:159-160)
static int gm_update_x(GmresRun &r, int kc, bool accumulate) {
    GmresWork &w = r.w;
    hipStream_t s = r.s;
    const int64_t n = r.n;
    std::vector<double> hR((size_t)r.ld * r.K), hg((size_t)r.ld), y;
    PSK_HIP(hipMemcpyAsync(hR.data(), w.R, hR.size() * 8, hipMemcpyDeviceToHost, s));
    PSK_HIP(hipMemcpyAsync(hg.data(), w.g, hg.size() * 8, hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    if (!small_solve(kc + 1, hR.data(), r.ld, hg.data(), y))
        return fail(PSK_ERR_ARG, "GMRES least-squares system is singular (LinAlgError in the reference)");
    PSK_HIP(hipMemcpyAsync(w.dy, y.data(), (size_t)(kc + 1) * 8, hipMemcpyHostToDevice, s));
    const dim3 g((unsigned)((n + kBlock - 1) / kBlock)), blk(kBlock);
    const int acc = accumulate ? 1 : 0;
    if (!r.gen) {
        hipLaunchKernelGGL(gm_update_x_kernel, g, blk, 0, s, n, w.Q, w.ldq, w.dy, kc + 1, r.dinv, w.x, acc);
    } else {   // the gemv into w, the preconditioner into tt, then add / copy
        hipLaunchKernelGGL(gm_update_x_kernel, g, blk, 0, s, n, w.Q, w.ldq, w.dy, kc + 1, (const double *)nullptr, w.w, 0);
        PSK_HIP(hipGetLastError());
        PSK_TRY(prec_apply_dev(r.M, n, w.w, w.tt, s));
        hipLaunchKernelGGL(gm_add_or_copy_kernel, g, blk, 0, s, n, w.tt, w.x, acc);
    }
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

// the cycle raised `done` at its step hs.kconv: x, the true residual ||b - A x|| and the result  (:159-174)
static int gm_converged(GmresRun &r, psk_result *res) {
    GmresWork &w = r.w;
    const int kc = r.hs.kconv;
    PSK_TRY(gm_update_x(r, kc, r.it > 0));
    PSK_TRY(launch_spmv(r.A, kSpmvResid, w.x, w.u, nullptr, w.bv, w.pa, nullptr, r.s));
    ++r.spmvs;
    hipLaunchKernelGGL(gm_true_resid_kernel, dim3(1), dim3(kBlock), 0, r.s, w.pa, 1, w.st);
    PSK_HIP(hipGetLastError());
    PSK_TRY(gm_read_state(r));
    const GmresState &hs = r.hs;
    res->iters = r.it + kc + 1;
    res->exit = hs.brk ? PSK_EXIT_ARNOLDI_BREAKDOWN : PSK_EXIT_TOLERANCE;
    res->resid_recursive = hs.rec;
    res->status = PSK_CONVERGED;
    res->success = 1;
    result_true_resid("GMRES", hs.true_resid, hs.tauNormB, r.ctl->tau, hs.rec, true, res);
    return PSK_OK;
}

// a cycle of Kc steps ended without `done`: x from all of them, and the result when that was maxiter (hit_maxiter)
static int gm_cycle_end(GmresRun &r, int64_t Kc, psk_result *res) {
    PSK_TRY(gm_update_x(r, (int)Kc - 1, r.it > 0));
    r.it += Kc;
    if (r.it < r.ctl->maxiter) return PSK_OK;
    // maxiter reached (reference: NameError at :180) -> handleMaxiter(k, x, |g|, ...)
    // without fail_on_maxiter a stop that the tolerance did not make, at the same iteration number
    r.hit_maxiter = true;
    res->resid_recursive = r.hs.rec;
    const int64_t maxiter = r.ctl->maxiter;
    result_outcome({0, r.ctl->fail_on_maxiter ? 0 : 1, 0, maxiter_iters(maxiter), 0, r.hs.rec, nullptr}, maxiter, res);
    return PSK_OK;
}

// behind the last cycle: the checks of the in-launch reductions, loop_ms, norm_b, the b = 0 result, the history, x
static int gm_report(GmresRun &r, psk_result *res, double *hist, double *xout, int32_t loc) {
    const GmresState &hs = r.hs;
    PSK_TRY(solve_finish(r, res));   // the MGS / normalisation / SpMV dots are in-launch reductions
    res->norm_b = hs.normB;
    res->spmv_launches = r.spmvs;
    if (hs.zero_b) result_trivial(res);   // no step ran and res is as the entry point zeroed it (resid = 0)
    // every step reported one residual (reportIter, :155): iters + 1 entries at maxiter (k = maxiter - 1)
    const int64_t nh = hs.zero_b ? 0 : res->iters + (r.hit_maxiter ? 1 : 0);
    return result_copy_out(r, nh, r.w.dhist, r.w.x, res, hist, xout, loc);
}

static int gm_solve(GmresRun &r, const double *b, double *xout, psk_result *res, double *hist, int32_t loc) {
    hipStream_t s = r.s;
    const int64_t maxiter = r.ctl->maxiter;
    int64_t need[2];
    PSK_TRY(gm_workspace(r.A, maxiter, r.ctl->restart, r.gen, true, r.w, need));
    GmresWork &w = r.w;
    PSK_TRY(solve_kit(r.c, false, &r.kit));
    StampPoll poll(r.kit);   // the host-mapped done stamp gm_start_kernel and gm_normalize_kernel write
    PSK_HIP(hipMemsetAsync(w.st, 0, sizeof(GmresState), s));
    // Hessenberg and rotated copies start at zero: entries below the subdiagonal are never written
    // and the least-squares solve reads them (HBar = np.zeros, GMRESSolver.py:80)
    PSK_HIP(hipMemsetAsync(w.H, 0, w.hbytes, s));
    PSK_HIP(hipMemsetAsync(w.R, 0, w.hbytes, s));
    PSK_TRY(to_device_vec(b, loc, r.n, w.bv, s));
    PSK_HIP(hipMemsetAsync(w.x, 0, (size_t)r.n * 8, s));
    PSK_HIP(hipEventRecord(r.kit->ev0, s));
    for (bool first = true;; first = false) {
        PSK_TRY(gm_cycle_start(r, poll, first));
        if (first) {   // the one wait in front of the loop: b = 0 runs no step (:67-68)
            PSK_TRY(gm_read_state(r));
            if (r.hs.zero_b) break;
        }
        const int64_t Kc = maxiter - r.it < r.K ? maxiter - r.it : r.K;
        // Step numbers and stamps count from the cycle's start. A stamp ends the solve, so none is left over from an
        // earlier cycle, and the stream is drained between cycles: step k is not enqueued iff `done` was raised at
        // a step <= k - 3 of this cycle.
        int64_t steps = 0;   // not needed: the state says where the cycle ended
        PSK_TRY(poll_loop<2>(poll, r, Kc, &steps, [&](int64_t k) { return gm_step(r, k); }));
        PSK_TRY(gm_read_state(r));
        if (r.hs.done) {
            PSK_TRY(gm_converged(r, res));
            break;
        }
        PSK_TRY(gm_cycle_end(r, Kc, res));
        if (r.hit_maxiter) break;
    }
    return gm_report(r, res, hist, xout, loc);
}

}  // namespace psk

using namespace psk;

extern "C" int psk_gmres(const psk_csr *Ac, const psk_prec *M, const double *b, double *xout,
                         const psk_ctl *ctl, psk_result *res, double *hist, int32_t loc) {
    // restart is this entry point's own argument; its refusal names both, so it is made here for both
    if (ctl && (ctl->maxiter < 0 || ctl->restart < 0)) return fail(PSK_ERR_ARG, "psk_gmres: negative maxiter/restart");
    GmresRun r{};
    return solve_entry("psk_gmres", "GMRES", r, Ac, M, b, xout, ctl, res, 1, kVecTile, [&]() -> int {
        r.K = gm_basis(ctl->maxiter, ctl->restart);
        r.ld = (int)(r.K + 1);
        r.gv = grid_for_rows(r.c, r.n, kVecTile);
        r.C = 1;
        PSK_TRY(gm_fits_hbm(r));
        if (r.n == 0) {   // no rows: b = 0
            result_trivial(res);
            return PSK_OK;
        }
        return gm_solve(r, b, xout, res, hist, loc);
    });
}
