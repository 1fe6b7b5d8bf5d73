/*
 * psk.h — C ABI of libpsk.so, the MI355X (gfx950) Krylov engine behind
 * pysolvers_amd.Linear (a drop-in for krlong014/PySolvers' PySolvers/Linear).
 *
 * Plain C: pointers, sizes and PODs only; no torch/HIP types cross this line.
 * Every entry point returns PSK_OK (0) or a negative PSK_ERR_* code; the text
 * of the last error of the calling thread is available from psk_last_error().
 * NUMERICAL failure (breakdown, maxiter, GMRES true-residual miss) is NOT an
 * error: it is reported in psk_result.status exactly as the reference reports
 * it through SolveStatus(success=False, ...) (IterativeSolver.py:101-129).
 *
 * Reference interfaces each group replaces (paths relative to the reference root):
 *   psk_csr_*        scipy.sparse CSR handed to LinearSolver.solve(A, b)
 *                    (LinearSolver.py:30-33) — uploaded once, kept in HBM.
 *   psk_spmv         mvmult(A, x)                 IterativeLinearSolver.py:94-106
 *   psk_dot/nrm2     np.dot / IterativeSolver.norm (npla.norm)  IterativeSolver.py:86-88
 *   psk_axpy         x + alpha*p style updates    PCGSolver.py:121-122,138
 *   psk_prec_*       PreconditionerType.form(A) -> applyRight(vec)
 *                    PreconditionerType.py:4-19, Preconditioner.py:3-68;
 *                    JACOBI = DInv*v with DInv = reciprocal(diag(A)) (ClassicSmoothers.py:8,14)
 *   psk_pcg          PCGSolver.solve              PCGSolver.py:64-142
 *   psk_gmres        GMRESSolver.solve            GMRESSolver.py:55-180 (restart==0)
 *   psk_comm_*, psk_csr_create_fd2d_dist: row-block sharding across GPUs (RCCL over
 *                    xGMI); no reference counterpart (the reference is single-process).
 *   psk_csr_create_fd2d: examples/FDLaplacian2D.py:5-23 generated on the device,
 *                    bit-identical arrays and entry order.
 *   psk_prec_create_trisolve  RightIC applyRight (ICPreconditioner.py:58-63), Gauss-Seidel
 *                    smoother U^-1 (ClassicSmoothers.py:28-36), coarse SuperLU solve
 *                    (VCycleManager.py:34-37): one sync-free triangular-solve chain.
 *   psk_prec_create_amg  AMGPreconditioner.apply (AMGPreconditioner.py:46-51) ->
 *                    AMGVCycleSolver.solve (VCycleSolver.py:52-95) -> VCycleManager.runLevel
 *                    (VCycleManager.py:31-62), hierarchy built on the host.
 *   psk_vcycle       AMGVCycleSolver.solve as a solver of its own (VCycleSolver.py:52-95): the
 *                    cycles of a psk_prec_create_amg hierarchy with the loop, the stopping test and
 *                    the history on the device.
 *   psk_mm_*         scipy.io.mmread(path).tocsr() (examples/DHTestProblem.py:27-28).
 *   psk_sa_aggregate BuildAggregates + BuildFilteredMatrix (SmoothedAggregation.py:57-183),
 *                    O(nnz) host code.
 *   psk_csr_matmat, psk_csr_transpose, psk_sa_prolongator: the scipy products, transpose and numpy
 *                    smoothing lines of the AMG setup (SmoothedAggregation.py:185-205,
 *                    MLHierarchy.py:283-322) on the device, same bits in the same stored order.
 *   psk_csr_ilu0, psk_prec_create_ilu0: ILU(0) factored on the device; no reference counterpart (the
 *                    reference's incomplete factors are SuperLU's).
 *   psk_csr_iluk_pattern, psk_prec_create_iluk: level-of-fill ILU(k), the fill pattern built on the device; no
 *                    reference counterpart.
 *   psk_prec_trisolve_sweeps: opt-in approximate triangular applies by Jacobi sweeps; no reference counterpart.
 *   psk_pcg_multi    several right-hand sides in one PCG loop, each column the recurrence of psk_pcg; no reference
 *                    counterpart (the reference solves one vector per call).
 *   psk_csr_fsai, psk_prec_create_fsai: factorized sparse approximate inverse G ~ L^-1 formed on the device and
 *                    applied as two SpMVs; no reference counterpart.
 *   psk_color_plan, psk_prec_create_mcgs: Gauss-Seidel in a colour ordering, one streaming launch per colour; no
 *                    reference counterpart (the reference's Gauss-Seidel smoother is spsolve(triu(A), .)).
 */
#ifndef PSK_H
#define PSK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSK_ABI_VERSION 4

/* return codes */
#define PSK_OK               0
#define PSK_ERR_ARG         -1   /* bad argument (AssertionError in the reference, PCGSolver.py:79-83) */
#define PSK_ERR_HIP         -2
#define PSK_ERR_RCCL        -3
#define PSK_ERR_ALLOC       -4
#define PSK_ERR_UNSUPPORTED -5

/* psk_result.status */
#define PSK_CONVERGED        0   /* handleConvergence            IterativeSolver.py:101-107 */
#define PSK_MAXITER          1   /* handleMaxiter                IterativeSolver.py:115-129 */
#define PSK_BREAKDOWN        2   /* handleBreakdown              IterativeSolver.py:109-113 */
#define PSK_TRUE_RESID_FAIL  3   /* GMRES true residual missed   GMRESSolver.py:167-174 */

/* psk_result.exit: why the iteration loop stopped (gates the host-side checks a caller-supplied
   norm needs, e.g. the GMRES true-residual test GMRESSolver.py:163-174, without inferring it from
   the history length) */
#define PSK_EXIT_NONE             0   /* no loop ran (b = 0: IterativeSolver.py:86-88 / GMRESSolver.py:67-68) */
#define PSK_EXIT_TOLERANCE        1   /* recursive residual <= tau*||b||  PCGSolver.py:129, GMRESSolver.py:158 */
#define PSK_EXIT_ARNOLDI_BREAKDOWN 2  /* GMRES: h_{k+1,k} <= 1e-16 ||h_k|| (counts as convergence, :122,:158) */
#define PSK_EXIT_MAXITER          3   /* maxiter reached (k == maxiter-1 with !failOnMaxiter for PCG, :130) */
#define PSK_EXIT_DOT_BREAKDOWN    4   /* PCG dot(u,r) == 0 or dot(p,Ap) == 0  :104-105, :114-115 */

/* where the vector pointers of a call live */
#define PSK_HOST   0
#define PSK_DEVICE 1

/* preconditioner kinds */
#define PSK_PREC_IDENTITY 0      /* IdentityPreconditionerType   PreconditionerType.py:13-19 */
#define PSK_PREC_JACOBI   1      /* DInv*v                        ClassicSmoothers.py:5-16 pattern */
#define PSK_PREC_ILU      2      /* triangular-solve chain: SuperLU ILU.solve ILUTPreconditioner.py:70-78,
                                    IC, Gauss-Seidel, coarse LU (psk_prec_create_trisolve) */
#define PSK_PREC_AMG      3      /* smoothed-aggregation V-cycles  AMGPreconditioner.py:46-51 */
#define PSK_PREC_DENSE    4      /* x = A^-1 f by a dense inverse: the AMG coarse solve spsolve(A_c, f),
                                    VCycleManager.py:34-37 (psk_prec_create_dense_inverse) */
#define PSK_PREC_CHEBYSHEV 5     /* Chebyshev polynomial in D^-1 A (psk_prec_create_chebyshev); no reference
                                    counterpart (the reference's smoothers are Jacobi and Gauss-Seidel) */

typedef struct psk_csr  psk_csr;    /* device CSR (int32 rowptr/colidx, f64 vals), library-owned */
typedef struct psk_prec psk_prec;   /* formed preconditioner, library-owned */
typedef struct psk_comm psk_comm;   /* RCCL communicator + rank geometry */

/* CommonSolverArgs (IterativeSolver.py:42-57) minus the print knobs. */
typedef struct psk_ctl {
    int64_t maxiter;          /* CommonSolverArgs.maxiter */
    double  tau;              /* relative residual tolerance */
    int32_t fail_on_maxiter;  /* CommonSolverArgs.failOnMaxiter */
    int32_t restart;          /* GMRES only: 0 = reference non-restarted (Krylov dim = maxiter) */
    int32_t check_every;      /* host polls the device status every N iterations; 0 = auto */
    int32_t time_kernels;     /* S > 0: HIP-event timing of every S-th SpMV launch (iterations k with
                                 k % S == 0; psk_result.spmv_ms); 0 = off */
    double  norm_b;           /* GMRES: > 0 = ||b|| in the caller's norm (CommonSolverArgs.norm,
                                 GMRESSolver.py:66) for the threshold tau*||b|| and psk_result.norm_b;
                                 0 = the device 2-norm. PCG ignores it (a non-2-norm PCG is driven by
                                 the host, IterativeSolver.py:86-88). Zero-initialise. */
} psk_ctl;

typedef struct psk_result {
    int32_t status;           /* PSK_CONVERGED / MAXITER / BREAKDOWN / TRUE_RESID_FAIL */
    int32_t success;          /* SolveStatus.success() */
    int64_t iters;            /* SolveStatus.iters() (reference conventions, incl. k on maxiter) */
    double  resid;            /* SolveStatus.resid(): PCG recursive ||r||; GMRES true ||b-Ax|| */
    double  resid_recursive;  /* last recursive residual estimate */
    double  norm_b;           /* ||b|| */
    double  loop_ms;          /* device wall time of the solve (HIP events) */
    double  spmv_ms;          /* mean duration of the timed SpMV launches when ctl.time_kernels */
    int64_t spmv_launches;    /* number of SpMV launches (the timed ones when ctl.time_kernels) */
    int64_t hist_len;         /* valid entries written to hist */
    char    msg[256];         /* SolveStatus.msg() */
    int32_t exit;             /* PSK_EXIT_* (ABI 3) */
    int32_t reserved;
    /* ABI 4, sharded PCG with ctl.time_kernels: the iterations whose SpMV is timed also time, on this rank,
     * the scalar exchange after that SpMV (p.Ap: the mailbox gather kernel — its duration is the wait for the
     * slowest rank plus the transport — or the RCCL all-gather) and the halo exchange of p that feeds the
     * next SpMV (pack + send/recv, on the stream that runs it: the second stream when overlapped with K3).
     * Means over the samples; 0 when unsharded or untimed. */
    double  gather_ms;
    double  halo_ms;
    int64_t comm_samples;
} psk_result;

/* ---- library / device ---------------------------------------------------------------- */
int         psk_abi_version(void);
const char *psk_last_error(void);
int         psk_device_count(int32_t *n);
int         psk_set_device(int32_t dev);
int         psk_synchronize(void);
/* Drain every device stream and release the library's process-lifetime resources (streams, events,
 * host-mapped words, reduction arrays) while the HIP runtime is alive; call once at process exit
 * (the Python binding registers it with atexit). Afterwards entry points that need a device return
 * PSK_ERR_ARG and psk_csr_destroy / psk_prec_destroy / psk_dfree are no-ops. No reference
 * counterpart (process teardown). */
int         psk_shutdown(void);
/* psk_shutdown with options. PSK_SHUTDOWN_RESET_DEVICE: afterwards hipDeviceReset() every device the
 * library used, releasing the HIP runtime's own per-device state (e.g. its cooperative-launch queue) while
 * HSA is alive; only for a process in which libpsk is the only HIP user (the Python binding passes it
 * when torch was never imported) and skipped while an RCCL communicator is alive. No reference
 * counterpart (process teardown). */
#define PSK_SHUTDOWN_RESET_DEVICE 1
int         psk_shutdown_ex(int32_t flags);
/* device memory helpers (so a host binding can keep vectors resident in HBM) */
int psk_dmalloc(int64_t bytes, void **dptr);
int psk_dfree(void *dptr);
int psk_h2d(void *dst, const void *src, int64_t bytes);
int psk_d2h(void *dst, const void *src, int64_t bytes);
int psk_dmemset0(void *dst, int64_t bytes);

/* ---- CSR matrices ---------------------------------------------------------------------- */
/* Copy a CSR matrix (rowptr[n+1], colidx[nnz], vals[nnz]; stored entry order is kept,
 * sorted or not) into HBM. loc says where the three arrays live. int32 indices:
 * nnz <= 2^31 - 1 - 1536 (PSK_ERR_UNSUPPORTED beyond; FD 16384^2 has 1.34e9). */
int psk_csr_create(int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                   const double *vals, int32_t loc, psk_csr **out);
/* FDLaplacian2D(a, b, m) generated on the device (examples/FDLaplacian2D.py:5-23). */
int psk_csr_create_fd2d(double a, double b, int64_t m, psk_csr **out);
/* Rectangular nrows x ncols CSR (AMG prolongators / restrictions, MLHierarchy.py:283-292). */
int psk_csr_create_rect(int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                        const double *vals, int32_t loc, psk_csr **out);
int psk_csr_info(const psk_csr *A, int64_t *n, int64_t *nnz);
/* SpMV storage layout of A (same y bit for bit either way; the CSR arrays are always kept):
 *   PSK_LAYOUT_CSR          one workgroup per tile of rows, the tile's entries streamed in stored
 *                           order and the products staged through LDS;
 *   PSK_LAYOUT_SLICED       a sliced copy: 256-row slices, slot-major inside a slice, one row per
 *                           lane, padding slots up to the slice's widest row, values in slot pairs
 *                           (16-B loads); a slice whose columns all lie within +-32767 of their rows
 *                           stores 16-bit column deltas two to a 32-bit word, any other slice 32-bit
 *                           columns;
 *   PSK_LAYOUT_SLICED_WIDE  the same with 32-bit columns in every slice;
 *   PSK_LAYOUT_SLICED_DICT  SLICED with the values replaced by one-byte indices into a dictionary of
 *                           the matrix's distinct values (at most 8 bit patterns: stencils, graph
 *                           Laplacians), 3 B per slot with 16-bit columns;
 *   PSK_LAYOUT_DIAG         (round 5) diagonal storage: every row's entries lie, in stored order, on
 *                           a subsequence of K <= 8 diagonals c = row + d_j (a row-block shard's
 *                           outside columns mapped to its halo) and all entries of a diagonal hold
 *                           one value (constant-coefficient stencils such as FDLaplacian2D); the
 *                           offsets and values are kernel arguments, one presence byte per row.
 * Every creation path picks DIAG when the matrix has one, else SLICED_DICT (values permitting) or
 * SLICED when its stream is no larger than the CSR stream (12 B/entry + 4 B/row); env
 * PSK_SPMV_LAYOUT=csr|sliced|sliced_wide|sliced_dict|diag overrides (sliced: no dictionary),
 * PSK_SPMV_DIAG=0 leaves DIAG out of the automatic choice. Forcing SLICED_DICT on a matrix with more
 * than 8 distinct values, or DIAG on one without the diagonal structure, fails with
 * PSK_ERR_UNSUPPORTED. set = -1 queries, a PSK_LAYOUT_*
 * value switches (building or freeing the copy). Out: *slots = padded slots of the sliced copy (0
 * without one; DIAG: n K), *packed_slots = those in 16-bit slices, *stream_bytes = matrix bytes one
 * SpMV streams in the current layout (CSR: 12 nnz + 4 (n+1); DIAG: n). Out pointers may be NULL. Replaces
 * nothing in the reference (scipy keeps CSR): a device storage choice under mvmult
 * (IterativeLinearSolver.py:94-106). */
#define PSK_LAYOUT_CSR         0
#define PSK_LAYOUT_SLICED      1
#define PSK_LAYOUT_SLICED_WIDE 2
#define PSK_LAYOUT_SLICED_DICT 3
#define PSK_LAYOUT_DIAG        4
int psk_csr_layout(psk_csr *A, int32_t set, int32_t *layout, int64_t *slots, int64_t *packed_slots,
                   int64_t *stream_bytes);
/* Copy the arrays back to host buffers (any pointer may be NULL). */
int psk_csr_download(const psk_csr *A, int32_t *rowptr, int32_t *colidx, double *vals);
int psk_csr_destroy(psk_csr *A);

/* ---- kernels on the hot path ------------------------------------------------------------ */
/* y = A x, per-row stored-order sum from 0.0, product rounded before the add:
 * bit-identical to scipy csr_matvec. For a distributed matrix x is the local
 * [owned | halo] vector and the halo is refreshed first (collective). */
int psk_spmv(const psk_csr *A, const double *x, double *y, int32_t loc);
/* Measurement: `reps` back-to-back y = A x launches (device pointers) between two HIP events on
 * the library stream; *avg_ms = elapsed / reps (one untimed warm-up launch first). */
int psk_spmv_timed(const psk_csr *A, const double *x, double *y, int32_t reps, double *avg_ms);
int psk_dot(int64_t n, const double *x, const double *y, int32_t loc, double *out);
int psk_nrm2(int64_t n, const double *x, int32_t loc, double *out);
/* y = y + alpha*x (two roundings, as numpy's y + alpha*x) */
int psk_axpy(int64_t n, double alpha, const double *x, double *y, int32_t loc);

/* ---- preconditioners (PreconditionerType.form / applyRight) ---------------------------- */
int psk_prec_create(const psk_csr *A, int32_t kind, psk_prec **out);
/* ILU from host factors of SuperLU spilu (RightILUTPreconditioner, ILUTPreconditioner.py:51-53):
 * L (unit lower, diagonal optional) and U (upper with diagonal) as CSR, perm_r / perm_c as in
 * scipy's SuperLU (Pr A Pc = L U). apply(v) = (U^-1 L^-1 (v scattered by perm_r))[perm_c]. */
int psk_prec_create_ilu(int64_t n, const int32_t *l_rowptr, const int32_t *l_colidx, const double *l_vals,
                        const int32_t *u_rowptr, const int32_t *u_colidx, const double *u_vals,
                        const int32_t *perm_r, const int32_t *perm_c, psk_prec **out);
/* General triangular-solve chain on the device (host CSR arrays, copied):
 *   bb[j] = v[gather_in[j]]          (gather_in NULL: bb = v)
 *   y = L^-1 bb                      (L lower; l_unit: unit diagonal, stored diagonal entries ignored;
 *                                     else the stored diagonal divides; L NULL: y = bb)
 *   z = U^-1 y                       (U upper; same rules with u_unit; U NULL: z = y)
 *   out[i] = z[gather_out[i]]        (gather_out NULL: out = z)
 * Row i's off-diagonal products are accumulated in stored order with FMA, then one wave sum. */
int psk_prec_create_trisolve(int64_t n, const int32_t *l_rowptr, const int32_t *l_colidx, const double *l_vals,
                             int32_t l_unit, const int32_t *u_rowptr, const int32_t *u_colidx,
                             const double *u_vals, int32_t u_unit, const int32_t *gather_in,
                             const int32_t *gather_out, psk_prec **out);
/* Direct solve x = A^-1 f through the explicit inverse, formed once on the device (rocSOLVER getrf +
 * getri, loaded at first use) and applied as one streamed GEMV per solve, with `refine` (0..4) steps of
 * x <- x + A^-1 (f - A x) after it. Replaces spsolve(A_c, f) for the AMG coarse level
 * (VCycleManager.py:34-37; pass it as psk_prec_create_amg's `coarse`). A is BORROWED (refinement).
 * PSK_ERR_UNSUPPORTED when n > 32768 (8.6 GB) or rocSOLVER cannot be loaded, PSK_ERR_ARG when A is
 * singular. The input vector of an apply must be 16-byte aligned. */
int psk_prec_create_dense_inverse(const psk_csr *A, int32_t refine, psk_prec **out);
/* Chebyshev polynomial preconditioner / smoother of `degree` >= 1 in D^-1 A, D = diag(A) (the Jacobi DInv),
 * for the eigenvalues of D^-1 A in [lmax/ratio, lmax]; f64, every operation rounded as written:
 *   lmin = lmax/ratio, theta = (lmax+lmin)/2, delta = (lmax-lmin)/2, sigma = theta/delta, rho_0 = 1/sigma,
 *   c0 = 1/theta; for k = 1..degree-1: rho_k = 1/(2 sigma - rho_{k-1}), alpha_k = rho_k rho_{k-1},
 *   beta_k = 2 rho_k/delta (host doubles);
 *   apply z = M^-1 v: d = c0 (DInv v), z = d; then for k = 1..degree-1, ONE launch each:
 *   d = alpha_k d + beta_k (DInv (v - A z)), z = z + d, the row sums of A z as psk_spmv forms them.
 * degree 1 is Jacobi scaled by c0. lmax <= 0 selects the Gershgorin bound max_i (sum_j |a_ij|) |DInv_i| (row sums
 * in stored order), a true upper bound, so the operator is definite for a definite A; ratio > 1 (30 is customary
 * for a smoother). Symmetric for symmetric A: usable by PCG, by GMRES and as an AMG smoother
 * (psk_prec_create_amg). Each step streams A once (CSR arrays), has no dependency chain and no grid sum.
 * A is BORROWED. PSK_ERR_ARG: degree < 1, ratio <= 1, A not square or empty, a diagonal entry that is zero,
 * missing or not finite; PSK_ERR_UNSUPPORTED: a sharded A. Replaces nothing in the reference. */
int psk_prec_create_chebyshev(const psk_csr *A, int32_t degree, double lmax, double ratio, psk_prec **out);
/* The formed polynomial: coeffs (nullable) receives 2*degree-1 doubles, c0 then the (alpha_k, beta_k) pairs of
 * k = 1..degree-1. Any out pointer may be NULL. PSK_ERR_ARG when M is not a PSK_PREC_CHEBYSHEV. */
int psk_prec_chebyshev_info(const psk_prec *M, int32_t *degree, double *lmax, double *lmin, double *coeffs);
/* Smoothed-aggregation AMG preconditioner over a host-built hierarchy (levels 0 = coarsest ..
 * num_levels-1 = finest, MLHierarchy.py:250-258). Arrays of num_levels handles, all BORROWED
 * (they must outlive the preconditioner): A[k] level matrices (A[num_levels-1] = the fine A),
 * P[k] (n_{k+1} x n_k) and R[k] (n_k x n_{k+1}) for k < num_levels-1, smoother[k] for k >= 1
 * (any preconditioner S: one sweep is x <- x + S^-1 (f - A x): PSK_PREC_ILU upper solve with
 * triu(A_k) = Gauss-Seidel, PSK_PREC_JACOBI = Jacobi; ClassicSmoothers.py:5-36; PSK_PREC_CHEBYSHEV), coarse = the
 * level-0 direct solve. apply(v): x = v; num_iters V-cycles, stopping after the first cycle whose
 * ||v - A x|| < tau ||v|| (VCycleSolver.py:119-146). */
int psk_prec_create_amg(int32_t num_levels, psk_csr *const *A, psk_csr *const *P, psk_csr *const *R,
                        psk_prec *const *smoother, psk_prec *coarse, int32_t num_iters, int32_t nu_pre,
                        int32_t nu_post, double tau, psk_prec **out);
/* Schedule of factor `which` (0 = L, 1 = U) of a triangular-solve chain: 0 = sync-free (one wave per
 * row, global dependency levels), 1 = band (one workgroup per block of the solve order, local levels
 * behind barriers, LDS ring of ring_words doubles), 2 = LDS (factors of at most 18432 rows: one
 * workgroup, sync-free inside it with x in LDS), 3 = grid (2-D stencil factors: one wave per band of
 * 64 lines advancing along a skewed coordinate), 4 = part (rows cut into strips of their natural
 * index, one workgroup per CU, in-strip dependencies through LDS; its layout is built when chosen or
 * when PSK_TRISOLVE_PART=1 at creation), 5 = levels (round 5: ONE workgroup, a dependency level per step
 * behind a barrier, x in an LDS ring; for factors with narrow levels and dependencies a bounded number of
 * solve positions back; built when chosen or when PSK_TRISOLVE_LEVELS=1 at creation). The library picks the fastest by host cost models
 * (est_*_us); set = 0..5 forces one (PSK_ERR_UNSUPPORTED when the factor has no such layout), -1 only
 * queries. Any out pointer may be NULL. */
int psk_prec_trisolve_schedule(psk_prec *M, int32_t which, int32_t set, int32_t *schedule, int64_t *blocks,
                               int32_t *ring_words, double *est_syncfree_us, double *est_band_us);
/* Grid-schedule shape of factor `which` (0 = L, 1 = U): out[0..6] = line width w, lines H, twice the
 * skew sigma2 and its phase (a solve-order position y*w + x - off runs at step x + ((sigma2*y + phase)
 * >> 1)), leading empty positions off, steps per 64-line band, dictionary records (0 = per-step
 * records). PSK_ERR_UNSUPPORTED when the factor is not a 2-D stencil. No compute (diagnostics, tests). */
int psk_prec_trisolve_grid_info(const psk_prec *M, int32_t which, int64_t *out);
/* Approximate solves of factor `which` (0 = L, 1 = U) of a triangular-solve chain by Jacobi sweeps.
 * set >= 1: that many sweeps replace the factor's schedule in every later apply; set = 0: back to the exact
 * schedule (psk_prec_trisolve_schedule's, untouched by this call); set = -1: query only. *sweeps (nullable)
 * receives the value in force. Never chosen by the library itself.
 *
 * Arithmetic (all f64). The factor T is split into its off-diagonal entries N and its diagonal d; a unit factor
 * has d = 1, its stored diagonal is ignored and nothing is divided. With b = rhs[rhs_idx] and s sweeps:
 *     x(0)_i = b_i / d_i
 *     x(j)_i = (b_i - sum_k N_ik x(j-1)_k) / d_i      j = 1..s        (IEEE division)
 *     x      = x(s)
 * A row's sum is formed by G = 1, 4, 16 or 64 lanes (chosen per factor from its mean off-diagonal row length:
 * <= 2, <= 8, <= 32, more; PSK_TRISWEEP_WIDTH=1|4|16|64 in the environment when sweeps are set overrides it, for
 * tests): lane t accumulates the row's entries t, t + G, ... in stored order with fma from 0.0, and the G lane
 * sums are added in one fixed tree; b_i - sum and the division round separately. Every row of sweep j reads only
 * x(j-1), never a value its own launch wrote (pure Jacobi on two alternating buffers), so the result is the same
 * bits run after run. There is no dependency chain and no wait: one launch for x(0) and one per sweep on the apply's
 * stream, nothing else synchronises. N is nilpotent: levels - 1 sweeps (psk_prec_info) give the exact solve up to
 * the summation order. With a fixed s the apply is a fixed linear operator (GMRES, BiCGStab and PCG may use it;
 * for a symmetric A the ILU(0) chain with equal counts stays symmetric).
 *
 * The first set >= 1 on a chain allocates two more n-vectors, freed by psk_prec_destroy. PSK_ERR_ARG when M is
 * NULL or not a PSK_PREC_ILU, which is not 0 or 1, the factor is absent, set < -1 or set > 65536; PSK_ERR_ALLOC
 * when the vectors cannot be allocated. On any error nothing changes. An AMG Gauss-Seidel smoother chain in
 * sweep mode is honoured (the paired-sweep kernel steps aside). */
int psk_prec_trisolve_sweeps(psk_prec *M, int32_t which, int32_t set, int32_t *sweeps);
/* Host-only: the grid plan psk_prec_create_trisolve would make for one triangular factor (CSR with its
 * diagonal; upper = 1: solved from the last row up), without any device work — out[0..6] = w, H,
 * sigma2, phase, off, steps per band, record width K. PSK_ERR_UNSUPPORTED when it is not a 2-D stencil. */
int psk_trisolve_grid_plan(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                           int32_t upper, int64_t *out);
/* kind, size and triangular-solve shape of a preconditioner (any out pointer may be NULL). */
int psk_prec_info(const psk_prec *M, int32_t *kind, int64_t *n, int64_t *nnz_l, int64_t *nnz_u,
                  int64_t *levels_l, int64_t *levels_u);
/* Jacobi: *uniform = 1 when every DInv entry is the same double (*value; constant-diagonal matrices
 * such as stencils), in which case psk_pcg reads that scalar instead of streaming DInv (same
 * products bit for bit, 16 B per row and iteration less). PSK_JACOBI_UNIFORM=0 at creation disables. */
int psk_prec_jacobi_uniform(const psk_prec *M, int32_t *uniform, double *value);
int psk_prec_apply(const psk_prec *M, int64_t n, const double *v, double *out, int32_t loc);
int psk_prec_destroy(psk_prec *M);

/* ---- MatrixMarket input (host only, except psk_csr_create_mm) --------------------------------- */
/* scipy.io.mmread(path).tocsr() (examples/DHTestProblem.py:27-28) for coordinate files:
 * real/integer/pattern, general/symmetric/skew-symmetric; symmetric files expanded, rows sorted by
 * column, duplicates summed, explicit zeros kept. psk_mm_info gives the sizes (nnz_max = entries,
 * doubled for symmetric files) so the caller can allocate rowptr[nrows+1], colidx/vals[nnz_max];
 * psk_mm_read fills them and returns the actual nnz. */
int psk_mm_info(const char *path, int64_t *nrows, int64_t *ncols, int64_t *nnz_max);
int psk_mm_read(const char *path, int32_t *rowptr, int32_t *colidx, double *vals, int64_t *nnz);
int psk_csr_create_mm(const char *path, psk_csr **out);

/* ---- AMG setup (host only, no GPU needed) --------------------------------------------------- */
/* Smoothed-aggregation coarsening of one level, SmoothedAggregation.py:41-183 in O(nnz):
 * agg[i] = aggregate of node i (the reference's list order: isolated nodes, then phase-1
 * aggregates; phase 2 by strongest |A[i,k]|), *count = number of aggregates, and af_vals =
 * the values of the filtered matrix A_f (same structure as A; entries outside N_i lumped onto
 * the diagonal in stored order, including the neighbourhood growth the reference's set aliasing
 * causes). tol is the strength threshold (0.08 * 0.5^(lvl-1) by default). */
int psk_sa_aggregate(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, double tol,
                     int32_t *agg, int64_t *count, double *af_vals);

/* ---- sparse operator construction on the device (spgemm.hip) --------------------------------- */
/* C = A B for an (m x k) A and a (k x n) B, both on the device: scipy's csr_matmat (`A @ B`), bit for bit and in
 * its stored entry order. For output row i enumerate the products t = 0, 1, ...: the entries jj of A's row i in
 * stored order and, for each, the entries kk of B's row A.col[jj] in stored order; product t is the rounded
 * A.val[jj] * B.val[kk] (a separate multiply and add, no FMA) on column B.col[kk]; a column's value is
 * ((0.0 + p_a) + p_b) + ... over its products in ascending t; the columns are emitted in DESCENDING order of their
 * first t and a column whose sum == 0.0 is dropped. Duplicate columns inside a row of A or B, unsorted rows,
 * explicit zeros and empty rows need no special case. The result ends like psk_csr_create(..., PSK_DEVICE) (the
 * SpMV layout choice applies) and may be rectangular. PSK_ERR_ARG: inner dimensions differ. PSK_ERR_UNSUPPORTED:
 * a sharded operand, a result over the int32 nnz limit, or a row with more than PSK_SPGEMM_ROW_CAP products.
 * *C is written only on success. The result does not depend on the launch geometry. */
#define PSK_SPGEMM_ROW_CAP 1024
int psk_csr_matmat(const psk_csr *A, const psk_csr *B, psk_csr **C);
/* A.transpose().tocsr() on the device: row j of the result holds A's entries of column j in ascending source
 * row and, within one source row, in stored order (duplicates kept; deterministic). PSK_ERR_UNSUPPORTED: a
 * sharded operand. */
int psk_csr_transpose(const psk_csr *A, psk_csr **At);
/* SA_coarsen's lines after the aggregation (SmoothedAggregation.py:185-229) from psk_sa_aggregate's outputs:
 * P = S Phat with S on A's structure, s = omega * af_vals[e], v = s / d[row], S[e] = col == row ? 1 - v : -v
 * (every operation rounded once, IEEE division), d[row] = the sum of the row's stored diagonal entries in
 * stored order from 0.0 (scipy's diagonal()), Phat's row i = the single entry (agg[i], 1.0), n x count, and the
 * product as psk_csr_matmat. agg[n] and af_vals[nnz] live where loc says. PSK_ERR_ARG: A not square, an
 * aggregate outside [0, count) (checked for PSK_HOST). */
int psk_sa_prolongator(const psk_csr *A, const int32_t *agg, int64_t count, const double *af_vals, double omega,
                       int32_t loc, psk_csr **P);

/* ---- ILU(0) on the device (ilu0.hip) ----------------------------------------------------------- */
/* F = the ILU(0) factors of a square A on the device, in one matrix with A's pattern and its rows in ascending
 * column order. A has at most one stored entry per (row, column) and a stored diagonal entry in every row; its rows
 * may be stored in any order (they are sorted into the working copy first). With v = the values of that copy, for
 * i = 0 .. n-1: for each entry e of row i with column k < i, in ascending k: l = v[e] / v[diag(k)] (IEEE division;
 * row k is final by then), v[e] = l, and for each entry f of row k with column j > k, in ascending j, if row i stores
 * column j at q: v[q] = v[q] - l * v[f] (the product rounded, then the difference: no FMA); then row i's pivot
 * v[diag(i)] is in error when it is 0.0 or not finite. L = strict-lower(F) with a unit diagonal, U = upper(F) with
 * the diagonal. The numeric phase runs one launch per dependency level of strict-lower(A) (the levels by the host
 * planner of the triangular solves, from the downloaded pattern); every value receives its updates in ascending k,
 * so the result does not depend on the launch geometry. The result ends like psk_csr_create(..., PSK_DEVICE) and
 * psk_csr_download reads it back. PSK_ERR_ARG: A not square or empty, a column outside [0, n), a row without a
 * stored diagonal entry, a zero or non-finite pivot (psk_last_error names the smallest such row).
 * PSK_ERR_UNSUPPORTED: a sharded A, a duplicate column within a row. *F is written only on success. A is only
 * read; nothing of it is borrowed. Replaces nothing in the reference (its incomplete factors are SuperLU's,
 * ILUTPreconditioner.py:51-53). */
int psk_csr_ilu0(const psk_csr *A, psk_csr **F);
/* The ILU(0) preconditioner of A: psk_csr_ilu0, then the factors downloaded once, split into L (unit) and U and
 * handed to the triangular-solve chain exactly as psk_prec_create_trisolve(n, L, l_unit = 1, U, u_unit = 0, no
 * gathers) takes host factors (copied; the planner picks each factor's schedule). The result is a PSK_PREC_ILU:
 * psk_prec_apply, psk_prec_info, psk_prec_trisolve_schedule and the solvers take it like any other. Errors as
 * psk_csr_ilu0; A is not borrowed. Replaces nothing in the reference. */
int psk_prec_create_ilu0(const psk_csr *A, psk_prec **out);

/* ---- level-of-fill ILU(k) on the device (iluk.hip) --------------------------------------------- */
/* The ILU(k) pattern of a square A, built on the device. A has at most one stored entry per (row, column) and a
 * stored diagonal entry in every row; its rows may be stored in any order; 0 <= k <= PSK_ILUK_MAX_LEVEL. With S = the
 * copy of A whose rows are in ascending column order:
 *   Levels. Every stored entry of A has level 0, explicit zeros included. Then, for i = 0 .. n-1: for each entry
 *   (i, c) of row i with c < i, in ascending c (fill entries included as this same pass adds them), and for every entry
 *   (c, j) of the finished row c with j > c: cand = lev(i,c) + lev(c,j) + 1; if cand <= k and (i, j) is absent or holds
 *   a larger level, lev(i,j) = cand.
 *   Pattern. Every entry with lev <= k.
 * *P has that pattern with rows in ascending column order; it holds A's value where A stores the entry and +0.0 at
 * a fill entry. *Lev (NULL: not wanted) has the same structure and the levels as doubles. Both end like
 * psk_csr_create(..., PSK_DEVICE). The ILU(k) factor of A is, bit for bit, psk_csr_ilu0(*P) in the arithmetic stated
 * above for psk_csr_ilu0; k = 0 gives S itself and therefore the bits of psk_csr_ilu0(A). The device algorithm
 * (k rounds, each parallel over the rows; iluk.hip) gives exactly the pattern and levels of this sequential rule
 * and does not depend on the launch geometry.
 * PSK_ILUK_ROW_CAP = 512 is the longest row of *P the kernels hold (a row's new columns are collected in a hash set
 * in LDS: 24 KiB per workgroup at this cap, six workgroups per CU; 1024 would halve that). The cap holds for k >= 1;
 * k = 0 runs no round and takes rows of any length, as psk_csr_ilu0 does.
 * PSK_ERR_ARG: A not square or empty, a column outside [0, n), a row without a stored diagonal entry, k out of range.
 * PSK_ERR_UNSUPPORTED: a sharded A; a duplicate column within a row; for k >= 1 a filled row longer than PSK_ILUK_ROW_CAP
 * (psk_last_error names the smallest such row); a result over the int32 nnz limit. *P and *Lev are written only on
 * success. A is only read; nothing of it is borrowed. Replaces nothing in the reference. */
#define PSK_ILUK_MAX_LEVEL 8
#define PSK_ILUK_ROW_CAP 512
int psk_csr_iluk_pattern(const psk_csr *A, int32_t k, psk_csr **P, psk_csr **Lev);
/* The ILU(k) preconditioner of A: psk_csr_iluk_pattern, then psk_prec_create_ilu0 on the padded matrix — the numeric
 * factorisation, the L / U split and the hand-off to the triangular-solve chain are those of ILU(0), unchanged. The
 * result is a PSK_PREC_ILU: psk_prec_apply, psk_prec_info, psk_prec_trisolve_schedule, psk_prec_trisolve_sweeps and
 * the solvers take it like any other. Errors as psk_csr_iluk_pattern, then as psk_csr_ilu0 (a zero or non-finite
 * pivot on the padded pattern is reported in psk_csr_ilu0's words); A is not borrowed. */
int psk_prec_create_iluk(const psk_csr *A, int32_t k, psk_prec **out);

/* ---- factorized sparse approximate inverse on the device (fsai.hip) ---------------------------- */
/* G = the FSAI factor of a square, symmetric, definite A on a prescribed pattern: a sparse lower-triangular
 * G ~ L^-1, where s A = L L^T and s = +-1 is A's sign, formed from n independent small dense problems. pattern == NULL
 * means A's own pattern; otherwise pattern is a square device CSR of A's size of which only the structure is read,
 * and its entries with column > row are ignored.
 * Row i's index set: J = the pattern row's columns <= i in ascending order, m = |J|. J must contain i
 * (PSK_ERR_ARG). A duplicate column within a row of A or of the pattern is PSK_ERR_UNSUPPORTED, and so is
 * m > PSK_FSAI_ROW_CAP (psk_last_error names the smallest such row). Rows of A and of the pattern may be stored in
 * any order (they are sorted into working copies first).
 * Sign: s = +1 when row 0's stored diagonal entry of A is > 0, -1 when it is < 0 (zero, missing or not finite:
 * PSK_ERR_ARG); *sign = s. The factorisation runs on s A, an exact sign flip, so a negative definite A (such as
 * FDLaplacian2D(-1, 1, m)) is taken as Jacobi takes it.
 * Arithmetic: all f64, every operation rounded once, a product rounded before its add or subtract (no FMA).
 *   Submatrix, for 0 <= b <= a < m: B[a][b] = s * (the entry of row J[a] of A with column J[b], or 0.0 when it is not
 *   stored). Only A's lower triangle is read; symmetry is not checked.
 *   Cholesky, for b = 0..m-1 and a = b..m-1: t = B[a][b], then t = t - C[a][k] * C[b][k] for k = 0..b-1 in ascending
 *   k. If a == b, t must be > 0 and finite (else PSK_ERR_ARG "not positive definite", psk_last_error naming the
 *   smallest such row i) and C[b][b] = sqrt(t); otherwise C[a][b] = t / C[b][b] (IEEE division).
 *   Back substitution for g = C^-T e_m: g[m-1] = 1.0 / C[m-1][m-1]; for a = m-2 down to 0: u = 0.0, then
 *   u = u + C[b][a] * g[b] for b = a+1..m-1 ascending, and g[a] = (-u) / C[a][a].
 *   Row i of G stores the columns J in ascending order with the values g.
 * Every value's update sequence is fixed above, so the result does not depend on the launch geometry or on which of
 * the two numeric kernels handled the row: one lane per row when every m <= 4 (stencils on their own pattern), one
 * wave per row otherwise or when flags holds PSK_FSAI_WAVE_ONLY. No kernel waits for another wave.
 * The result ends like psk_csr_create(..., PSK_DEVICE) (the SpMV layout choice applies) and psk_csr_download reads
 * it back. *G and *sign are written only on success. A and the pattern are only read; nothing is borrowed.
 * PSK_ERR_UNSUPPORTED also: a sharded A or pattern. PSK_ERR_ARG also: A not square or empty, a pattern of another
 * size, a column outside [0, n), an unknown flag. Replaces nothing in the reference. */
#define PSK_PREC_FSAI      6       /* preconditioner kind: M^-1 v = G^T (G v) (psk_prec_create_fsai) */
#define PSK_FSAI_ROW_CAP   64      /* longest pattern row (lower part, diagonal included) */
#define PSK_FSAI_WAVE_ONLY 1       /* flags: every row through the general (wave-per-row) kernel */
int psk_csr_fsai(const psk_csr *A, const psk_csr *pattern, int32_t flags, psk_csr **G, int32_t *sign);
/* The FSAI preconditioner of A: psk_csr_fsai, then Gt = s G^T by psk_csr_transpose (the values flipped exactly when
 * s = -1). M^-1 v = Gt (G v) ~ A^-1 v: t = G v, out = Gt t, two launches of the library's SpMV on the apply's stream
 * with the bits of two psk_spmv calls. s M^-1 is symmetric positive definite by construction (G has a positive
 * diagonal), so PCG and MINRES may use it on a definite A; GMRES, BiCGStab and the AMG smoother slot take it like
 * any other. The preconditioner owns G, Gt and one n-vector; psk_prec_info reports kind PSK_PREC_FSAI,
 * nnz_l = nnz_u = nnz(G) and 0 levels. Errors as psk_csr_fsai; A and the pattern are not borrowed. Replaces nothing
 * in the reference. */
int psk_prec_create_fsai(const psk_csr *A, const psk_csr *pattern, int32_t flags, psk_prec **out);
/* The formed factor: A's sign, the entries of G and its longest row. Any out pointer may be NULL. PSK_ERR_ARG when M
 * is not a PSK_PREC_FSAI. */
int psk_prec_fsai_info(const psk_prec *M, int32_t *sign, int64_t *nnz_g, int32_t *max_row);

/* ---- multicolour Gauss-Seidel (color_plan.hip, mcgs.hip) ---------------------------------------- */
/* A colouring of the n rows of a square CSR structure (host arrays; no device is touched): first-fit greedy in natural
 * row order on the structure of A + A^T. The neighbours of row i are the columns j != i stored in row i plus the rows
 * j != i that store column i; explicitly stored zeros count as structure; rows may be unsorted and hold duplicate
 * columns. For i = 0..n-1 ascending, color[i] = the smallest c >= 0 that no already-coloured neighbour holds;
 * *ncolors = max(color) + 1. No two neighbours share a colour. O(nnz) (A^T's structure by a counting sort). Exactly
 * red/black on the 5-point stencil. PSK_ERR_ARG: n <= 0, a column outside [0, n), row pointers that do not start at 0 or that decrease. Replaces
 * nothing in the reference. */
int psk_color_plan(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t *color, int32_t *ncolors);
/* The multicolour Gauss-Seidel preconditioner of a square device CSR A: z = M^-1 v is `sweeps` Gauss-Seidel sweeps
 * for A z = v from z = 0 with the rows ordered by the colours of psk_color_plan, C of them. Rows of one colour do not
 * reference each other, so each colour is one streaming launch: no dependency level, no wait between workgroups, no
 * grid sum, and a sweep over all colours reads A once.
 * Setup: A's structure is coloured on the host; more than PSK_MCGS_MAX_COLORS colours is PSK_ERR_UNSUPPORTED
 * (psk_last_error names the count). The preconditioner owns a colour-grouped copy of A (colour 0's rows first, ascending
 * row index inside a colour, every row's entries in their stored order) and DInv_i = 1.0 / a_ii, a_ii = the sum of row
 * i's stored col == row entries in stored order as for PSK_PREC_JACOBI; a diagonal that is zero, missing or not
 * finite is PSK_ERR_ARG (psk_last_error names the smallest such row). A is not borrowed.
 * Apply, all f64, every operation rounded once, a product rounded before its add (no FMA):
 *   z = 0
 *   repeat `sweeps` times: for colour k in ORDER, for every row i of colour k independently:
 *       acc = 0.0;  acc = acc + a_ij * z_j for every stored entry of row i, diagonal included, in stored order
 *       z_i = z_i + DInv_i * (v_i - acc)
 * ORDER = 0, 1, ..., C-1; with PSK_MCGS_SYMMETRIC, 0, ..., C-1, C-2, ..., 0 (2C-1 launches; repeating colour C-1
 * would change nothing in exact arithmetic). A launch reads z_j of other colours and writes only its own rows' z_i, so
 * the result does not depend on the launch geometry. out must not alias v.
 * With PSK_MCGS_SYMMETRIC and a symmetric positive definite A the operator is symmetric positive definite for any
 * sweeps >= 1: it is (I - (I - M_sgs^-1 A)^sweeps) A^-1 with M_sgs the symmetric Gauss-Seidel splitting in the colour
 * order. PCG and MINRES take it with the flag; GMRES, BiCGStab and the smoother[k] slot of psk_prec_create_amg take
 * either form (as a smoother, x <- x + M^-1 (f - A x) with sweeps = 1 is one Gauss-Seidel sweep from x in the
 * colour order). psk_pcg_multi answers PSK_ERR_UNSUPPORTED for it.
 * psk_prec_info reports kind PSK_PREC_MCGS, nnz_l = nnz_u = nnz(A) and levels_l = levels_u = C.
 * PSK_ERR_ARG also: sweeps < 1, an unknown flag, A not square or empty. PSK_ERR_UNSUPPORTED also: a sharded A.
 * Replaces nothing in the reference. */
#define PSK_PREC_MCGS        7     /* preconditioner kind: multicolour Gauss-Seidel (psk_prec_create_mcgs) */
#define PSK_MCGS_MAX_COLORS  64    /* most colours a matrix may need */
#define PSK_MCGS_SYMMETRIC   1     /* flags: colours forward then backward (symmetric Gauss-Seidel) */
int psk_prec_create_mcgs(const psk_csr *A, int32_t sweeps, int32_t flags, psk_prec **out);
/* What was formed: the colour count, the sweeps, the flags and the rows of each colour (color_rows: *ncolors counts, at
 * most PSK_MCGS_MAX_COLORS). Any out pointer may be NULL. PSK_ERR_ARG when M is not a PSK_PREC_MCGS. */
int psk_prec_mcgs_info(const psk_prec *M, int32_t *ncolors, int32_t *sweeps, int32_t *flags, int64_t *color_rows);

/* ---- solvers ------------------------------------------------------------------------------ */
/* M == NULL means identity. b, x: length n (local length for a distributed A); with loc ==
 * PSK_DEVICE b is read in place and x written in place during the solve (x must not alias b). hist: nullable
 * HOST array of ctl->maxiter doubles receiving the per-iteration residual norms reportIter
 * sees (PCG ||r_k||, GMRES |g[k+1]|); entries past res->iters+1 are left untouched.
 * x is overwritten with the solution (SolveStatus.soln()). */
int psk_pcg(const psk_csr *A, const psk_prec *M, const double *b, double *x, const psk_ctl *ctl,
            psk_result *res, double *hist, int32_t loc);
int psk_gmres(const psk_csr *A, const psk_prec *M, const double *b, double *x, const psk_ctl *ctl,
              psk_result *res, double *hist, int32_t loc);
/* Right-preconditioned BiCGStab for nonsymmetric A (no reference counterpart: the reference's only nonsymmetric
 * method is GMRES): about eight vectors and two SpMVs per iteration whatever the iteration count, no restart
 * (ctl->restart is ignored). x0 = 0, every elementwise operation rounded once:
 *   r = rhat = p = b; rho = rhat.r; per iteration k: v = A M^-1 p; alpha = rho / rhat.v; s = r - alpha v;
 *   ||s|| <= tau*||b||: x += alpha M^-1 p, hist[k] = ||s||, stop (the half step). Else t = A M^-1 s;
 *   omega = t.s / t.t; x = (x + alpha M^-1 p) + omega M^-1 s; r = s - omega t; hist[k] = ||r||; stop when
 *   ||r|| <= tau*||b|| or k == maxiter-1 with !fail_on_maxiter; beta = (rhat.r / rho)(alpha / omega);
 *   rho = rhat.r; p = r + beta (p - omega v).
 * Stopping at iteration k: PSK_CONVERGED, iters = k+1, hist_len = k+1; on a tolerance exit (PSK_EXIT_TOLERANCE)
 * resid = the true ||b - A x|| and resid_recursive the recursive one, PSK_TRUE_RESID_FAIL when the true one
 * misses tau*||b|| (as psk_gmres). rhat.v, t.t, omega or rhat.r == 0 at iteration k: PSK_BREAKDOWN, iters = k
 * (PSK_EXIT_DOT_BREAKDOWN). maxiter reached: PSK_MAXITER, iters = maxiter-1. b = 0: as psk_pcg. ctl->norm_b as for
 * psk_gmres. spmv_launches counts the SpMV launches that did their work. A sharded A with more than one rank:
 * PSK_ERR_UNSUPPORTED. */
int psk_bicgstab(const psk_csr *A, const psk_prec *M, const double *b, double *x, const psk_ctl *ctl,
                 psk_result *res, double *hist, int32_t loc);
/* Right-preconditioned IDR(s) (Sonneveld and van Gijzen) for nonsymmetric A (no reference counterpart): a fixed
 * footprint of 2s + 5 vectors (2s + 6 with Jacobi, 2s + 7 with a general preconditioner; the shadow space is
 * regenerated from a hash, never stored), ONE SpMV and one
 * preconditioner apply per step, 1 <= s <= PSK_IDRS_MAX_S (ctl->restart is ignored). The biorthogonal variant, each new
 * direction made orthogonal from a single s-wide dot product. One STEP is one SpMV: hist gets one entry per step, and
 * iters, maxiter and hist_len count steps. x0 = 0, every elementwise operation rounded once:
 *   P[i][j] = double(splitmix64(i*s + j) >> 11) * 2^-52 - 1.0, with splitmix64(t): z = t + 0x9E3779B97F4A7C15;
 *     z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB; z ^ z>>31 (mod 2^64): exact in
 *     f64, the same on every run, not orthonormalised
 *   x = 0; r = b; normB = sqrt(b.b) (or ctl->norm_b); thr = tau*normB; G = U = 0 (n x s); Mm = I_s; om = 1; j = 0
 *   cycle:
 *     f_i = p_i.r, i = 0..s-1
 *     for k = 0..s-1:
 *       c_i, i = k..s-1:  t = f_i;  t = t - Mm[i][l]*c_l, l = k..i-1;  c_i = t / Mm[i][i]
 *       v = r;  v = v - c_i*g_i, i = k..s-1;  v = M^-1 v;  u = om*v;  u = u + c_i*u_i, i = k..s-1
 *       g = A u                                                                  (step j's SpMV)
 *       q_i = p_i.g, i = 0..s-1
 *       a_i, i = 0..k-1:  t = q_i;  t = t - Mm[i][l]*a_l, l = 0..i-1;  a_i = t / Mm[i][i]
 *       g = g - a_i*g_i, u = u - a_i*u_i, i = 0..k-1;  g_k = g;  u_k = u
 *       Mm[i][k], i = k..s-1:  t = q_i;  t = t - Mm[i][l]*a_l, l = 0..k-1;  Mm[i][k] = t
 *       Mm[k][k] == 0: breakdown
 *       beta = f_k / Mm[k][k];  r = r - beta*g;  x = x + beta*u;  hist[j] = sqrt(r.r);  stop test;  j++
 *       f_i = f_i - beta*Mm[i][k], i = k+1..s-1
 *     v = M^-1 r;  t = A v                                                       (step j's SpMV)
 *     tt = t.t;  ts = t.r;  rr = the r.r of the previous step;  tt == 0 or ts == 0: breakdown
 *     rho = ts / (sqrt(tt)*sqrt(rr));  om = ts/tt;  |rho| < 0.7: om = (om*0.7)/|rho|
 *     x = x + om*v;  r = r - om*t;  hist[j] = sqrt(r.r);  stop test;  j++
 *   stop test: hist[j] <= thr, or j == maxiter-1 with !fail_on_maxiter.
 * Every dot product is a sum of products rounded one by one, one per row, in an order that depends on the tile and
 * slot indices only: two identical calls give identical bits, whatever the SpMV layout of A.
 * Stopping at step j: PSK_CONVERGED, iters = j+1, hist_len = j+1; on a tolerance exit (PSK_EXIT_TOLERANCE) resid = the
 * true ||b - A x||, measured by one more SpMV, and resid_recursive the recursive one, PSK_TRUE_RESID_FAIL when the true
 * one misses tau*||b|| (as psk_bicgstab). A breakdown at step j: PSK_BREAKDOWN, iters = j, hist_len = j
 * (PSK_EXIT_DOT_BREAKDOWN), resid = NaN. maxiter reached: PSK_MAXITER, iters = maxiter-1. b = 0: as psk_pcg.
 * ctl->norm_b as for psk_gmres. spmv_launches counts the SpMV launches that did their work: one per step, plus the
 * true residual's. s outside 1..PSK_IDRS_MAX_S: PSK_ERR_ARG. A sharded A with more than one rank:
 * PSK_ERR_UNSUPPORTED. */
#define PSK_IDRS_MAX_S 8
int psk_idrs(const psk_csr *A, const psk_prec *M, const double *b, double *x, const psk_ctl *ctl,
             int32_t s, psk_result *res, double *hist, int32_t loc);
/* Preconditioned MINRES for SYMMETRIC INDEFINITE A (no reference counterpart): Paige-Saunders MINRES in the
 * operation order of scipy.sparse.linalg.minres, with an SPD preconditioner M, x0 = 0, no shift; one SpMV, two dot
 * products and a fixed footprint per iteration (ctl->restart is ignored). Every elementwise operation rounded once:
 *   r1 = b; z = M^-1 r1; beta1^2 = r1.z        (< 0: preconditioner not positive definite; == 0: b = 0 exit)
 *   normB = sqrt(b.b) (or ctl->norm_b); scale = normB / beta1 (exactly 1 for the identity)
 *   oldb = 0; beta = beta1; dbar = epsln = 0; phibar = beta1; cs = -1; sn = 0; w = w2 = 0; r2 = r1
 *   k = 0, 1, ...:
 *     s = 1/beta; v = s z
 *     y = A v;  k >= 1: y = y - (beta/oldb) r1
 *     alfa = v.y                                  (AFTER the r1 term: the stable ordering, and scipy's)
 *     y = y - (alfa/beta) r2;  r1 = r2;  r2 = y;  z = M^-1 r2
 *     oldb = beta;  beta^2 = r2.z  (< 0: preconditioner not positive definite);  beta = sqrt(.)
 *     oldeps = epsln; delta = cs dbar + sn alfa; gbar = sn dbar - cs alfa; epsln = sn beta; dbar = -cs beta
 *     gamma = sqrt(gbar^2 + beta^2)               (== 0: breakdown, singular system)
 *     cs = gbar/gamma; sn = beta/gamma; phi = cs phibar; phibar = sn phibar
 *     w1 = w2; w2 = w; w = (v - oldeps w1 - delta w2) (1/gamma);  x = x + phi w
 *     hist[k] = scale phibar
 *     hist[k] <= tau normB, or k == maxiter-1 and !fail_on_maxiter: stop
 * (v is stored and y = A v runs on it, so the iterates are scipy's to rounding. b.z == 0 with b != 0 is refused like
 * b.z < 0.)
 * THE NORM IN WHICH CONVERGENCE IS JUDGED: phibar is ||r_k|| in the M^-1 norm, sqrt(r.M^-1 r), the quantity MINRES
 * minimises; hist[k] is scaled so that hist[k] / norm_b is the relative reduction in that norm. With the identity it
 * is ||b - A x_k||_2. Under a preconditioner the 2-norm residual is bounded by ||r||_2/||b||_2 <= sqrt(cond(M)) tau,
 * not by tau. A Krylov space that is exhausted gives beta = 0, hence phibar = 0, and leaves by the ordinary test.
 * Stopping at iteration k: PSK_CONVERGED, iters = k+1, hist_len = k+1; on a tolerance exit (PSK_EXIT_TOLERANCE)
 * resid = the true ||b - A x||_2, measured by one more SpMV, and resid_recursive = hist[k]. With the identity a true
 * residual above tau*normB is PSK_TRUE_RESID_FAIL (as psk_gmres); under a preconditioner the solve's contract is
 * the preconditioned norm and the status stays converged. r.z < 0 (at the init: iters = 0; at iteration k:
 * iters = k): PSK_BREAKDOWN, PSK_EXIT_DOT_BREAKDOWN, resid = NaN, "preconditioner not positive definite";
 * gamma == 0: the same codes, "breakdown gamma==0". maxiter reached: PSK_MAXITER, iters = maxiter-1. b = 0: as
 * psk_pcg. ctl->norm_b as for psk_gmres. spmv_launches counts the SpMV launches that did their work: one per
 * iteration, plus the true residual's. A must be symmetric (not checked). A sharded A with more than one rank:
 * PSK_ERR_UNSUPPORTED. */
int psk_minres(const psk_csr *A, const psk_prec *M, const double *b, double *x, const psk_ctl *ctl,
               psk_result *res, double *hist, int32_t loc);
/* PCG on 1 <= nrhs <= PSK_PCG_MULTI_MAX right-hand sides in ONE device loop (no reference counterpart: the reference
 * solves one vector per call). The matrix is streamed once per iteration for all columns; the bound is the grid sum's
 * width (one sum carries one dot product of every column).
 * B and X are n x nrhs, row-major: element (i, j) at i*nrhs + j, a C-contiguous numpy (n, nrhs) array; with loc ==
 * PSK_DEVICE B is read in place and X written once, at the end (X must not alias B: PSK_ERR_ARG). res points to nrhs
 * results, res[j] column j's. hist: nullable HOST array of nrhs * ctl->maxiter doubles, column j's history from
 * hist + j*maxiter; entries past res[j].hist_len are left untouched.
 * EACH COLUMN IS AN INDEPENDENT PCG with the recurrence of psk_pcg (PCGSolver.py:97-138), x0 = 0, every elementwise
 * operation rounded once (no contraction), every matrix row summed in stored order from 0.0 with the products
 * rounded first (the bits of psk_spmv on that column):
 *   r = b; u = M^-1 r; p = u; normB = sqrt(b.b); udr = u.r
 *   k = 0, 1, ...: Ap = A p; alpha = udr / p.Ap; x = x + alpha p; r = r - alpha Ap; u = M^-1 r; hist[k] = sqrt(r.r);
 *       hist[k] <= tau*normB, or k == maxiter-1 with !fail_on_maxiter: stop
 *       beta = u.r / udr; udr = u.r; p = u + beta p
 * Every dot product is a sum of products rounded one by one, one per row, in an order that depends on the tile and
 * slot indices only: for a given nrhs a column's sums, and with them all its bits, do not depend on its position
 * among the columns or on what the other columns hold, and two identical calls give identical bits. (The sums are
 * not those of psk_pcg: iteration counts may differ from it where a residual lies within rounding of the threshold.)
 * Each column has its own udr, alpha, beta, normB, threshold, history, iteration count, exit and breakdown, reported
 * as psk_pcg reports them: stopping at iteration k is PSK_CONVERGED with iters = k+1, hist_len = k+1, resid =
 * resid_recursive = hist[k], exit = PSK_EXIT_TOLERANCE (or PSK_EXIT_MAXITER by the maxiter rule); u.r == 0 at the
 * start (b != 0) is PSK_BREAKDOWN with iters = 0, p.Ap == 0 at iteration k PSK_BREAKDOWN with iters = k, hist_len = k,
 * resid = NaN, exit = PSK_EXIT_DOT_BREAKDOWN; maxiter reached is PSK_MAXITER with iters = maxiter-1, resid = the last
 * hist; b_j = 0 is x_j = 0, PSK_CONVERGED, iters = 1, resid = 0, exit = PSK_EXIT_NONE, hist_len = 0. A breakdown stops
 * that column only. A column that has stopped is frozen: later iterations write nothing to its x, r, p or hist (x_j is
 * the iterate it stopped with). The loop ends when every column has stopped, or at maxiter.
 * loop_ms, spmv_launches (launches of the multi-column SpMV that did their work) and, with ctl->time_kernels, spmv_ms
 * are device-wide: the same in every res[j]. ctl->norm_b and ctl->restart are ignored.
 * Preconditioners: M == NULL (identity) and PSK_PREC_JACOBI; any other kind is PSK_ERR_UNSUPPORTED, and so is a matrix
 * sharded over more than one rank. nrhs outside 1 .. PSK_PCG_MULTI_MAX: PSK_ERR_ARG. The loop reads the matrix's CSR
 * arrays whatever its SpMV layout (psk_csr_layout); it shares the matrix's solver workspace with the other solvers. */
#define PSK_PCG_MULTI_MAX 4
int psk_pcg_multi(const psk_csr *A, const psk_prec *M, int32_t nrhs, const double *B, double *X,
                  const psk_ctl *ctl, psk_result *res /* nrhs of them */, double *hist, int32_t loc);
/* The standalone AMG V-cycle solver, AMGVCycleSolver.solve (VCycleSolver.py:52-95), on the device: M is a
 * PSK_PREC_AMG whose finest level matrix is the system matrix (PSK_ERR_ARG otherwise); its own num_iters and
 * tau are ignored, ctl->maxiter (> 0) and ctl->tau rule. x0 = copy(b) (:69), or the caller's x with
 * PSK_VCYCLE_X0_GIVEN. Each cycle: x = runCycle(b, x), r = b - A x, hist[k] = ||r||, stop when
 * ||r|| < tau*||b|| (strict, :90): PSK_CONVERGED, iters = k+1, exit = PSK_EXIT_TOLERANCE, x = that cycle's
 * iterate. maxiter reached: handleMaxiter(maxiter-1, ...) — PSK_MAXITER, iters = maxiter-1, success =
 * !fail_on_maxiter, x = the last iterate, resid = the last norm, exit = PSK_EXIT_MAXITER. b = 0: x = 0,
 * iters = 1, exit = PSK_EXIT_NONE, no cycle runs. ctl->check_every: cycles between the host's looks at the
 * device's done word (0 = 1); the results do not depend on it. ctl's time_kernels, restart and norm_b are
 * ignored; res->spmv_ms, gather_ms, halo_ms and comm_samples are 0. */
#define PSK_VCYCLE_X0_GIVEN 1   /* x holds the starting iterate; default x0 = copy(b), VCycleSolver.py:69 */
int psk_vcycle(const psk_prec *M, const double *b, double *x, const psk_ctl *ctl,
               psk_result *res, double *hist, int32_t flags, int32_t loc);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ------------------------------------- */
#define PSK_UNIQUE_ID_BYTES 128
int psk_comm_unique_id(uint8_t *id /* PSK_UNIQUE_ID_BYTES */);
int psk_comm_init(int32_t nranks, int32_t rank, const uint8_t *id, psk_comm **out);
/* Validation only: a communicator of `nranks` with no RCCL behind it. Sharded matrices can be
 * built on ONE GPU for any rank and psk_spmv then takes the full local [owned | halo] x from the
 * caller; collectives (and hence sharded solves) return PSK_ERR_UNSUPPORTED. */
int psk_comm_init_dry(int32_t nranks, int32_t rank, psk_comm **out);
/* Validation only: a communicator whose collectives run through a POSIX shared-memory segment
 * `name` ("/..."; the same on every rank, unique per job) between nranks processes of ONE host,
 * stream-ordered like the RCCL calls they stand in for (D2H, host barrier, H2D). Lets the sharded
 * solvers run with nranks > 1 on a single GPU, where RCCL refuses duplicate devices. Slow; never
 * used for timing. */
int psk_comm_init_host(int32_t nranks, int32_t rank, const char *name, psk_comm **out);
/* Device-side exchange of the sharded solvers' scalars (round 5): attach the host-shared mailbox `name`
 * ('/...', a POSIX shared-memory name, the same on every rank; collective over the ranks of c, which
 * must share one node). psk_pcg then exchanges its per-rank dot products by direct system-scope stores
 * of the kernels that finish them into every rank's mailbox slot and a one-wave gather kernel per rank,
 * instead of ncclAllGather (the halo of p stays on RCCL / the host transport). Same bits as the
 * all-gather: every rank still sums the P values in rank order. Replaces nothing in the reference. */
int psk_comm_mailbox(psk_comm *c, const char *name);
/* Self-check of the attached mailbox (collective over c's ranks): `rounds` exchanges of known values
 * through the same kernel stores and gather the solvers use; PSK_ERR_RCCL when a value is wrong or never
 * arrives (bounded wait). bench.py runs it before a multi-GPU run and falls back to RCCL all-gathers. */
int psk_comm_mailbox_check(psk_comm *c, int32_t rounds);
int psk_comm_destroy(psk_comm *c);
/* Rank `rank`'s row block of FDLaplacian2D(a,b,m): rows [row_begin,row_end) split on
 * whole grid lines; local columns are [owned | halo_lo | halo_hi]. */
int psk_csr_create_fd2d_dist(double a, double b, int64_t m, psk_comm *c, psk_csr **out,
                             int64_t *row_begin, int64_t *row_end);
/* Host-only: the row block and local column layout psk_csr_create_fd2d_dist uses for `rank`
 * (callable without a GPU; the CPU tests check the sharding plan with it). */
int psk_fd2d_dist_plan(int64_t m, int32_t nranks, int32_t rank, int64_t *row_begin, int64_t *row_end,
                       int64_t *ncols, int64_t *halo_lo, int64_t *halo_hi);
/* General row-block sharding: rank c->rank's rows [row_starts[rank], row_starts[rank+1]) of a
 * global n_global x n_global CSR (the row split of every rank in row_starts[nranks+1], 0 ..
 * n_global). Host arrays of the local rows only, GLOBAL column indices: rowptr[nloc+1] may start
 * anywhere (entry j of local row i is colidx[rowptr[i]-rowptr[0]+j']); stored order is kept.
 * Local columns are [owned | halo], the halo being the distinct off-block columns in ascending
 * global order (psk_csr_halo_cols). The pattern must be structurally symmetric across ranks (as
 * any matrix PCG runs on): each rank sends a peer the owned rows that reference the peer's block,
 * which is then exactly what the peer needs; under RCCL every rank checks this at creation and all
 * of them return PSK_ERR_ARG otherwise. Halo sends that are not a contiguous row range are packed
 * by one gather kernel before the grouped ncclSend/ncclRecv. Replaces: nothing in the reference
 * (single-process); the solvers take such a matrix with rank-local b and x. */
int psk_csr_create_dist(int64_t n_global, const int64_t *row_starts, const int64_t *rowptr,
                        const int32_t *colidx, const double *vals, psk_comm *c, psk_csr **out);
/* Global index of every halo column of a sharded matrix, in local column order (cols may be
 * NULL to query the count). */
int psk_csr_halo_cols(const psk_csr *A, int64_t *cols, int64_t *count);
/* Halo plan of a sharded matrix, one entry per peer rank (ascending): what is sent to it and which
 * segment of the halo it fills. Arrays may be NULL; *npeers <= nranks-1. */
int psk_csr_halo_peers(const psk_csr *A, int32_t *ranks, int64_t *send_counts, int64_t *recv_counts,
                       int64_t *recv_offsets, int32_t *npeers);
/* Validation: the values halo_exchange sends, peer by peer, for the local vector x (device
 * pointers; out holds sum(send_counts) doubles), packed by the same kernel. No communication. */
int psk_csr_halo_pack(const psk_csr *A, const double *x, double *out);

#ifdef __cplusplus
}
#endif
#endif /* PSK_H */
