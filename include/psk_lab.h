/* psk_lab.h — test / lab entry points of libpsk_lab.so (round 6: out of the product library and its header).
 *
 * libpsk_lab.so is a separate shared library linked against libpsk.so (it shares libpsk's device context,
 * streams and handles). Nothing in include/psk.h or the product path uses it; tests/test_gpu_progress.py and
 * tools/progress_probe.py load it (pysolvers_amd._native.load_lab()). None of these replaces a reference
 * interface. */
#ifndef PSK_LAB_H
#define PSK_LAB_H

#include "psk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Lab / tests of the triangular solves' forward progress (round 5; replaces nothing in the reference).
 * psk_lab_occupy_begin starts `wgs` workgroups of 1024 threads holding `lds_bytes` of LDS each on a
 * stream of their own, spinning until psk_lab_occupy_end releases them behind everything enqueued on the
 * solver's stream so far (or `seconds` pass: *timed_out = 1); a solve enqueued in between can use only
 * what they leave free. psk_lab_trisolve_workers: the workgroups the last sync-free launch of factor
 * `which` enrolled and the grid it was launched with (the sync-free schedule deals its rows over the
 * workgroups that started, not over the grid). */
int psk_lab_occupy_begin(int32_t wgs, int32_t lds_bytes, double seconds);
int psk_lab_occupy_end(int32_t *timed_out);
/* Lab: nwg workgroups of 128 threads with lds_bytes of LDS, each spinning usec; rec_out[3*i..] = start, end
 * (s_memrealtime, 100 MHz) and XCD of workgroup i. Waits for the launch. */
int psk_lab_dispatch_probe(int32_t nwg, int32_t lds_bytes, double usec, int64_t *rec_out);
/* Lab: occupiers per XCD (HW_REG_XCC_ID) of the last psk_lab_occupy_begin, counts[8]. */
int psk_lab_occupy_xcc(int32_t *counts);
int psk_lab_trisolve_workers(const psk_prec *M, int32_t which, int32_t *enrolled, int32_t *grid);
/* Lab / tests of the triangular-solve planner (plan_factor, trisolve_plan.hip); touches no GPU. The plan of one
 * factor (CSR with its diagonal unless `unit`; nat: the natural index of every row, or NULL) for a device of
 * num_cus CUs whose sync-free launch runs syncfree_waves waves (on a device: psk_lab_trisolve_workers' grid x 4):
 * *schedule = the TriSchedule chosen, est[6] = the cost models' estimates in us by TriSchedule (-1: not
 * eligible), info[8] = levels, band K / blocks / ring words / narrow, grid K / dictionary records, levels steps
 * (0 where the layout was not built). Reads PSK_TRISOLVE_* / PSK_BAND_NARROW as factor creation does. */
int psk_lab_trisolve_plan(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, int32_t upper,
                          int32_t unit, const int32_t *nat, int32_t num_cus, int64_t syncfree_waves, int32_t *schedule,
                          double *est, int64_t *info);
/* Lab / tests of the host shard planner (dist_plan and dist_peers, dist_plan.hip); touches no GPU. The plan
 * psk_csr_create_dist makes for rank `rank` of P: rows [row_starts[rank], row_starts[rank+1]) of a global CSR with
 * n_global columns, given as that block's rowptr (nloc + 1 entries, any base) and colidx (global columns).
 * row_starts and rowptr must be monotone (psk_csr_create_dist checks that before it plans). Outputs, all allocated
 * by the caller: lcol[nnz] = the local column of every entry; halo = the global ids of the halo columns, *nhalo of
 * them (at most nnz); pack = the send rows of the packed peers, concatenated, *npack of them (at most nnz);
 * peers[7 * k ..] = rank, send_count, send_begin, packed, pack_off, recv_count, recv_offset of halo peer k, *npeers
 * of them (at most P). A column index outside [0, n_global) is refused with PSK_ERR_ARG. */
int psk_lab_dist_plan(int64_t n_global, const int64_t *row_starts, int32_t P, int32_t rank, const int64_t *rowptr,
                      const int32_t *colidx, int32_t *lcol, int64_t *halo, int64_t *nhalo, int32_t *pack, int64_t *npack,
                      int64_t *peers, int32_t *npeers);
/* Lab / tests of the AMG smoother's paired Gauss-Seidel sweeps (round 6, amg_gs_pair.hip gs_pair_kernel): set = 0
 * runs every level's sweeps one launch each (the serialized path), 1 pairs them on the levels that qualify, -1
 * leaves the setting; *levels_on = the levels pairing now, *levels_eligible = the levels that qualify. */
int psk_lab_amg_gs_pair(psk_prec *M, int32_t set, int32_t *levels_on, int32_t *levels_eligible);
/* Lab (round 6): back-to-back SpMV launches (dot = 0: plain y = A x; 1: the PCG loop's kSpmvDot launch) that cycle
 * through nbuf (x, y) device buffer pairs, one warm launch per pair first, then reps timed launches between two
 * events; *avg_ms = the mean launch. nbuf = 1 is psk_spmv_timed; nbuf > 1 with more bytes than the Infinity Cache
 * holds prices the launch without a cache-resident x (tools/mall_probe.py). */
int psk_lab_spmv_rotate(const psk_csr *A, const double *const *xs, double *const *ys, int32_t nbuf, int32_t reps,
                        int32_t dot, double *avg_ms);
/* Lab (round 6): the SpMV launch's own time (dispatch-recorded events) when each launch follows a streaming write
 * kernel (scratch = src, 16-B accesses): target 0 = no writer, 1 = the writer writes the SpMV's x (as K3 writes the
 * p the next SpMV gathers), 2 = it writes `scratch` (another buffer of n doubles). reps <= 256. */
int psk_lab_spmv_after_write(const psk_csr *A, double *x, double *y, const double *src, double *scratch,
                             int32_t target, int32_t reps, int32_t dot, double *avg_ms);
/* Lab (tools/cheby_ab.py): one Chebyshev step (PSK_PREC_CHEBYSHEV handle of degree >= 3, device vector v) timed two
 * ways between HIP events on the library stream, reps launches back to back after one untimed step: the fused
 * launch (cheby_step_kernel), and the same update composed of the residual SpMV in A's current layout, the DInv
 * scale, the d update and the z update (four launches). Milliseconds per step. */
int psk_lab_cheby_ab(const psk_prec *M, const double *v, int32_t reps, double *fused_ms, double *pieces_ms);
/* Lab / tests of the PCG loop's staggered x flush (pcg_state.hpp); the first two touch no GPU.
 * psk_lab_pcg_stagger: *blocks = S, the row blocks the build flushes in turn (0: built with the uniform flush only),
 * *ring = the depth of the ring of p buffers. psk_lab_pcg_flush_schedule: the one schedule function the SpMV's flush
 * role, K3, pcg_flush_kernel and the host call, for any S >= 1: *blk = the block of K3 tile `tile` of nv, and
 * first_last[2] = the first and last iteration whose x update is pending for that block when the flush role of SpMV
 * launch k runs (in_spmv = 1; the launch serves block k mod S) or when K3 / pcg_flush_kernel of iteration k runs
 * (in_spmv = 0); first > last: none; first == 0: the block was never stored (x is the implicit 0).
 * psk_lab_pcg_flush: pcg_flush_kernel as after a breakdown at iteration k >= 1 on host vectors: x[n] (in and out),
 * ring[ring depth][n] (row j = the buffer of p_i, i mod depth == j), alphas[k]; stag = 1 per-block ranges, 0 the
 * uniform rule. */
int psk_lab_pcg_stagger(int32_t *blocks, int32_t *ring);
/* *on = 1 when psk_pcg of matrix A in its current SpMV layout with preconditioner M (NULL: none) takes the staggered
 * flush, 0 when it keeps the uniform flush in K3. */
int psk_lab_pcg_staggers(const psk_csr *A, const psk_prec *M, int32_t *on);
int psk_lab_pcg_flush_schedule(int32_t S, int64_t nv, int64_t tile, int64_t k, int32_t in_spmv, int32_t *blk,
                               int64_t *first_last);
int psk_lab_pcg_flush(int64_t n, int64_t k, int32_t stag, double *x, const double *ring, const double *alphas);
/* Tests of the solvers' workspace layouts (solve_loop.hpp Carve); touches no GPU. Runs the layout function of
 * `solver` on null-based carvers, the one its solve sizes and carves its buffers with: offsets[*count] = the byte
 * offset of every region in the order the layout takes them (PCG, GMRES, BiCGStab, MINRES: the regions of the matrix's
 * large workspace, then those of its small one, each counted from its own buffer's start), bytes[2] = the sizes the two
 * buffers are grown to (the V-cycle has one: bytes[1] = 0). On entry *count = the capacity of offsets.
 * PCG reads n, ncols, maxiter, flags (GEN, OWN_X) and P ranks; GMRES n, maxiter, restart, flags (GEN); the V-cycle
 * n, maxiter, flags (DEV_IO); BiCGStab n, maxiter, flags (GEN); MINRES n, maxiter, flags (GEN); the multi-column PCG
 * (psk_pcg_multi) n, maxiter and P = nrhs (1 .. PSK_PCG_MULTI_MAX, PSK_ERR_ARG beyond).
 * Solver id 4 is not taken:
 * tests/test_solver_layout.py keeps it as its example of an unknown solver. */
#define PSK_LAB_SOLVER_PCG 0
#define PSK_LAB_SOLVER_GMRES 1
#define PSK_LAB_SOLVER_VCYCLE 2
#define PSK_LAB_SOLVER_BICGSTAB 3
#define PSK_LAB_SOLVER_MINRES 5
#define PSK_LAB_SOLVER_PCG_MULTI 6
#define PSK_LAB_LAYOUT_GEN 1    /* general preconditioner (u, GMRES's w and t, or BiCGStab's ph and sh, materialised) */
#define PSK_LAB_LAYOUT_OWN_X 2  /* PCG: x in the workspace (host vectors), not the caller's device vector */
#define PSK_LAB_LAYOUT_DEV_IO 4 /* V-cycle: b and x are the caller's device vectors (not staged) */
int psk_lab_solver_layout(int32_t solver, int64_t n, int64_t ncols, int64_t maxiter, int64_t restart, int32_t flags,
                          int32_t P, int64_t *offsets, int32_t *count, int64_t *bytes);
/* Tests of the GMRES Arnoldi kernels (tests/test_gpu_gmres_arnoldi.py): what the last psk_gmres on matrix A left in
 * its workspace. psk_gmres carves A's two workspace buffers with one layout function and the buffers stay on the
 * matrix after the solve; this carves them again for the same maxiter, restart and gen (1: a general preconditioner,
 * one that is neither none nor Jacobi), waits for the library stream and copies to host arrays, any of which may be
 * NULL. With K = the basis of one cycle (restart, or maxiter when it is 0 or larger): Q = the first `cols` basis
 * vectors of the last cycle, n x cols column-major (the padded column stride removed); H = the unrotated Hessenberg
 * columns and R = the rotated ones, (K+1) x K column-major; CS[2K] = the rotations (c, s); g[K+1]; y[K+1] = the last
 * least-squares solution; state[6] = done, brk, kconv, normB, tauNormB, rec of the solve's device state. In a
 * restarted solve H, R, CS and g hold the last cycle's columns on top of what earlier cycles left beyond them.
 * PSK_ERR_ARG when either buffer is smaller than that layout needs or cols > K+1. It reads only.
 * psk_lab_gmres_prefill: psk_gmres never clears its basis or its rotations, so a test of what the kernels leave
 * untouched (the columns after a breakdown or after convergence) first grows A's two buffers to what that solve will
 * ask for and sets every byte of both to `byte`; the solve then keeps the buffers. */
int psk_lab_gmres_internals(const psk_csr *A, int64_t maxiter, int32_t restart, int32_t gen, int32_t cols, double *Q,
                            double *H, double *R, double *CS, double *g, double *y, double *state);
int psk_lab_gmres_prefill(psk_csr *A, int64_t maxiter, int32_t restart, int32_t gen, int32_t byte);
/* Tests of the PCG kernels (tests/test_gpu_pcg_kernels.py): what the last psk_pcg on the unsharded matrix A left in
 * its workspace. psk_pcg carves A's two workspace buffers with one layout function and the buffers stay on the matrix
 * after the solve; this carves them again for the same maxiter, gen (1: a general preconditioner, one that is
 * neither none nor Jacobi) and own_x (1: the solve ran on host vectors, so x lives in the workspace; 0: x is the
 * caller's device vector), waits for the library stream and copies to host arrays, any of which may be NULL.
 * r[n], Ap[n]; ring[depth][ncols] with depth = psk_lab_pcg_stagger's *ring: row j = the buffer of p_i, i mod depth ==
 * j (gen = 1 keeps one buffer, p in place: only row 0 is copied, the other rows are left as passed); u[n] is copied
 * only with gen = 1 (the Jacobi / identity kernels never store u), x[n] only with own_x = 1; alphas, udr and hist have
 * maxiter + 1 entries each (alphas[k] and udr[k + 1] are stored by K3 of an iteration k that did not end the solve;
 * the general path stores no alphas); sums[3] = the last finished grid sums p.Ap, r.r and u.r (part1[0], part2[0] and
 * part2[1]; with gen = 1 the third is pcg_dot_kernel's sum, part3[0]); state[8] = done, brk_kind, iters, resid, normB,
 * tauNormB, live, x_written of the solve's device state. PSK_ERR_ARG when either buffer is smaller than that layout
 * needs or the matrix is sharded. It reads only.
 * psk_lab_pcg_prefill: psk_pcg clears none of these regions (each entry is written before it is read), so a test of
 * what the kernels queued behind a stop leave untouched first grows A's two buffers to what that solve will ask for
 * and sets every byte of both to `byte`; the solve then keeps the buffers. */
int psk_lab_pcg_internals(const psk_csr *A, int64_t maxiter, int32_t gen, int32_t own_x, double *r, double *ring,
                          double *Ap, double *u, double *x, double *alphas, double *udr, double *hist, double *sums,
                          double *state);
int psk_lab_pcg_prefill(psk_csr *A, int64_t maxiter, int32_t gen, int32_t own_x, int32_t byte);
/* Tests of the multi-column PCG kernels (tests/test_gpu_pcg_multi.py): what the last psk_pcg_multi on matrix A left in
 * its workspace, carved again for the same maxiter and nrhs; waits for the library stream and copies to host arrays,
 * any of which may be NULL. With KP = nrhs rounded up to 2 or 4: alphas, udr and pap hold nrhs rows of maxiter + 1
 * entries (alphas[j][k] and pap[j][k] = column j's alpha and p.Ap sum of iteration k, udr[j][k] its u.r in front of
 * iteration k; entries of iterations the column did not run are left as the solve found them); r, p, Ap and x are the
 * final INTERLEAVED work vectors, n x KP row-major (padding columns included); state holds 10 doubles per column:
 * done (0 running, 1 converged or b = 0, 2 breakdown), brk_kind, iters, history entries, normB, tauNormB, the current
 * udr, the last reported ||r||, the init's b.b sum and the last r.r sum the column took part in. PSK_ERR_ARG when
 * either buffer is smaller than that layout needs, nrhs is out of range or the matrix is sharded. It reads only. */
int psk_lab_pcg_multi_internals(const psk_csr *A, int64_t maxiter, int32_t nrhs, double *alphas, double *udr, double *pap,
                                double *r, double *p, double *Ap, double *x, double *state);
/* Measurement (tools/ilu0_ab.py): where the last psk_csr_ilu0 / psk_prec_create_ilu0 of this process spent its time.
 * out[0..6] = ms of the column sort and structure checks, of the pattern download and dependency levels, of the
 * numeric launches (HIP events around them), of the value download and L / U split, of psk_prec_create_trisolve
 * (planner and uploads; the last two are 0 after psk_csr_ilu0), then the level count and the lanes per row. Touches
 * no GPU. */
int psk_lab_ilu0_timing(double *out);
/* Measurement (tools/iluk_ab.py): the last psk_csr_iluk_pattern / psk_prec_create_iluk of this process. out[0..6] = ms
 * of the symbolic phase (sort, rounds, padding; host wall time), the level k, the rounds that added entries, the
 * rounds in which the 64-lane instance ran beside a narrower one, the lanes per row of the last round, nnz(A), nnz(P).
 * The numeric and planner times of the same call are psk_lab_ilu0_timing's. Touches no GPU. */
int psk_lab_iluk_timing(double *out);
#ifdef __cplusplus
}
#endif

#endif /* PSK_LAB_H */
