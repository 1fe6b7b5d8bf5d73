// trisolve_syncfree.hip — the sync-free schedule and its single-workgroup LDS variant (they share the row
// pipeline).
//
// Sync-free (sptrsv_kernel): one wave per row, rows dealt to a co-resident grid in a
// level-sorted topological order computed on the host (k-th row of that order -> wave k mod W; every
// row depends only on rows earlier in the order, so the first unsolved row can always proceed).
// Level order instead of index order cut the apply at FD m=1024 from 255 ms to 17 ms. Each
// dependency level costs about one cross-CU hand-off (~1 us, MI355X_MICROARCH.md "handoff-1to1").
#include "trisolve.hpp"

#include <algorithm>

namespace psk {

// Branch-free row pipeline (the LDS kernel's, SfSrc below). The compiler's vmcnt waits count only
// the memory operations it knows were issued; a load under a divergent branch (a lane test, a row
// past the end) is not counted, so the wait for a row's first dependency became vmcnt(0) — it also
// waited for the prefetch of the rows D ahead issued after it, which is what the pipeline exists to
// hide. Every load of SfSrc is issued by every lane at a clamped, valid address (the value selected
// afterwards), the row header is loaded per lane (VMEM, counted in order, not SMEM), and the rare
// slow path (a row longer than the register chunks) ends with an explicit vmcnt(0), so the fast
// path's counts survive its join.
constexpr int kSfChunks = 3;   // 64-entry chunks of a row held in registers (longer rows loop)
struct SfBody {
    int32_t row, s, e, ri, c[kSfChunks];
    double v[kSfChunks], d;
};


// the loads of a row (positions clamped into [0, n), entries into [0, nnz); callers select)
struct SfSrc {
    int64_t n;
    int32_t last;   // nnz - 1 (>= 0)
    const int32_t *krp, *kci, *krow, *ridx;   // ridx: rhs_idx, or krow (any valid int array of n)
    const double *kva, *dg;                   // dg: diag, or rhs (any valid double array of n)
    bool has_ri, has_d;
    int32_t zv;                               // opaque zero: per-lane header loads
    __device__ void head(int64_t k, SfHead &h) const {
        const int64_t kk = (k < n ? k : n - 1) + zv;
        h.row = krow[kk];
        h.s = krp[kk];
        h.e = krp[kk + 1];
    }
    __device__ void body(const SfHead &h, SfBody &b, int lane) const {
        b.row = h.row;
        b.s = h.s;
        b.e = h.e;
        // lanes past the row's end re-read its first entry (the line lane 0 reads; an empty row: the
        // entry before it), never one shared address (a hot line every wave would hit)
        const int32_t fb = h.s < h.e ? h.s : (h.e > 0 ? h.e - 1 : 0);
#pragma unroll
        for (int j = 0; j < kSfChunks; ++j) {
            const int32_t idx = h.s + 64 * j + lane;
            const bool ok = idx < h.e;
            const int32_t ic = ok ? idx : fb;
            const int32_t c = kci[ic];
            const double v = kva[ic];
            b.c[j] = ok ? c : -1;
            b.v[j] = ok ? v : 0.0;
        }
        const int32_t ri = ridx[h.row];
        const double d = dg[h.row];
        b.ri = has_ri ? ri : h.row;
        b.d = has_d ? d : 1.0;
    }
};

// Sync-free: x_i = (rhs_i - sum_j T_ij x_j) / diag_i  (diag == nullptr: unit), rhs_i = rhs[rhs_idx[i]]
// when rhs_idx is given. The factor is stored in SOLVE ORDER (host-built): position k holds row
// krow[k] with entries [krp[k], krp[k+1]) of kci/kva, so a wave's rows stream. Wave w takes positions
// w, w+W, ... and software-pipelines them: while it waits on the dependencies of position k it already
// has position k+W's row, entries, right-hand side and diagonal in flight (stage B) and position
// k+2W's row header (stage A), so a row costs one hand-off round trip instead of a chain of dependent
// HBM loads (order -> rowptr -> entries -> rhs index -> rhs). Its loads stay under lane tests: the
// branch-free form of the LDS kernel below (SfSrc) measured 27.0 -> 27.9-28.9 ms on configs[2]'s ILU
// apply (profiles/r3_grid_phase_probe.txt), where the hand-off, not the compiler's waits, bounds a row.
struct SfRow {
    int32_t row, s, e, c[kSfChunks];
    double v[kSfChunks], b, d;
};

__device__ __forceinline__ void sptrsv_rows(int64_t n, const int32_t *__restrict__ krp, const int32_t *__restrict__ kci,
                                            const double *__restrict__ kva, const double *__restrict__ diag,
                                            const double *__restrict__ rhs, const int32_t *__restrict__ rhs_idx, double *x,
                                            int32_t *err, const int32_t *__restrict__ krow, int64_t wave, int64_t W) {
    const int lane = threadIdx.x & 63;
    if (wave >= n) return;
    auto head = [&](int64_t k, SfHead &h) {
        if (k < n) {
            h.row = krow[k];
            h.s = krp[k];
            h.e = krp[k + 1];
        }
    };
    auto body = [&](int64_t k, const SfHead &h, SfRow &b) {
        if (k < n) {
            b.row = h.row;
            b.s = h.s;
            b.e = h.e;
#pragma unroll
            for (int j = 0; j < kSfChunks; ++j) {
                const int32_t idx = h.s + 64 * j + lane;
                b.c[j] = idx < h.e ? kci[idx] : -1;
                b.v[j] = idx < h.e ? kva[idx] : 0.0;
            }
            if (lane == 0) {
                b.b = rhs[rhs_idx ? rhs_idx[h.row] : h.row];
                b.d = diag ? diag[h.row] : 1.0;
            }
        }
    };
    SfHead ha, hb;
    SfRow cur, nxt;
    head(wave, ha);
    body(wave, ha, cur);
    head(wave + W, hb);
    for (int64_t k = wave; k < n; k += W) {
        // the first poll of this row goes out before the prefetches, so waiting for it does not
        // wait for them (loads complete in order)
        uint64_t bits[kSfChunks];
#pragma unroll
        for (int j = 0; j < kSfChunks; ++j)
            bits[j] = cur.c[j] >= 0 ? __hip_atomic_load(reinterpret_cast<const uint64_t *>(x + cur.c[j]),
                                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                    : 0;
        body(k + W, hb, nxt);       // stage B of k+W (its header arrived an iteration ago)
        head(k + 2 * W, hb);        // stage A of k+2W
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kSfChunks; ++j)   // lane's entries in stored order: lane, lane+64, ...
            if (cur.c[j] >= 0) {
                double xv = __longlong_as_double((long long)bits[j]);
                if (is_sentinel(xv)) xv = wait_pub(x + cur.c[j], err);
                acc = fma(cur.v[j], xv, acc);
            }
        // longer rows: kSfTail chunks of entries, then their x values, in flight at once
        for (int32_t base = cur.s + 64 * kSfChunks; base < cur.e; base += 64 * kSfTail) {
            int32_t tc[kSfTail];
            double tv[kSfTail];
            uint64_t tb[kSfTail];
#pragma unroll
            for (int t = 0; t < kSfTail; ++t) {
                const int32_t idx = base + 64 * t + lane;
                tc[t] = idx < cur.e ? kci[idx] : -1;
                tv[t] = idx < cur.e ? kva[idx] : 0.0;
            }
#pragma unroll
            for (int t = 0; t < kSfTail; ++t)
                tb[t] = tc[t] >= 0 ? __hip_atomic_load(reinterpret_cast<const uint64_t *>(x + tc[t]), __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT)
                                   : 0;
#pragma unroll
            for (int t = 0; t < kSfTail; ++t)
                if (tc[t] >= 0) {
                    double xv = __longlong_as_double((long long)tb[t]);
                    if (is_sentinel(xv)) xv = wait_pub(x + tc[t], err);
                    acc = fma(tv[t], xv, acc);
                }
        }
        const double sum = row_total(acc);
        if (lane == 0) {
            double r = cur.b - sum;
            if (diag) r = r / cur.d;
            store_pub(x + cur.row, r);
        }
        cur = nxt;
    }
}

__global__ __launch_bounds__(kBlock) void sptrsv_kernel(int64_t n, const int32_t *__restrict__ krp,
                                                        const int32_t *__restrict__ kci, const double *__restrict__ kva,
                                                        const double *__restrict__ diag, const double *__restrict__ rhs,
                                                        const int32_t *__restrict__ rhs_idx, double *x,
                                                        int32_t *err, const int32_t *__restrict__ krow,
                                                        uint32_t *sched) {
    // positions dealt over the waves of the workgroups that enrolled (sched_enroll), not over the grid
    uint32_t R = 0;
    const int rank = sched_enroll(sched, &R, err);
    if (rank >= 0) sptrsv_rows(n, krp, kci, kva, diag, rhs, rhs_idx, x, err, krow, (int64_t)rank * kWaves + (threadIdx.x >> 6),
                               (int64_t)R * kWaves);
    sched_leave(sched);
}

// LDS-resident: a factor small enough for x to live in LDS (the AMG coarse LU: 16.6k rows, 3008
// levels, ~140 entries per row) is solved by ONE workgroup of 16 waves running the sync-free
// schedule above with x in LDS: a dependency hand-off is an LDS write seen by another wave's LDS
// poll (~0.1 us) instead of a device-scope store seen by a polling load (~1-2 us). Each wave still
// prefetches its next rows' entries from HBM while it waits. x is copied out at the end.
constexpr int kLdsThreads = 1024;
constexpr int kLdsTail = 8;
constexpr int kLdsDepth = 3;   // rows in flight per wave (PSK_LDS_DEPTH=1..3 overrides)

template <int D>
__global__ __launch_bounds__(kLdsThreads) void sptrsv_lds_kernel(int64_t n, const int32_t *__restrict__ krp,
                                                                 const int32_t *__restrict__ kci,
                                                                 const double *__restrict__ kva,
                                                                 const double *__restrict__ diag,
                                                                 const double *__restrict__ rhs,
                                                                 const int32_t *__restrict__ rhs_idx, double *x,
                                                                 int32_t *err, const int32_t *__restrict__ krow) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t *xs = reinterpret_cast<uint64_t *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6, W = kLdsThreads / 64;
    for (int64_t i = tid; i < n; i += kLdsThreads) xs[i] = kSentinel;
    __syncthreads();
    auto lds_wait = [&](int32_t c) -> double {
        uint64_t b = __hip_atomic_load(xs + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        int64_t spins = 0;
        while (b == kSentinel) {
            if (++spins > kMaxSpins) {
                atomicExch(err, 1);
                return 0.0;
            }
            __builtin_amdgcn_s_sleep(1);
            b = __hip_atomic_load(xs + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return __longlong_as_double((long long)b);
    };
    const int32_t nnz = krp[n];
    if (nnz == 0) {   // diagonal factor: no dependencies
        for (int64_t k = wave; k < n; k += W) {
            const int32_t row = krow[k];
            double r = rhs[rhs_idx ? rhs_idx[row] : row];
            if (diag) r = r / diag[row];
            if (lane == 0) x[row] = r;
        }
        return;
    }
    const SfSrc src{n, nnz - 1, krp, kci, krow, rhs_idx ? rhs_idx : krow, kva, diag ? diag : rhs,
                    rhs_idx != nullptr, diag != nullptr, opaque_zero()};
    // register ring of D rows per wave: row k's entries are loaded D rows (D*W positions) before
    // it is solved and its header 2D rows before, so a wave keeps D rows of HBM loads in flight
    // while it waits on LDS hand-offs (one row in flight cost one HBM round trip per row); all of
    // them branch-free (see SfSrc), so the compiler's vmcnt waits leave them in flight
    SfHead hq[D];
    SfBody bq[D];
#pragma unroll
    for (int t = 0; t < D; ++t) src.head(wave + t * W, hq[t]);
#pragma unroll
    for (int t = 0; t < D; ++t) src.body(hq[t], bq[t], lane);
#pragma unroll
    for (int t = 0; t < D; ++t) src.head(wave + (D + t) * W, hq[t]);
    for (int64_t k0 = wave; k0 < n; k0 += D * W) {
#pragma unroll
        for (int t = 0; t < D; ++t) {
            const int64_t k = k0 + t * W;
            if (k >= n) break;
            const SfBody cur = bq[t];
            const double bv = rhs[cur.ri];   // goes out before the prefetches (loads complete in order)
            src.body(hq[t], bq[t], lane);
            src.head(k + 2 * D * W, hq[t]);
            // all of this row's first LDS reads go out together; only a sentinel among them waits
            uint64_t bits[kSfChunks];
#pragma unroll
            for (int j = 0; j < kSfChunks; ++j)
                bits[j] = __hip_atomic_load(xs + (cur.c[j] >= 0 ? cur.c[j] : 0), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_WORKGROUP);
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < kSfChunks; ++j)   // lane's entries in stored order: lane, lane+64, ...
                if (cur.c[j] >= 0)
                    acc = fma(cur.v[j],
                              bits[j] == kSentinel ? lds_wait(cur.c[j]) : __longlong_as_double((long long)bits[j]), acc);
            // longer rows (the dense tail of an LU factor, uniform): kLdsTail chunks of entries in flight at once
            if (cur.e - cur.s > 64 * kSfChunks) {
                for (int32_t base = cur.s + 64 * kSfChunks; base < cur.e; base += 64 * kLdsTail) {
                    int32_t tc[kLdsTail];
                    double tv[kLdsTail];
                    uint64_t tb[kLdsTail];
#pragma unroll
                    for (int u = 0; u < kLdsTail; ++u) {
                        const int32_t idx = base + 64 * u + lane;
                        tc[u] = idx < cur.e ? kci[idx] : -1;
                        tv[u] = idx < cur.e ? kva[idx] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < kLdsTail; ++u)
                        tb[u] = tc[u] >= 0 ? __hip_atomic_load(xs + tc[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0;
#pragma unroll
                    for (int u = 0; u < kLdsTail; ++u)
                        if (tc[u] >= 0)
                            acc = fma(tv[u], tb[u] == kSentinel ? lds_wait(tc[u]) : __longlong_as_double((long long)tb[u]),
                                      acc);
                }
                drain_vm();
            }
            const double sum = row_total(acc);
            double r = bv - sum;
            if (diag) r = r / cur.d;
            // every lane: the same value to the same LDS word
            __hip_atomic_store(xs + cur.row, (uint64_t)__double_as_longlong(r), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    for (int64_t i = tid; i < n; i += kLdsThreads) x[i] = __longlong_as_double((long long)xs[i]);
}

// Sync-free grid: every resident slot the occupancy API reports minus one workgroup per CU (the
// hardware admits one fewer than the API at some SGPR counts, MI355X_MICROARCH.md "Residency"); all
// waves must be co-resident, since a row's wave may wait on any earlier position. The spin-waiting
// schedules (sync-free, band, partitioned) size their grids to fit and launch them plainly: a
// cooperative launch adds nothing they use (no grid barrier), and it left HIP holding per-process
// state whose teardown in exit() faulted under rocprofv3 (profiles/r4_exit_fault.txt). Every wait is
// bounded, so a workgroup that never became resident would surface as a reported error, not a hang.
int syncfree_grid(const Context *c) {
    static int per_cu = -1;
    if (per_cu < 0) {
        int api = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&api, reinterpret_cast<const void *>(&sptrsv_kernel), kBlock,
                                                         0) != hipSuccess)
            api = 2;
        per_cu = std::max(1, std::min(api, 8) - 1);
    }
    return c->num_cus * per_cu;
}

int launch_syncfree(const Context *c, int64_t n, const TriFactor &T, const double *rhs, const int32_t *rhs_idx,
                    double *x, int32_t *err, hipStream_t s) {
    const int32_t *rp = T.rowptr, *ci = T.colidx, *ord = T.order;
    const double *va = T.vals, *dg = T.diag;
    uint32_t *sch = T.sched;
    void *args[] = {&n, &rp, &ci, &va, &dg, &rhs, &rhs_idx, &x, &err, &ord, &sch};
    PSK_HIP(hipLaunchKernel(reinterpret_cast<const void *>(&sptrsv_kernel), dim3(syncfree_grid(c)), dim3(kBlock), args, 0, s));
    return PSK_OK;
}

int launch_lds(const Context *c, int64_t n, const TriFactor &T, const double *rhs, const int32_t *rhs_idx,
               double *x, int32_t *err, hipStream_t s) {
    constexpr int depth = kLdsDepth;
    const void *k = depth <= 1   ? reinterpret_cast<const void *>(&sptrsv_lds_kernel<1>)
                    : depth == 2 ? reinterpret_cast<const void *>(&sptrsv_lds_kernel<2>)
                                 : reinterpret_cast<const void *>(&sptrsv_lds_kernel<3>);   // 4 spills
    const int32_t *rp = T.rowptr, *ci = T.colidx, *ord = T.order;
    const double *va = T.vals, *dg = T.diag;
    void *args[] = {&n, &rp, &ci, &va, &dg, &rhs, &rhs_idx, &x, &err, &ord};
    PSK_HIP(hipLaunchKernel(k, dim3(1), dim3(kLdsThreads), args, (size_t)n * sizeof(double), s));
    return PSK_OK;
}

}  // namespace psk
