// ilu0.hip — ILU(0) factored on the device (psk_csr_ilu0) and handed to the triangular-solve chain
// (psk_prec_create_ilu0). Replaces nothing in the reference, whose incomplete factorisations are SuperLU's
// (ILUTPreconditioner.py:51-53, ICPreconditioner.py): ILU(0) keeps A's own pattern, so the factors cost 12 B per
// entry of A and a 5-point grid of m lines has 2m - 1 dependency levels.
//
// The factorisation, to the bit. A is square with at most one stored entry per (row, column) and a stored diagonal
// entry in every row; v = the values of the copy whose rows are in ascending column order. For i = 0 .. n-1:
//   for each entry e of row i with column k < i, in ascending k:
//     l = v[e] / v[diag(k)] (IEEE division; row k is final), v[e] = l,
//     for each entry f of row k with column j > k: if row i stores column j at q, v[q] = v[q] - l * v[f]
//     (the product rounded, then the difference: the library is built with -ffp-contract=off);
//   row i's pivot v[diag(i)] is in error when it is 0.0 or not finite.
// F = that copy: L = strict-lower(F) with a unit diagonal, U = upper(F) with the diagonal. Every v[q] receives its
// updates in ascending k whatever the schedule below, so the result does not depend on the launch geometry.
//
// Kernels (gfx950, wave64; no floating-point atomics, no workgroup or wave waits on another, every loop bounded by
// a row length):
//  * ilu0_sort_kernel: ONE WAVE PER ROW ranks the row's entries by column (quadratic in the row length, as
//    spgemm.hip's transpose ranks its segments) into the working copy, records the diagonal's position and flags a
//    duplicate column, a missing diagonal and a column outside [0, n).
//  * ilu0_level_kernel<G>: ONE LAUNCH PER DEPENDENCY LEVEL of strict-lower(A) (the host planner's level_order,
//    trisolve_plan.hip), enqueued back to back with no host synchronisation between them; the rows of a level are
//    independent and every row they read was finished by an earlier launch, so the launch boundary is the only
//    ordering. G lanes (1, 4, 16 or 64, from the mean row length) share a row: lane t OWNS the row's entries t, t + G,
//    ... and is the only lane that reads or writes their values, so no lane depends on another lane's store. For
//    each k < i in turn the owner of that entry forms l, the group gets it by a register shuffle, and every lane looks
//    its owned columns j > k up in row k's upper part by binary search. A row of any length is correct (506 entries
//    in the tests); long rows are slow, not wrong.
//    Bytes: a level streams its rows (12 B per entry) and, per lower entry, the upper part of the row it names
//    (served by L2: the rows of the previous levels); the time is launches and dependent-load latency, not bandwidth.
//  * a bad pivot: the smallest such row into one device word by an integer atomic min; later levels still run (inf
//    and NaN are harmless) and the host reads the word once at the end.
#include "trisolve.hpp"

#include <chrono>
#include <climits>
#include <cstdlib>

namespace psk {

// where the last psk_csr_ilu0 / psk_prec_create_ilu0 of this process spent its time (psk_lab_ilu0_timing)
static Ilu0Timing g_timing;
const Ilu0Timing &ilu0_last_timing() { return g_timing; }

namespace {

constexpr int32_t kFlagDup = 1, kFlagNoDiag = 2, kFlagRange = 4;

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
            return fail(PSK_ERR_ALLOC, "ilu0: hipMalloc of a temporary failed");
        p.push_back(q);
        *out = static_cast<T *>(q);
        return PSK_OK;
    }
};

struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap_ms() {
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};

// HIP refuses a grid dimension of 2^32 threads or more: workgroups beyond 2^20 go to a second dimension
constexpr int64_t kGridX = (int64_t)1 << 20;
dim3 grid_for_blocks(int64_t nb) {
    return nb <= kGridX ? dim3((unsigned)(nb > 0 ? nb : 1)) : dim3((unsigned)kGridX, (unsigned)((nb + kGridX - 1) / kGridX));
}
__device__ __forceinline__ int64_t block_index() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__global__ __launch_bounds__(kBlock) void ilu0_sort_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ col,
                                                           const double *__restrict__ val, int32_t *__restrict__ fcol,
                                                           double *__restrict__ fval, int32_t *__restrict__ diag,
                                                           int32_t *flag) {
    const int lane = threadIdx.x & 63;
    const int64_t i = block_index() * kWaves + (threadIdx.x >> 6);
    if (i >= n) return;   // wave-uniform
    const int32_t s0 = rowptr[i], L = rowptr[i + 1] - s0;
    int32_t bad = 0;
    bool found = false;
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
        fval[s0 + rank] = val[s0 + q];
        if (c == i) {
            diag[i] = s0 + rank;
            found = true;
        }
    }
    if (!__any(found ? 1 : 0) && lane == 0) bad |= kFlagNoDiag;
    if (bad) atomicOr(flag, bad);
}

// rows[0..nrows): one dependency level. v is read and written (no __restrict__): a lane writes only the entries it owns.
template <int G>
__global__ __launch_bounds__(kBlock) void ilu0_level_kernel(const int32_t *__restrict__ rows, int64_t nrows,
                                                            const int32_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ col,
                                                            const int32_t *__restrict__ diag, double *v,
                                                            int32_t *bad_row) {
    const int64_t gid = block_index() * kBlock + threadIdx.x;
    const int64_t grp = gid / G;
    const int32_t t = (int32_t)(gid % G);
    if (grp >= nrows) return;   // the whole group leaves together
    const int32_t i = rows[grp];
    const int32_t r0 = rowptr[i], r1 = rowptr[i + 1], d = diag[i];
    for (int32_t e = r0; e < d; ++e) {   // bounds uniform over the group
        const int32_t k = col[e], dk = diag[k];
        const int32_t owner = (e - r0) & (G - 1);
        double l = 0.0;
        if (t == owner) {
            l = v[e] / v[dk];
            v[e] = l;
        }
        if (G > 1) l = __shfl(l, owner, G);
        const int32_t u0 = dk + 1, u1 = rowptr[k + 1];
        int32_t q = r0 + t;   // this lane's first owned entry after e
        if (q <= e) q += ((e - q) / G + 1) * G;
        for (; q < r1; q += G) {
            const int32_t j = col[q];
            int32_t lo = u0, hi = u1;
            while (lo < hi) {
                const int32_t mid = lo + ((hi - lo) >> 1);
                if (col[mid] < j) lo = mid + 1;
                else hi = mid;
            }
            if (lo < u1 && col[lo] == j) v[q] = v[q] - l * v[lo];
        }
    }
    if (t == ((d - r0) & (G - 1))) {
        const double piv = v[d];
        if (piv == 0.0 || !__builtin_isfinite(piv)) atomicMin(bad_row, i);
    }
}

template <int G>
void launch_level(const int32_t *rows, int64_t nrows, const psk_csr *F, const int32_t *diag, int32_t *bad_row,
                  hipStream_t s) {
    const int64_t nb = (nrows * G + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ilu0_level_kernel<G>, grid_for_blocks(nb), dim3(kBlock), 0, s, rows, nrows,
                       (const int32_t *)F->rowptr, (const int32_t *)F->colidx, diag, F->vals, bad_row);
}

// lanes per row from the mean row length (PSK_ILU0_WIDTH=1|4|16|64 overrides: tests of the geometry independence)
int group_width(int64_t n, int64_t nnz) {
    if (const char *e = std::getenv("PSK_ILU0_WIDTH")) {
        const int w = std::atoi(e);
        if (w == 1 || w == 4 || w == 16 || w == 64) return w;
    }
    const double mean = n > 0 ? (double)nnz / (double)n : 0.0;
    return mean <= 2.0 ? 1 : mean <= 8.0 ? 4 : mean <= 32.0 ? 16 : 64;
}

// the sorted pattern on the host, kept for the caller that splits the factors
struct HostPattern {
    std::vector<int32_t> rp, ci, diag;
};

// *out is written only on success; hp (nullable) receives the sorted pattern
int ilu0_factor(const psk_csr *A, psk_csr **out, HostPattern *hp) {
    if (!A || !out) return fail(PSK_ERR_ARG, "psk_csr_ilu0: NULL argument");
    if (A->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_ilu0: sharded matrix");
    if (A->n != A->ncols) return fail(PSK_ERR_ARG, "psk_csr_ilu0: A must be square");
    if (A->n == 0 || A->nnz == 0) return fail(PSK_ERR_ARG, "psk_csr_ilu0: A is empty");
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    const int64_t n = A->n, nnz = A->nnz;
    g_timing = Ilu0Timing();
    Clock clk;
    Tmp tmp;
    int32_t *diag, *words, *order;
    PSK_TRY(tmp.get(n, &diag));
    PSK_TRY(tmp.get(2, &words));   // [0] = structure flags, [1] = smallest row with a bad pivot
    PSK_TRY(tmp.get(n, &order));
    psk_csr *F = nullptr;
    PSK_TRY(csr_new_device(n, n, nnz, &F));
    auto work = [&]() -> int {
        const int32_t init[2] = {0, INT32_MAX};
        PSK_HIP(hipMemcpyAsync(words, init, sizeof(init), hipMemcpyHostToDevice, s));
        PSK_HIP(hipMemcpyAsync(F->rowptr, A->rowptr, (size_t)(n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(ilu0_sort_kernel, grid_for_blocks((n + kWaves - 1) / kWaves), dim3(kBlock), 0, s, n,
                           (const int32_t *)A->rowptr, (const int32_t *)A->colidx, (const double *)A->vals, F->colidx,
                           F->vals, diag, words);
        PSK_HIP(hipGetLastError());
        int32_t flags = 0;
        PSK_HIP(hipMemcpyAsync(&flags, words, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipStreamSynchronize(s));
        if (flags & kFlagRange) return fail(PSK_ERR_ARG, "psk_csr_ilu0: column index out of range");
        if (flags & kFlagDup) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_ilu0: duplicate column within a row");
        if (flags & kFlagNoDiag) return fail(PSK_ERR_ARG, "psk_csr_ilu0: a row has no stored diagonal entry");
        g_timing.sort_ms = clk.lap_ms();
        // dependency levels of strict-lower(A) on the host (the planner's level_order)
        HostPattern local;
        HostPattern &P = hp ? *hp : local;
        P.rp.resize((size_t)n + 1);
        P.ci.resize((size_t)nnz);
        P.diag.resize((size_t)n);
        PSK_HIP(hipMemcpyAsync(P.rp.data(), F->rowptr, (size_t)(n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipMemcpyAsync(P.ci.data(), F->colidx, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipMemcpyAsync(P.diag.data(), diag, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PSK_HIP(hipStreamSynchronize(s));
        std::vector<int32_t> ord, lev;
        std::vector<int64_t> lp;
        int64_t nlev = 0;
        {
            HostFactor H;
            H.n = n;
            H.upper = false;
            H.rp.assign((size_t)n + 1, 0);
            for (int64_t i = 0; i < n; ++i) H.rp[i + 1] = H.rp[i] + (P.diag[i] - P.rp[i]);
            H.ci.resize((size_t)H.rp[n]);
            for (int64_t i = 0; i < n; ++i)
                std::copy(P.ci.begin() + P.rp[i], P.ci.begin() + P.diag[i], H.ci.begin() + H.rp[i]);
            level_order(H, ord, lev, nlev);
        }
        lp.assign((size_t)nlev + 1, 0);
        for (int64_t i = 0; i < n; ++i) lp[lev[i] + 1]++;
        for (int64_t l = 0; l < nlev; ++l) lp[l + 1] += lp[l];
        PSK_HIP(hipMemcpyAsync(order, ord.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        PSK_HIP(hipStreamSynchronize(s));
        g_timing.levels_ms = clk.lap_ms();
        g_timing.levels = nlev;
        // numeric phase: one launch per level, back to back
        const int G = group_width(n, nnz);
        g_timing.width = G;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        PSK_HIP(hipEventCreate(&ev0));
        if (hipEventCreate(&ev1) != hipSuccess) {
            (void)hipEventDestroy(ev0);
            return fail(PSK_ERR_HIP, "psk_csr_ilu0: hipEventCreate");
        }
        hipError_t e = hipEventRecord(ev0, s);
        for (int64_t l = 0; l < nlev && e == hipSuccess; ++l) {
            const int32_t *rows = order + lp[l];
            const int64_t nr = lp[l + 1] - lp[l];
            switch (G) {
            case 1: launch_level<1>(rows, nr, F, diag, words + 1, s); break;
            case 4: launch_level<4>(rows, nr, F, diag, words + 1, s); break;
            case 16: launch_level<16>(rows, nr, F, diag, words + 1, s); break;
            default: launch_level<64>(rows, nr, F, diag, words + 1, s); break;
            }
            if ((l & 1023) == 1023) e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(ev1, s);
        int32_t bad = INT32_MAX;
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, words + 1, sizeof(int32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
        (void)hipEventDestroy(ev0);
        (void)hipEventDestroy(ev1);
        if (e != hipSuccess) return fail(PSK_ERR_HIP, std::string("psk_csr_ilu0: ") + hipGetErrorString(e));
        g_timing.numeric_ms = ms;
        (void)clk.lap_ms();
        if (bad != INT32_MAX)
            return fail(PSK_ERR_ARG, "psk_csr_ilu0: zero or non-finite pivot in row " + std::to_string(bad));
        return csr_finish_device(F, s);
    };
    const int rc = work();
    if (rc != PSK_OK) {
        (void)hipStreamSynchronize(s);
        csr_discard(F);
        return rc;
    }
    *out = F;
    return PSK_OK;
}

}  // namespace
}  // namespace psk

using namespace psk;

extern "C" {

int psk_csr_ilu0(const psk_csr *A, psk_csr **F) { return ilu0_factor(A, F, nullptr); }

int psk_prec_create_ilu0(const psk_csr *A, psk_prec **out) {
    if (!out) return fail(PSK_ERR_ARG, "psk_prec_create_ilu0: NULL argument");
    HostPattern P;
    psk_csr *F = nullptr;
    PSK_TRY(ilu0_factor(A, &F, &P));
    Clock clk;
    const int64_t n = F->n, nnz = F->nnz;
    std::vector<double> va((size_t)nnz);
    int rc = psk_csr_download(F, nullptr, nullptr, va.data());
    (void)psk_csr_destroy(F);
    if (rc != PSK_OK) return rc;
    // L = strict-lower(F) (unit diagonal, not stored), U = upper(F) with the diagonal: rows stay column-sorted
    std::vector<int32_t> lrp((size_t)n + 1, 0), urp((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        lrp[i + 1] = lrp[i] + (P.diag[i] - P.rp[i]);
        urp[i + 1] = urp[i] + (P.rp[i + 1] - P.diag[i]);
    }
    std::vector<int32_t> lci((size_t)lrp[n]), uci((size_t)urp[n]);
    std::vector<double> lva((size_t)lrp[n]), uva((size_t)urp[n]);
    for (int64_t i = 0; i < n; ++i) {
        std::copy(P.ci.begin() + P.rp[i], P.ci.begin() + P.diag[i], lci.begin() + lrp[i]);
        std::copy(va.begin() + P.rp[i], va.begin() + P.diag[i], lva.begin() + lrp[i]);
        std::copy(P.ci.begin() + P.diag[i], P.ci.begin() + P.rp[i + 1], uci.begin() + urp[i]);
        std::copy(va.begin() + P.diag[i], va.begin() + P.rp[i + 1], uva.begin() + urp[i]);
    }
    P = HostPattern();
    std::vector<double>().swap(va);
    g_timing.split_ms = clk.lap_ms();
    rc = psk_prec_create_trisolve(n, lrp.data(), lci.data(), lva.data(), 1, urp.data(), uci.data(), uva.data(), 0,
                                  nullptr, nullptr, out);
    g_timing.plan_ms = clk.lap_ms();
    return rc;
}

}  // extern "C"
