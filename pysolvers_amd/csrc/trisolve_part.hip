// trisolve_part.hip — the partitioned schedule.
//
// Partitioned (sptrsv_part_kernel): the rows are cut into P strips of the NATURAL index (the
// matrix's own numbering before the factorisation's permutations: for ILU the original equation /
// unknown of every factor row), one strip per workgroup of 16 waves, one workgroup per CU. A strip of
// a mesh-like matrix is a band of the mesh, so most dependencies of its rows are rows of the same
// strip: those hand-offs go through LDS (~0.1 us) instead of a device-scope store seen by a polling
// load (~1 us). Each workgroup runs its rows in ASAP order (earliest finish under the cost model,
// host-computed: a topological order), dealt round-robin to its waves; every wave runs the sync-free
// row pipeline above. Entry codes: c >= 0 = another strip's row, read from x with the sentinel
// protocol; c < 0 = the strip's own row at local position qd = -c-1, read from an LDS cache of
// kPartSlots results (slot qd mod kPartSlots) whose tag is the local position it holds. Rows write x
// (the output) and the cache; the tag goes to kPartWriting while a slot is rewritten, so a reader
// that sees the same tag before and after reading the value has that row's value, a newer tag means
// the slot was reused (the value is then read from x), an older one that the row is not done. Same
// per-row arithmetic as sync-free (same entry order, lane partials, row_total), so bit-identical to it.
// Progress: all P workgroups are co-resident (one per CU, P <= CUs); the globally ASAP-first unsolved
// row has all its dependencies solved and every earlier row of its wave is ASAP-earlier.
#include "trisolve.hpp"

namespace psk {

constexpr int32_t kPartPad = INT32_MIN;         // padding lane
constexpr int32_t kPartEmpty = -1, kPartWriting = -2;
constexpr size_t kPartLds = (size_t)kPartSlots * (sizeof(double) + sizeof(int32_t));

// Every load of the row pipeline is unconditional (clamped positions, entry arrays padded by
// kPartPadEntries on the host, the right-hand side pre-gathered): a load under a divergent branch
// makes the compiler wait for ALL outstanding loads (vmcnt(0)) at the join, which would serialise
// the prefetch of the next rows behind this row's dependency polls.
#ifdef PSK_PART_PROF
// development probe: [0] wave cycles, [1] local-wait cycles, [2] remote-wait cycles, [3] rows,
// [4] local waits, [5] remote waits, [6] slot reuses, [7] max wave cycles (summed over the launch)
__device__ unsigned long long g_part_prof[8];
extern "C" int psk_part_prof_read(unsigned long long *out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_part_prof), sizeof(g_part_prof)) != hipSuccess) return -1;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_part_prof), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
// per-position phase stamps (clock64) of the first 2^17 positions, 8 words each: [0] the row's turn
// (its wave's pipeline loads for later rows issued), [1] local (LDS) dependencies read, [2] every
// entry's x value in and the lane partial summed (remote polls included), [3] row total (DPP),
// [4] quotient, [5] x and the LDS cache written (issued); [6] 1 if the spin waited, [7] spins
constexpr int kPartTraceWords = 8;
__device__ unsigned long long g_part_trace[kPartTraceWords << 17];
extern "C" int psk_part_trace_read(unsigned long long *out, int64_t n) {
    if (n > (1 << 17)) n = 1 << 17;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_part_trace), (size_t)n * 8 * kPartTraceWords) == hipSuccess ? 0 : -1;
}
#define PART_PROF(...) __VA_ARGS__
#else
#define PART_PROF(...)
#endif
struct PtBody {
    int32_t row, s, e, c[kPtChunks];
    double v[kPtChunks], b, d;
};

template <bool UNIT>
__global__ __launch_bounds__(kPartThreads) void sptrsv_part_kernel(
    const int64_t *__restrict__ seg, const int32_t *__restrict__ krp, const int32_t *__restrict__ kcode,
    const double *__restrict__ kva, const double *__restrict__ diag, const double *__restrict__ rhs, double *x,
    int32_t *err, const int32_t *__restrict__ krow) {
    extern __shared__ __align__(16) unsigned char smem[];
    // LDS accesses are workgroup-scope relaxed atomics: ds_read / ds_write in program order, no waits
    // between them (a wave's LDS operations execute in issue order)
    uint64_t *sv = reinterpret_cast<uint64_t *>(smem);
    int32_t *st = reinterpret_cast<int32_t *>(smem + kPartSlots * sizeof(double));
    auto ld_tag = [&](int32_t s) { return __hip_atomic_load(st + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    auto ld_val = [&](int32_t s) {
        return __longlong_as_double((long long)__hip_atomic_load(sv + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    };
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6;
    for (int i = tid; i < kPartSlots; i += kPartThreads) st[i] = kPartEmpty;   // before the barrier: plain
    __syncthreads();
    const int64_t base = seg[blockIdx.x], R = seg[blockIdx.x + 1] - base;
    if (wave >= R) return;
    PART_PROF(const unsigned long long pt0 = clock64(); unsigned long long plw = 0, prw = 0, pnl = 0, pnr = 0, pev = 0;)
    auto head = [&](int64_t q, SfHead &h) {   // q >= R: a valid position whose row is never used
        const int64_t k = base + (q < R ? q : R - 1);
        h.row = krow[k];
        h.s = krp[k];
        h.e = krp[k + 1];
    };
    auto body = [&](const SfHead &h, PtBody &b) {
        b.row = h.row;
        b.s = h.s;
        b.e = h.e;
#pragma unroll
        for (int j = 0; j < kPtChunks; ++j) {
            const int32_t idx = h.s + 64 * j + lane;   // < nnz + kPartPadEntries
            const int32_t c = kcode[idx];
            b.v[j] = kva[idx];
            b.c[j] = idx < h.e ? c : kPartPad;
        }
        b.b = rhs[h.row];
        b.d = UNIT ? 1.0 : diag[h.row];
    };
    // an entry's x value: bits/t1/v/t2 are its first reads (issued together for the whole row)
    auto resolve = [&](int32_t c, uint64_t bits, int32_t t1, double v, int32_t t2) -> double {
        if (c >= 0) {
            const double xv = __longlong_as_double((long long)bits);
            return is_sentinel(xv) ? wait_pub(x + c, err) : xv;
        }
        const int32_t qd = ~c, slot = qd & (kPartSlots - 1);   // ~c == -c-1
        int64_t spins = 0;
        PART_PROF(const unsigned long long w0 = clock64(); if (!(t1 == qd && t2 == qd)) pnl++;)
        while (!(t1 == qd && t2 == qd)) {
            if (t1 > qd || t1 == qd) {
                PART_PROF(pev++;)
                return wait_pub(x + krow[base + qd], err);   // slot reused: x has it
            }
            if (++spins > kMaxSpins) {
                atomicExch(err, 2);
                return 0.0;
            }
            __builtin_amdgcn_s_sleep(1);
            t1 = ld_tag(slot);
            v = ld_val(slot);
            t2 = ld_tag(slot);
        }
        PART_PROF(plw += clock64() - w0;)
        return v;
    };
    // Software pipeline over the wave's rows u = 0, 1, ... (position wave + u*W): in iteration u the
    // wave issues the first x polls of row u+1, the entries of row u+3 and the header of row u+5, then
    // resolves row u. Every load a step waits for was issued at least one iteration earlier and the
    // polls go out first, so (loads completing in order) resolving row u waits only for its own polls
    // and what was issued two iterations before: a wave keeps ~3 rows of loads in flight and a row
    // whose dependencies are done costs no memory round trip of its own. Rings: bodies and headers 4,
    // polls 2; the loop is unrolled by 4 so every ring index is a constant.
    auto poll = [&](const PtBody &b, uint64_t *bits) {   // first polls of the remote entries
#pragma unroll
        for (int j = 0; j < kPtChunks; ++j)
            bits[j] = __hip_atomic_load(reinterpret_cast<const uint64_t *>(x + (b.c[j] >= 0 ? b.c[j] : 0)),
                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    constexpr int64_t W = kPartWaves;
    SfHead H[4];
    PtBody B[4];
    uint64_t P[2][kPtChunks];
    head(wave, H[0]);
    head(wave + W, H[1]);
    head(wave + 2 * W, H[2]);
    body(H[0], B[0]);
    body(H[1], B[1]);
    body(H[2], B[2]);
    head(wave + 3 * W, H[3]);
    head(wave + 4 * W, H[0]);
    poll(B[0], P[0]);
    for (int64_t q0 = wave; q0 < R; q0 += 4 * W) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t q = q0 + t * W;
            if (q >= R) break;
            poll(B[(t + 1) & 3], P[(t + 1) & 1]);   // row u+1 (entries issued two iterations ago)
            body(H[(t + 3) & 3], B[(t + 3) & 3]);   // row u+3 (header issued two iterations ago)
            head(q + 5 * W, H[(t + 1) & 3]);         // row u+5
            const PtBody &cur = B[t];
            const uint64_t *pc = P[t & 1];
            PART_PROF(const unsigned long long ph0 = clock64(); unsigned long long nspin = 0;)
            // x values of the row's register chunks: remote ones from the early polls, local ones from
            // the LDS cache, polled by the whole wave until every local entry is present (the spin's
            // control flow is uniform); reused slots and unpublished remote values then wait on x
            double xv[kPtChunks];
            bool pend[kPtChunks];
#pragma unroll
            for (int j = 0; j < kPtChunks; ++j) {
                xv[j] = 0.0;   // remote values are read from the polls only below (no wait for them here)
                pend[j] = cur.c[j] < 0 && cur.c[j] != kPartPad;   // local, not yet read
            }
            PART_PROF(const unsigned long long w0 = clock64(); bool waited = false;)
            for (int64_t spins = 0;; ++spins) {
                bool left = false;
#pragma unroll
                for (int j = 0; j < kPtChunks; ++j)
                    if (pend[j]) {
                        const int32_t qd = ~cur.c[j], slot = qd & (kPartSlots - 1);
                        const int32_t t1 = ld_tag(slot);
                        const double v = ld_val(slot);
                        const int32_t t2 = ld_tag(slot);
                        if (t1 == qd && t2 == qd) {
                            xv[j] = v;
                            pend[j] = false;
                        } else if (t1 >= qd) {   // slot reused (or being rewritten): x holds the value
                            xv[j] = wait_pub(x + krow[base + qd], err);
                            pend[j] = false;
                            PART_PROF(pev++;)
                        } else {
                            left = true;
                        }
                    }
                if (!__any(left)) break;
                if (spins > kMaxSpins) {
                    if (lane == 0) atomicExch(err, 2);
                    break;
                }
                PART_PROF(waited = true; ++nspin;)
#ifndef PSK_PART_SLEEP
#define PSK_PART_SLEEP 1
#endif
                __builtin_amdgcn_s_sleep(PSK_PART_SLEEP);
            }
            PART_PROF(if (waited) { plw += clock64() - w0; pnl++; }
                      for (int j = 0; j < kPtChunks; ++j) __asm__ volatile("" ::"v"(xv[j]));
                      const unsigned long long ph1 = clock64();)
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < kPtChunks; ++j) {
                const int32_t c = cur.c[j];
                if (c == kPartPad) continue;
                if (c >= 0) {
                    xv[j] = __longlong_as_double((long long)pc[j]);
                    if (is_sentinel(xv[j])) {
                        PART_PROF(const unsigned long long w1 = clock64(); pnr++;)
                        xv[j] = wait_pub(x + c, err);
                        PART_PROF(prw += clock64() - w1;)
                    }
                }
                acc = fma(cur.v[j], xv[j], acc);
            }
            for (int32_t b0 = cur.s + 64 * kPtChunks; b0 < cur.e; b0 += 64 * kSfTail) {   // long rows
                int32_t tc[kSfTail];
                double tv[kSfTail];
#pragma unroll
                for (int u = 0; u < kSfTail; ++u) {
                    const int32_t idx = b0 + 64 * u + lane;
                    tc[u] = idx < cur.e ? kcode[idx] : kPartPad;
                    tv[u] = idx < cur.e ? kva[idx] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < kSfTail; ++u)
                    if (tc[u] != kPartPad) {
                        const int32_t c = tc[u], slot = ~c & (kPartSlots - 1);
                        const uint64_t bt = c >= 0 ? __hip_atomic_load(reinterpret_cast<const uint64_t *>(x + c),
                                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                   : 0;
                        const int32_t a1 = c < 0 ? ld_tag(slot) : 0;
                        const double vv = c < 0 ? ld_val(slot) : 0.0;
                        const int32_t a2 = c < 0 ? ld_tag(slot) : 0;
                        acc = fma(tv[u], resolve(c, bt, a1, vv, a2), acc);
                    }
            }
            PART_PROF(__asm__ volatile("" ::"v"(acc)); const unsigned long long ph2 = clock64();)
            const double sum = row_total(acc);
            PART_PROF(__asm__ volatile("" ::"v"(sum)); const unsigned long long ph3 = clock64();)
            if (lane == 0) {
                double r = cur.b - sum;
                if (!UNIT) r = r / cur.d;
                PART_PROF(__asm__ volatile("" ::"v"(r)); const unsigned long long ph4 = clock64();)
                store_pub(x + cur.row, r);
                const int32_t slot = (int32_t)(q & (kPartSlots - 1));
                __hip_atomic_store(st + slot, kPartWriting, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_store(sv + slot, (uint64_t)__double_as_longlong(r), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_store(st + slot, (int32_t)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                PART_PROF(if (base + q < (1 << 17)) {
                    const unsigned long long ph5 = clock64();
                    unsigned long long *tr = g_part_trace + kPartTraceWords * (base + q);
                    tr[0] = ph0;
                    tr[1] = ph1;
                    tr[2] = ph2;
                    tr[3] = ph3;
                    tr[4] = ph4;
                    tr[5] = ph5;
                    tr[6] = waited ? 1 : 0;
                    tr[7] = nspin;
                })
            }
        }
    }
#ifdef PSK_PART_PROF
    unsigned long long vals[6] = {clock64() - pt0, plw, prw, pnl, pnr, pev};
    for (int i = 0; i < 6; ++i)
        for (int o = 32; o > 0; o >>= 1) vals[i] = max(vals[i], (unsigned long long)__shfl_xor((long long)vals[i], o));
    if (lane == 0) {
        atomicAdd(&g_part_prof[0], vals[0]);
        atomicAdd(&g_part_prof[1], vals[1]);
        atomicAdd(&g_part_prof[2], vals[2]);
        atomicAdd(&g_part_prof[4], vals[3]);
        atomicAdd(&g_part_prof[5], vals[4]);
        atomicAdd(&g_part_prof[6], vals[5]);
        atomicMax(&g_part_prof[7], vals[0]);
        atomicAdd(&g_part_prof[3], (unsigned long long)((R - wave + kPartWaves - 1) / kPartWaves));
    }
#endif
}

int launch_part(const Context *c, int64_t n, const TriFactor &T, const double *rhs, const int32_t *rhs_idx,
                double *x, int32_t *err, hipStream_t s) {
    const double *dg = T.diag;
    if (rhs_idx) return fail(PSK_ERR_ARG, "part schedule: gathered right-hand side (internal)");
    const void *k = dg ? reinterpret_cast<const void *>(&sptrsv_part_kernel<false>)
                       : reinterpret_cast<const void *>(&sptrsv_part_kernel<true>);
    const int64_t *sg = T.part.seg;
    const int32_t *prp = T.part.rp, *pc = T.part.code, *prow = T.part.row;
    const double *pv = T.part.va;
    void *args[] = {&sg, &prp, &pc, &pv, &dg, &rhs, &x, &err, &prow};
    PSK_HIP(hipLaunchKernel(k, dim3(T.part.P), dim3(kPartThreads), args, (unsigned)kPartLds, s));
    return PSK_OK;
}

}  // namespace psk
