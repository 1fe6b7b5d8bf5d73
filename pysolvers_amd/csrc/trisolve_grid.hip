// trisolve_grid.hip — the grid schedule (2-D stencil factors).
//
// Grid: a factor whose dependencies, in solve order q, form a 2-D stencil: with q = y*w + x (w
// positions per line), every off-diagonal entry of row q refers to q' = q - (yd*w + xd) with
// 0 <= yd < 64 lines back and, for the skew chosen by the host, ud = xd + g(y) - g(y - yd) >= 1 steps
// back along u = x + g(y) (the 5-point Gauss-Seidel factor triu(A): (0,1), (1,0), g(y) = y; an
// SA coarse operator of a 2-D grid: up to 2 lines back with diagonal neighbours). The skew may be a
// half integer, g(y) = (sigma2 * y + phase) >> 1 with sigma2 odd: SA level 3 of -FD 4096^2 (2048 lines
// of 1366) has a dependency (1 line, 2 positions ahead) on every other line only, which an integer
// skew can only meet with g(y) = 3y; g(y) = (5y + 1) >> 1 meets it with 13.6% fewer steps. One wave per band
// of 64 lines; lane j owns line y0+j and all lanes advance together along u, so step s solves 64
// rows that do not depend on each other; a dependency on the same band is a read of the LDS ring
// holding the band's last `ring` steps (ring[(s mod ring)*64 + lane]); only lanes j < yd reach into
// the band above, through the published values (pre-filled sentinel, agent-scope store / poll as
// the other schedules), prefetched D steps ahead with everything else a step needs. The critical
// path is the u range (w + g(H) steps) plus one hand-off lag per band, instead of one hand-off
// per dependency level. Per-row arithmetic is the band kernels': fma over the entries in stored
// order from 0.0, then (b - acc) / diag, so results are bit-identical to the band schedule.
#include "trisolve.hpp"

#include <algorithm>

namespace psk {

#ifdef PSK_GRID_PROF
// development probe (tools/grid_probe.py): per band start / end s_memtime, waits and cycles waited
// 8 words per band: start, end, waits on the band above, cycles waited, then the solver's cycles per
// step phase summed over the band: records + rhs ready, LDS ring reads, arithmetic (fma chain and
// division), ring write + x store issued
__device__ unsigned long long g_grid_prof[8192 * 8];
extern "C" int psk_grid_prof_read(unsigned long long *out, int nbands) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_grid_prof), sizeof(unsigned long long) * 8 * (size_t)nbands) ==
                   hipSuccess ? 0 : -1;
}
#endif

// Two waves per band. The SOLVER wave (lanes = the band's 64 lines) advances along u. Its records
// are stored in its access order — slot = (band * S_full + step) * 64 + lane — one 16-B-multiple
// record per slot, so a step's records are one contiguous 64-lane stream, prefetched D steps ahead;
// rhs and x stay in natural order (each lane walks its own line). Dependencies come from ONE LDS ring
// of kGridRing steps x kGridRW columns: columns [8 - maxyd, 8) hold the band above's last maxyd lines,
// written by the POLLER wave as their values get published (64 u-positions polled at a time, the ready
// prefix announced through an LDS counter after every round trip), column 8 + j the solver's lane j; a
// dependency (yd lines, ud steps back) of lane j is column 8 + j - yd of ring row (s - ud) whoever
// produced it. The ring is MIRRORED (every row written at r and r + kGridRing, one ds_write2st64), so a
// dependency's byte address is the step's row base plus a per-entry constant (kept per dictionary
// record): one VALU add per entry instead of the modular row arithmetic and an integer multiply.
// The step is bound by its instruction count (one wave, in order: ~160 instructions per step ran the
// 5-point sweep at ~630 cycles per step), so everything the step does not need per lane is scalar: the
// ring row, the wait test on the band above (a step limit), the index prefetch (a buffer load with a
// scalar offset). The solver's waits are scalar LDS spins. Padding entries (value 0, code 0 = the lane's
// own column of the current row: finite) add exactly +-0 to the fma chain. Per-row arithmetic is the
// band kernels': fma over the entries in stored order from 0.0, then (b - acc) / diag — bit-identical.
// DICT: the records come from a dictionary (TriFactor::grid_dict_n): per lane-step ONE 32-bit index
// load instead of the three record loads (codes, values, diagonal), the dictionary in LDS as one
// 64/128-B record per entry (values, diagonal, RN(1/diagonal), ring offsets), the next step's record
// looked up while the current step's ring reads are in flight.
constexpr int kGridRW = 72;                          // ring columns: 8 for the band above + 64 lanes
constexpr int kGridRing = 128;                       // ring rows (steps); the LDS holds 2 x 128 (mirror)
constexpr uint32_t kGridMirror = kGridRing * kGridRW * 8;   // bytes between a row and its mirror
template <int K>
struct GridDict {   // LDS record of a dictionary entry
    static constexpr int kBytes = K == 8 ? 128 : 64;
    // [0, 8K) values, [8K, 8K + 16) diagonal and RN(1/diagonal), then K uint32 ring offsets
    static constexpr int kDg = 8 * K, kOff = 8 * K + 16;
};
template <int K>
struct GridRec {
    uint32_t off[K];      // byte offset of each entry's ring word from the step's lane base
    double cf[K], d, rd;  // rd = RN(1 / d), DICT only
};
// ring byte offset of a dependency coded ud*64 + yd, from the lane base (lower copy of the current row,
// column 8 + j): the upper copy of row s - ud, column 8 + j - yd
__device__ __forceinline__ uint32_t grid_ring_off(uint32_t c) {
    return (uint32_t)(kGridRing - (int)(c >> 6)) * (kGridRW * 8) - (c & 63) * 8;
}
// (b - acc) / d on the solver's dependency chain without the IEEE division sequence (two
// dependent scale steps, the reciprocal, five fmas and the fix-up): q0 = RN(r * rd) from the
// correctly rounded reciprocal rd = RN(1/d) (computed once per dictionary entry, off the chain), then
// two Markstein corrections q <- RN(q + RN(r - q d) rd) with the remainder exact in an fma. With rd
// correctly rounded, a correction from any q within one ulp of r/d returns RN(r/d), and q0 is within
// 1.5 ulp, so the second correction returns the IEEE quotient; r = +-0 keeps q0 (the signed zero).
// tools/markstein_check.c: 0 mismatches against r / d in 2e8 random pairs after ONE correction.
// Exactness needs 1/d, r/d and the remainder normal: the host keeps the dictionary only for
// diagonals 2^-100 <= |d| <= 2^100, and a right-hand side r must be zero or inside [2^-900, 2^901)
// (biased exponent in [123, 1923]; tools/markstein_check.c covers both ends of the range and the
// zero/subnormal/infinite edges). The range test is NOT on the dependency chain: each lane ORs it into
// a flag (integer work on r's exponent beside the correction chain), the launch reports it at its end,
// and a conditional pass re-solves the factor with the IEEE division when any step was out of range
// (never, for a stencil solve) — the result is then that pass's, bit for bit the IEEE one. (A
// per-step branch around the IEEE division, round 4's first guard, put 22 instructions and two
// branches on every step: +13% per sweep.)
// The test: frexp's exponent (r = f 2^ex, 0.5 <= |f| < 1; 0 for zero, inf and NaN) in [-899, 901],
// and r not inf / NaN (a class test) — two VALU compares beside the chain, OR-ed into a scalar mask.
__device__ __forceinline__ double div_markstein(double r, double d, double rd, uint64_t &out_of_range) {
    const double q0 = r * rd;
    const double q1 = fma(fma(-q0, d, r), rd, q0);
    const double q2 = fma(fma(-q1, d, r), rd, q1);
    const int ex = __builtin_amdgcn_frexp_exp(r);
    out_of_range |= __builtin_amdgcn_ballot_w64((uint32_t)(ex + 899) > 1800u);
    out_of_range |= __builtin_amdgcn_ballot_w64(__builtin_amdgcn_class(r, 0x207));   // s/qNaN, -inf, +inf
    return r == 0.0 ? q0 : q2;
}
// MK (DICT only): Markstein quotient, range flag OR-ed into *rflag at the end (see div_markstein); !MK:
// IEEE division. gate != nullptr: the conditional re-solve, a no-op unless *gate is set.
template <int K, int D, bool DICT, bool MK>
__global__ __launch_bounds__(2 * kGridLanes) void sptrsv_grid_kernel(
    int64_t n, int64_t w, int64_t H, int64_t sigma2, int64_t phase, int64_t off, int64_t S_full, int upper, int pe,
    int maxyd,
    int unit, const double *__restrict__ rhs, double *x, int32_t *err, const double *__restrict__ grec,
    GridExt ext, const uint32_t *__restrict__ gidx, const double *__restrict__ gdict, int ndict, int32_t *rflag,
    const int32_t *gate, uint32_t *sched) {
    if (gate && __hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;   // uniform
    extern __shared__ __align__(16) unsigned char smem[];
    // the bands this workgroup solves: drawn one after the other from the ticket counter (band b waits only on
    // band b - 1, drawn earlier by a running workgroup; sched_next_block) until they run out. A workgroup
    // that finishes its band takes the next one itself: the launch never needs a workgroup that has not
    // started (round 5: with one band per workgroup, a launch beside a kernel holding most CUs stalled —
    // the dispatcher did not start its later workgroups on the CUs its finished ones freed, tests/
    // test_gpu_progress.py, profiles/r5_progress_probe.txt)
    __shared__ int64_t s_band;
    double *ring = reinterpret_cast<double *>(smem);                  // [2 * kGridRing][kGridRW]
    int64_t *ctl = reinterpret_cast<int64_t *>(smem + 2 * kGridMirror);
    unsigned char *dict = smem + 2 * kGridMirror + 16;                // DICT: ndict GridDict<K> records
    // gdict (host layout): [ndict][K] values, [ndict] diagonals, [ndict][K/2] code words
    if (DICT) {
        const uint32_t *gcode = reinterpret_cast<const uint32_t *>(gdict + (size_t)ndict * (K + 1));
        for (int i = threadIdx.x; i < ndict; i += 2 * kGridLanes) {
            unsigned char *rec = dict + (size_t)i * GridDict<K>::kBytes;
            double *cf = reinterpret_cast<double *>(rec);
            for (int k = 0; k < K; ++k) cf[k] = gdict[(size_t)i * K + k];
            const double dg = gdict[(size_t)ndict * K + i];
            reinterpret_cast<double *>(rec + GridDict<K>::kDg)[0] = dg;
            reinterpret_cast<double *>(rec + GridDict<K>::kDg)[1] = 1.0 / dg;
            uint32_t *ro = reinterpret_cast<uint32_t *>(rec + GridDict<K>::kOff);
            for (int k = 0; k < K; ++k) ro[k] = grid_ring_off((gcode[(size_t)i * (K / 2) + k / 2] >> (16 * (k & 1))) & 0xffff);
        }
    }
    const int64_t nbands = (H + kGridLanes - 1) / kGridLanes;
    auto run_band = [&](const int64_t band) {
        // ctl[0]: last u of the band above present in the ring (poller -> solver)
        // ctl[1]: last u the solver has finished (solver -> poller, ring capacity)
        const int tid = threadIdx.x, j = tid & 63;
        const int64_t y0 = band * kGridLanes;
        const int64_t ylast = (y0 + kGridLanes - 1 < H - 1) ? y0 + kGridLanes - 1 : H - 1;
        const int64_t u_lo = grid_g(sigma2, phase, y0), u_hi = (w - 1) + grid_g(sigma2, phase, ylast);
        const int S = (int)(u_hi - u_lo + 1);
        int min_ud = 1 << 30, max_ud = 0;
        for (int e = 0; e < pe; ++e) {
            const int ud = ext.delta[e] >> 6;
            min_ud = ud < min_ud ? ud : min_ud;
            max_ud = ud > max_ud ? ud : max_ud;
        }
        const bool has_ext = band > 0 && pe > 0;
        for (int i = tid; i < 2 * kGridRing * kGridRW; i += 2 * kGridLanes) ring[i] = 0.0;
        if (tid == 0) {
            ctl[0] = has_ext ? u_lo - max_ud - 1 : INT64_MAX / 2;
            ctl[1] = u_lo - 1;
        }
        __syncthreads();
    #ifdef PSK_GRID_PROF
        const unsigned long long t_start = __builtin_amdgcn_s_memtime();
        const unsigned long long rt_start = __builtin_amdgcn_s_memrealtime();
        unsigned long long n_wait = 0, c_wait = 0;
    #endif
        if (tid >= kGridLanes) {
            // ---------------- poller: u positions [u_lo - max_ud, u_hi - min_ud] of lines y0-maxyd .. y0-1
            if (!has_ext) return;
            const int64_t ua = u_lo - max_ud, ub = u_hi - min_ud;
            for (int64_t base = ua; base <= ub; base += kGridLanes) {
                const int64_t u = base + j;
                double *row_lo = ring + (size_t)((u - u_lo) & (kGridRing - 1)) * kGridRW + (8 - maxyd);
                double *row_hi = row_lo + kGridRing * kGridRW;
                // ring capacity: row (u - u_lo) last held u - kGridRing, which the solver reads until it passes
                // that position + max_ud
                int64_t spins = 0;
                while (__hip_atomic_load(&ctl[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <
                       base + kGridLanes - 1 - kGridRing + max_ud) {
                    if (++spins > kMaxSpins) { atomicExch(err, (2 << 24) | (int)band); return; }
                    __builtin_amdgcn_s_sleep(2);
                }
                uint32_t pending = 0;   // lines of this lane's u still to fetch
                for (int L = 0; L < maxyd; ++L) {
                    const int64_t yl = y0 - maxyd + L, xl = u - grid_g(sigma2, phase, yl), q = yl * w + xl - off;
                    const bool valid = u <= ub && yl >= 0 && xl >= 0 && xl < w && q >= 0 && q < n;
                    if (valid) {
                        pending |= 1u << L;
                    } else {
                        row_lo[L] = 0.0;
                        row_hi[L] = 0.0;
                    }
                }
                spins = 0;
                while (true) {
                    for (int L = 0; L < maxyd; ++L)
                        if (pending & (1u << L)) {
                            const int64_t yl = y0 - maxyd + L, q = yl * w + (u - grid_g(sigma2, phase, yl)) - off;
                            const double v = load_pub(x + (upper ? n - 1 - q : q));
                            if (!is_sentinel(v)) {
                                row_lo[L] = v;
                                row_hi[L] = v;
                                pending &= ~(1u << L);
                            }
                        }
                    // ready prefix of this chunk: lanes 0..r-1 have every line
                    const uint64_t notready = __ballot(pending != 0);
                    const int r = notready ? __builtin_ctzll(notready) : kGridLanes;
                    __builtin_amdgcn_s_waitcnt(0xc07f);   // ring writes before the announcement
                    if (j == 0 && r > 0)
                        __hip_atomic_store(&ctl[0], base + r - 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (!notready) break;
                    if (++spins > kMaxSpins) { atomicExch(err, (3 << 24) | (int)band); return; }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            return;
        }
        // ---------------- solver
        const int64_t y = y0 + j;
        // lane j's line holds grid positions [y*w, y*w + w) of [off, n + off) (the first `off` positions of
        // the first line are empty: a partial line leading the solve order); it is active for steps
        // [s_beg, s_end): x = s - gy in [x_lo, x_hi), gy = g(y) - g(y0) (the line's first step in the band)
        const int64_t x_lo = y * w < off ? off - y * w : 0;
        const int64_t x_hi = n + off - y * w < w ? n + off - y * w : w;
        const bool live = y < H && x_hi > x_lo;
        const int64_t gy = grid_g(sigma2, phase, y) - u_lo;
        const int s_beg = (int)(gy + (live ? x_lo : 0)), s_end = live ? (int)(gy + x_hi) : s_beg;
        const uint32_t s_len = (uint32_t)(s_end - s_beg);
        // byte offset of step s's row: rb8 + rs8 * s (32-bit: n <= kGridMaxRows; step indices < 2^23, so a
        // 24-bit multiply), q = y*w + s - gy - off; a line-less lane reads out of range (loads 0)
        const int64_t qb = y * w - gy - off;
        const uint32_t rb8 = live ? (uint32_t)((upper ? n - 1 - qb : qb) * 8) : kBufOOB - 8;
        const int32_t rs8 = live ? (upper ? -8 : 8) : 0;
        const bool pub = j >= kGridLanes - maxyd;   // the lines the band below reads: agent-scope stores
        const uint32_t lane8 = (uint32_t)(8 + j) * 8;
        const unsigned char *pstep = reinterpret_cast<const unsigned char *>(grec) +
                                     band * S_full * GridStep<K>::kBytes;
        // the index stream of this band: a buffer with the step in the scalar offset
        const __amdgpu_buffer_rsrc_t ridx = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint32_t *>(DICT ? gidx + band * S_full * kGridLanes : gidx), (short)0,
            DICT ? (int)(uint32_t)(S_full * kGridLanes * 4) : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rrhs = grid_rsrc(rhs, n), rx = grid_rsrc(x, n);
        // steps up to s_ok need nothing more from the band above (uniform)
        int s_ok = has_ext ? -max_ud - 1 + min_ud : INT32_MAX / 2;
        uint64_t rbad = 0;   // MK: lanes with a step's right-hand side outside the Markstein range (div_markstein)
        struct Slot {
            uint32_t idx;   // DICT: the record index
            uint32_t code[K / 2];
            double cf[K], d, b;
        };
        auto fetch = [&](int s, Slot &sl) {
            const int sc = s < S ? s : S - 1;   // past the end: re-read the last step (unused)
            const int sa = __builtin_elementwise_max(__builtin_elementwise_min(s, s_end - 1), s_beg);
            sl.b = grid_bload(rrhs, rb8 + (uint32_t)__mul24(rs8, sa));
            if (DICT) {
                sl.idx = __builtin_amdgcn_raw_buffer_load_b32(ridx, (uint32_t)j * 4, (uint32_t)sc * (kGridLanes * 4), 0);
                return;
            }
            const unsigned char *st = pstep + (int64_t)sc * GridStep<K>::kBytes;
            const uint32_t *pc = reinterpret_cast<const uint32_t *>(st + GridStep<K>::kCode) + j * (K / 2);
    #pragma unroll
            for (int k = 0; k < K / 2; ++k) sl.code[k] = pc[k];
            const dv2 *pf = reinterpret_cast<const dv2 *>(st + GridStep<K>::kCoef) + j * (K / 2);
    #pragma unroll
            for (int k = 0; k < K; k += 2) {
                const dv2 c = pf[k / 2];
                sl.cf[k] = c.x;
                sl.cf[k + 1] = c.y;
            }
            sl.d = reinterpret_cast<const double *>(st + GridStep<K>::kDiag)[j];
        };
        auto lookup = [&](uint32_t idx, GridRec<K> &rc) {   // DICT: the record of a step, from LDS
            const unsigned char *rec = dict + idx * GridDict<K>::kBytes;
    #pragma unroll
            for (int k = 0; k < K; k += 2) {
                const dv2 c = *reinterpret_cast<const dv2 *>(rec + 8 * k);
                rc.cf[k] = c.x;
                rc.cf[k + 1] = c.y;
            }
            const dv2 dd = *reinterpret_cast<const dv2 *>(rec + GridDict<K>::kDg);
            rc.d = dd.x;
            rc.rd = dd.y;
    #pragma unroll
            for (int k = 0; k < K; ++k) rc.off[k] = reinterpret_cast<const uint32_t *>(rec + GridDict<K>::kOff)[k];
        };
        // the ring values of step t are requested right after step t-1's ring write (one wave: the LDS
        // queue is in order, so they see it), and the step's other work — the x stores, the prefetch D
        // steps ahead, the dictionary lookup two steps ahead — runs while they are in flight: the chain
        // per step is the LDS round trip and the arithmetic, not the step's whole instruction stream
        auto wait_ext = [&](int t) {
            if (t > s_ok && t < S) {   // uniform: the band above not yet in the ring
    #ifdef PSK_GRID_PROF
                const unsigned long long tw = __builtin_amdgcn_s_memtime();
    #endif
                int64_t spins = 0;
                do {
                    const int known = __builtin_amdgcn_readfirstlane(
                        (int)(__hip_atomic_load(&ctl[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - u_lo));
                    s_ok = known + min_ud;   // ext_known >= u - min_ud  <=>  t <= known + min_ud
                    if (t <= s_ok) break;
                    if (++spins > kMaxSpins) { atomicExch(err, (1 << 24) | (int)band); break; }
                    __builtin_amdgcn_s_sleep(1);
                } while (true);
    #ifdef PSK_GRID_PROF
                n_wait += 1;
                c_wait += __builtin_amdgcn_s_memtime() - tw;
    #endif
            }
        };
        auto request = [&](int t, const Slot &sl, const GridRec<K> &rec, double *v) {
            const uint32_t base = lane8 + (uint32_t)(t & (kGridRing - 1)) * (kGridRW * 8);   // lower copy, row t
    #pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t ro = DICT ? rec.off[k] : grid_ring_off((sl.code[k >> 1] >> (16 * (k & 1))) & 0xffff);
                v[k] = *reinterpret_cast<const double *>(smem + base + ro);
            }
        };
        auto solve = [&](int s, const Slot &sl, const GridRec<K> &rec, const double *v) -> double {
            double acc = 0.0;
    #pragma unroll
            for (int k = 0; k < K; ++k) acc = fma(DICT ? rec.cf[k] : sl.cf[k], v[k], acc);   // stored order; padding adds +-0
            double r = sl.b - acc;
            const double d = DICT ? rec.d : sl.d;
            if (DICT && MK) {   // a select, not a branch, on `unit` (the chain stays branch-free)
                const double q = div_markstein(r, d, rec.rd, rbad);
                r = unit ? r : q;
            } else if (!unit) {
                r = r / d;
            }
            // both copies of the row (the mirror is kGridMirror bytes above)
            const uint32_t base = lane8 + (uint32_t)(s & (kGridRing - 1)) * (kGridRW * 8);
            *reinterpret_cast<double *>(smem + base) = r;
            *reinterpret_cast<double *>(smem + base + kGridMirror) = r;
            return r;
        };
        auto store_x = [&](int s, double r) {   // the lines the band below reads are published
            const bool act = (uint32_t)(s - s_beg) < s_len;
            const uint32_t o = rb8 + (uint32_t)__mul24(rs8, s);
            grid_bstore<0x10>(rx, act && pub ? o : kBufOOB, r);
            grid_bstore<0>(rx, act && !pub ? o : kBufOOB, r);
        };
        static_assert(D >= 3 && D % 2 == 0, "the lookup runs two steps ahead; step parity = slot parity");
        Slot buf[D];
    #pragma unroll
        for (int i = 0; i < D; ++i) fetch(i, buf[i]);
        GridRec<K> rq[2] = {};   // DICT: rq[t & 1] = the record of step t
        if (DICT) {
            lookup(buf[0].idx, rq[0]);
            lookup(buf[1].idx, rq[1]);
        }
        double vn[K];
        wait_ext(0);
        request(0, buf[0], rq[0], vn);
        for (int s0 = 0; s0 < S; s0 += D) {   // D even: step s0 + i has the parity of i
    #pragma unroll
            for (int i = 0; i < D; ++i) {
                const int s = s0 + i;
                const double r = solve(s, buf[i], rq[i & 1], vn);
                __asm__ volatile("" ::: "memory");   // the ring write before the next step's reads
                wait_ext(s + 1);
                request(s + 1, buf[(i + 1) % D], rq[(i + 1) & 1], vn);
                store_x(s, r);
                __asm__ volatile("" ::: "memory");
                fetch(s + D, buf[i]);
                if (DICT) lookup(buf[(i + 2) % D].idx, rq[i & 1]);   // step s + 2's record
                // issued HERE: left to itself the machine scheduler sank the lookup into the next step,
                // next to the ring reads that need it (two LDS round trips on the chain)
                __builtin_amdgcn_sched_barrier(0);
            }
            if (j == 0)   // progress for the poller's ring capacity
                __hip_atomic_store(&ctl[1], u_lo + s0 + D - 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (j == 0) __hip_atomic_store(&ctl[1], INT64_MAX / 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (MK && !unit && rbad != 0 && j == 0) atomicOr(rflag, 1);
    #ifdef PSK_GRID_PROF
        if (j == 0 && band < 8192) {
            g_grid_prof[band * 8 + 0] = t_start;
            g_grid_prof[band * 8 + 1] = __builtin_amdgcn_s_memtime();
            g_grid_prof[band * 8 + 2] = n_wait;
            g_grid_prof[band * 8 + 3] = c_wait;
            g_grid_prof[band * 8 + 4] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;   // XCD
            g_grid_prof[band * 8 + 5] = blockIdx.x;
            g_grid_prof[band * 8 + 6] = rt_start;                                       // 100 MHz, device-wide
            g_grid_prof[band * 8 + 7] = __builtin_amdgcn_s_memrealtime();
        }
    #endif
    };
    for (;;) {
        __syncthreads();   // the previous band's waves are done with the ring (and the dictionary is in LDS)
        if (threadIdx.x == 0) s_band = sched_next_block(sched, nbands);
        __syncthreads();
        const int64_t band = s_band;
        if (band >= nbands) break;
        run_band(band);
    }
}

// x = sentinel on the rows the grid schedule publishes — lines y with y mod 64 >= 64 - maxyd, the ones
// the band below polls (every other row is read only after the launch): maxyd/64 of the vector instead
// of all of it. gate != nullptr: only when *gate is set (before the conditional re-solve).
__global__ void grid_fill_published_kernel(int64_t n, int64_t w, int64_t H, int64_t off, int maxyd, int upper,
                                           double *x, const int32_t *gate) {
    if (gate && __hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const int64_t total = ((H + kGridLanes - 1) / kGridLanes) * maxyd * w;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t li = t / w, xx = t - li * w;
        const int64_t y = (li / maxyd) * kGridLanes + (kGridLanes - maxyd) + li % maxyd, q = y * w + xx - off;
        if (y < H && q >= 0 && q < n) reinterpret_cast<uint64_t *>(x)[upper ? n - 1 - q : q] = kSentinel;
    }
}
__global__ void grid_flag_reset_kernel(int32_t *flag) { *flag = 0; }

static size_t grid_lds_bytes(int K, int ndict) {   // mirrored ring, ctl, dictionary records
    const size_t rec = K == 8 ? GridDict<8>::kBytes : K == 4 ? GridDict<4>::kBytes : GridDict<2>::kBytes;
    return 2 * (size_t)kGridMirror + 2 * sizeof(int64_t) + (ndict > 0 ? (size_t)ndict * rec : 0);
}

static unsigned grid_fill_blocks(const TriFactor &T) {
    const int64_t total = ((T.grid.H + kGridLanes - 1) / kGridLanes) * T.grid.maxyd * T.grid.w;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + kBlock - 1) / kBlock, 4096));
}

int launch_grid_fill(const TriFactor &T, int64_t n, double *x, const int32_t *gate, hipStream_t s) {
    if (T.grid.pe == 0 || T.grid.maxyd == 0) return PSK_OK;   // no band waits on another
    hipLaunchKernelGGL(grid_fill_published_kernel, dim3(grid_fill_blocks(T)), dim3(kBlock), 0, s, n, T.grid.w, T.grid.H,
                       T.grid.off, T.grid.maxyd, T.upper ? 1 : 0, x, gate);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

int launch_grid(const Context *c, int64_t n, const TriFactor &T, const double *rhs, const int32_t *rhs_idx,
                double *x, int32_t *err, hipStream_t s) {
    if (rhs_idx) return fail(PSK_ERR_ARG, "grid schedule: gathered right-hand side (internal)");
    const void *k = nullptr, *kf = nullptr;
#ifndef PSK_GRID_D
#define PSK_GRID_D 12
#endif
#ifndef PSK_GRID_DD   // prefetch depth with the record dictionary (a step's slot: index + rhs)
#define PSK_GRID_DD PSK_GRID_D
#endif
    const bool dict = T.grid.dict_n > 0;
#define PSK_GRID_K(KK, DN)                                                                                    \
    do {                                                                                                      \
        k = dict ? reinterpret_cast<const void *>(&sptrsv_grid_kernel<KK, PSK_GRID_DD, true, true>)           \
                 : reinterpret_cast<const void *>(&sptrsv_grid_kernel<KK, DN, false, false>);                 \
        kf = reinterpret_cast<const void *>(&sptrsv_grid_kernel<KK, PSK_GRID_DD, true, false>);               \
    } while (0)
    if (T.grid.K == 2) PSK_GRID_K(2, PSK_GRID_D);
    else if (T.grid.K == 4) PSK_GRID_K(4, (PSK_GRID_D > 8 ? 8 : PSK_GRID_D));
    else if (T.grid.K == 8) PSK_GRID_K(8, (PSK_GRID_D > 6 ? 6 : PSK_GRID_D));
#undef PSK_GRID_K
    if (!k) return fail(PSK_ERR_ARG, "grid schedule: bad record width");
    int64_t w = T.grid.w, H = T.grid.H, sg = T.grid.sigma, gph = T.grid.phase, goff = T.grid.off, sfull = T.grid.S;
    int upper = T.upper ? 1 : 0, pe_ = T.grid.pe, myd = T.grid.maxyd;
    int unit = T.diag ? 0 : 1;
    const double *gr = T.grid.coef;
    GridExt ext = T.grid.ext;
    const uint32_t *gi = T.grid.idx;
    const double *gdd = T.grid.dict;
    int nd = T.grid.dict_n;
    int32_t *flag = dict ? T.grid.flag : nullptr;
    const int32_t *nogate = nullptr;
    uint32_t *sch = T.sched;
    void *args[] = {&n, &w, &H, &sg, &gph, &goff, &sfull, &upper, &pe_, &myd, &unit, &rhs, &x, &err, &gr, &ext, &gi,
                    &gdd, &nd, &flag, &nogate, &sch};
    // one workgroup per band, at most one per CU (a workgroup holds ~147 KiB of LDS); workgroups draw bands
    // until they run out, so fewer workgroups than bands still solve every band
    const unsigned nb = (unsigned)std::min<int64_t>((H + kGridLanes - 1) / kGridLanes, c->num_cus);
    const size_t lds = grid_lds_bytes(T.grid.K, T.grid.dict_n);
    PSK_HIP(hipLaunchKernel(k, dim3(nb), dim3(2 * kGridLanes), args, lds, s));
    if (dict) {   // conditional IEEE re-solve (div_markstein): no-ops unless a step was out of range
        const int32_t *gate = T.grid.flag;
        int32_t *noflag = nullptr;
        PSK_TRY(launch_grid_fill(T, n, x, gate, s));
        void *fargs[] = {&n, &w, &H, &sg, &gph, &goff, &sfull, &upper, &pe_, &myd, &unit, &rhs, &x, &err, &gr, &ext,
                         &gi, &gdd, &nd, &noflag, &gate, &sch};
        // one workgroup: a no-op unless the gate is set (then it solves every band itself, a rare path), and
        // a launch that needs no more than one free CU to complete
        PSK_HIP(hipLaunchKernel(kf, dim3(1), dim3(2 * kGridLanes), fargs, lds, s));
        hipLaunchKernelGGL(grid_flag_reset_kernel, dim3(1), dim3(1), 0, s, T.grid.flag);
        PSK_HIP(hipGetLastError());
    }
    return PSK_OK;
}

}  // namespace psk
