// trisolve_levels.hip — the levels schedule.
//
// For factors with few rows per dependency level (the SA level-1 operator of -FD 8192^2: 131k rows, 1706
// levels of <= 109 rows): step s solves lane t's row of one level (a level wider than the workgroup takes
// several steps), reading its dependencies from LDS, then a barrier. A hop between levels is an LDS round
// trip plus a barrier instead of a device-scope publication seen by a polling load (sync-free, ~1 us per
// level). Each value lives in an LDS slot the host assigned it (interval allocation: a slot is reused only
// in a step after its last reader), so dependencies any number of levels back are fine as long as the
// values alive at once fit the LDS. Records are field-major per step, loaded D steps ahead into registers;
// the barrier waits for LDS only (lgkmcnt), so those loads stay in flight across it. Per-row arithmetic:
// fma over the stored entries in stored order from 0.0, padding entries (-0.0 x 0.0) add exactly nothing,
// then (b - acc) / d: the band and grid kernels' bits.
#include "trisolve.hpp"

namespace psk {

template <int KM, int D>
__global__ __launch_bounds__(256) void sptrsv_levels_kernel(int64_t nsteps, int R, int64_t n, int unit,
                                                            const uint64_t *__restrict__ rc,
                                                            const uint64_t *__restrict__ sl,
                                                            const double *__restrict__ cf,
                                                            const double *__restrict__ dg,
                                                            const double *__restrict__ bp, double *__restrict__ x) {
    static_assert(KM % 4 == 0, "slots are loaded four per 8-byte word, coefficients two per 16-byte load");
    extern __shared__ double lv_ring[];   // R + 2 slots: R live values, R = 0.0 (padding), R + 1 = trash
    const int t = threadIdx.x, W = blockDim.x;
    for (int i = t; i <= R + 1; i += W) lv_ring[i] = 0.0;
    __syncthreads();
    struct Rec {
        uint64_t rc;
        uint64_t sw[KM / 4];
        double c[KM];
        double d, b;
    };
    (void)R;
    // every load is unconditional, branch-free and independent of the others (an address computed from a
    // loaded count would make the wave wait for that load at once; a predicated load becomes a branch,
    // after which the compiler waits for ALL outstanding loads): entries past a row's count are stored
    // padding (slot R, coefficient -0.0), the diagonal is stored as 1.0 for a unit factor
    const __amdgpu_buffer_rsrc_t rrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t *>(rc), (short)0,
                                                                         (int)(uint32_t)(nsteps * W * 8), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsl = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t *>(sl), (short)0,
                                                                         (int)(uint32_t)(nsteps * W * (KM / 4) * 8),
                                                                         0x00020000);
    const __amdgpu_buffer_rsrc_t rcf = grid_rsrc(cf, nsteps * W * KM), rdg = grid_rsrc(dg, nsteps * W),
                                 rbp = grid_rsrc(bp, nsteps * W), rx = grid_rsrc(x, n);
    auto fetch = [&](int64_t s, Rec &r) {
        const uint32_t sc = (uint32_t)(s < nsteps ? s : nsteps - 1);   // past the end: the last step (unused)
        const uint32_t p = sc * (uint32_t)W + (uint32_t)t;
        r.rc = __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(rrc, p * 8, 0, 0));
        r.d = grid_bload(rdg, p * 8);
        r.b = grid_bload(rbp, p * 8);
#pragma unroll
        for (int k4 = 0; k4 < KM / 4; ++k4)
            r.sw[k4] = __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(
                                                        rsl, ((sc * (KM / 4) + k4) * (uint32_t)W + (uint32_t)t) * 8, 0, 0));
#pragma unroll
        for (int k2 = 0; k2 < KM / 2; ++k2) {
            const auto v4 = __builtin_amdgcn_raw_buffer_load_b128(rcf, ((sc * (KM / 2) + k2) * (uint32_t)W + (uint32_t)t) * 16,
                                                                  0, 0);
            r.c[2 * k2] = __longlong_as_double((long long)((uint64_t)v4[0] | ((uint64_t)v4[1] << 32)));
            r.c[2 * k2 + 1] = __longlong_as_double((long long)((uint64_t)v4[2] | ((uint64_t)v4[3] << 32)));
        }
    };
    // The loop starts D steps early with zeroed records (idle: nothing stored), so that every record load
    // is issued inside the loop: loads issued before it (a prologue) would be merged into the loop
    // header's wait state and make the compiler wait for ALL loads at every iteration.
    Rec buf[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        buf[i].rc = (uint64_t)kLevelIdle | ((uint64_t)(R + 1) << 40);
#pragma unroll
        for (int k4 = 0; k4 < KM / 4; ++k4) buf[i].sw[k4] = 0;
#pragma unroll
        for (int k = 0; k < KM; ++k) buf[i].c[k] = 0.0;
        buf[i].d = 1.0;
        buf[i].b = 0.0;
    }
    for (int64_t s0 = -D; s0 < nsteps; s0 += D) {   // nsteps: a multiple of D (the host pads idle steps)
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int64_t s = s0 + i;
            double acc = 0.0;
            // every entry slot, padding included (-0.0 x 0.0 adds nothing): cutting the chain at the step's
            // widest row with a uniform branch per entry measured slower (0.93 vs 0.62 ms on AMG level 1:
            // the LDS reads no longer all go out before the first fma)
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                const uint32_t slot = (uint32_t)(buf[i].sw[k >> 2] >> (16 * (k & 3))) & 0xFFFFu;
                acc = fma(buf[i].c[k], lv_ring[slot], acc);
            }
            double r = buf[i].b - acc;
            if (!unit) r = r / buf[i].d;   // (uniform)
            lv_ring[(uint32_t)(buf[i].rc >> 40) & 0xFFFFu] = r;
            const uint32_t row = (uint32_t)buf[i].rc;
            grid_bstore<0>(rx, row != kLevelIdle ? row * 8u : kBufOOB, r);   // idle lanes: out of range, dropped
            fetch(s + D, buf[i]);
            // the step's ring writes before the next step's reads (LDS-only fences: the prefetch loads stay
            // in flight across the barrier)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        }
    }
}

// right-hand side into step order: bp[p] = rhs[idx ? idx[row] : row] (0 on idle lanes)
__global__ void levels_gather_kernel(int64_t np, const uint64_t *__restrict__ rc, const double *__restrict__ rhs,
                                     const int32_t *__restrict__ idx, double *__restrict__ bp) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const uint32_t row = (uint32_t)rc[p];
    bp[p] = row == kLevelIdle ? 0.0 : rhs[idx ? idx[row] : row];
}

int launch_levels(const Context *c, int64_t n, const TriFactor &T, const double *rhs, const int32_t *rhs_idx,
                  double *x, int32_t *err, hipStream_t s) {
    int64_t ns = T.lv.steps;
    const int64_t np = ns * T.lv.W;
    hipLaunchKernelGGL(levels_gather_kernel, dim3((unsigned)((np + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, np,
                       T.lv.rc, rhs, rhs_idx, T.lv.b);
    PSK_HIP(hipGetLastError());
    const void *k = T.lv.KM == 4    ? reinterpret_cast<const void *>(&sptrsv_levels_kernel<4, kLevelD>)
                    : T.lv.KM == 8  ? reinterpret_cast<const void *>(&sptrsv_levels_kernel<8, kLevelD>)
                    : T.lv.KM == 12 ? reinterpret_cast<const void *>(&sptrsv_levels_kernel<12, kLevelD>)
                                    : reinterpret_cast<const void *>(&sptrsv_levels_kernel<16, kLevelD>);
    int R = T.lv.R, unit = T.diag ? 0 : 1;
    const uint64_t *lrc = T.lv.rc;
    const uint64_t *lsl = T.lv.sl;
    const double *lcf = T.lv.cf, *ldg = T.lv.dg, *lb = T.lv.b;
    void *args[] = {&ns, &R, &n, &unit, &lrc, &lsl, &lcf, &ldg, &lb, &x};
    PSK_HIP(hipLaunchKernel(k, dim3(1), dim3(T.lv.W), args, (size_t)(R + 2) * sizeof(double), s));
    return PSK_OK;
}

}  // namespace psk
