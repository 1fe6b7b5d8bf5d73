// iluk.hip — level-of-fill ILU(k): the fill pattern built on the device (psk_csr_iluk_pattern) and the preconditioner
// on it (psk_prec_create_iluk = the pattern, then ilu0.hip's numeric phase and hand-off unchanged). Replaces nothing
// in the reference, whose incomplete factorisations are SuperLU's (ILUTPreconditioner.py:51-53).
//
// The definition is sequential (include/psk.h): rows in ascending order, each row's lower entries in ascending
// column, lev(i,j) = min(lev(i,j), lev(i,c) + lev(c,j) + 1) kept while <= k. The device algorithm is not: an entry of
// final level t >= 1 has a pair (i,c), (c,j), c < min(i,j), whose final levels are both < t and sum to t - 1, and no
// pair that sums to less. So ROUND t = 1 .. k reads the pattern of all entries of level < t (final by induction) and
// adds, for every row independently, the columns j that are absent from the row and have a pair with
// lev(i,c) + lev(c,j) = t - 1; all of them get level t. All k rounds run: a round that adds nothing skips its scan
// finish, allocation and fill pass, but a later round may still add entries (levels 1 + 1 make a level 3 on a pattern
// that has no level 2), so an empty round does not end the phase.
//
// Kernels (gfx950, wave64; no floating-point atomics — the only atomics are int32 compare-and-swap on LDS and
// integer min / or on three device words; no workgroup or wave waits on another; every loop bounded by a row
// length or the table size):
//  * iluk_sort_kernel: one wave per row ranks the row's entries by column into the working copy S (as ilu0.hip's
//    sort), records the diagonal's position and flags a duplicate column, a missing diagonal, a column outside
//    [0, n) and a row over the cap (the cap is not enforced at k = 0, where no round runs).
//  * iluk_round_kernel<G, FILL, SECOND>: G lanes (1, 4, 16 or 64, from the mean row length of the current pattern)
//    share a row; 256 / G rows per workgroup. The group walks the row's lower entries c in turn and strides over the
//    upper part of row c; a column with the wanted level that a binary search does not find in row i goes into the
//    row's open-addressing hash set in LDS (16 G slots; the set's content does not depend on the insertion order).
//    Count pass (FILL = false): D = the set's size -> the row's new length. Fill pass: the same set again, compacted
//    into a list, then every old and new entry is placed at (old entries with a smaller column) + (new entries with a
//    smaller column): ascending columns, whatever the order in the set. A set holds up to 8 G new columns per
//    round; a row that needs more is marked and redone by the G = 64 instance (SECOND = true, launched only when a
//    row asked for it), whose 512 = PSK_ILUK_ROW_CAP cover every row under the cap. A row over the cap is frozen
//    (copied from then on) and the smallest such row kept in a device word: rows depend only on rows above them,
//    so every row up to the smallest one over the cap is still exact and that row is the one the definition names.
//    LDS: (16 G + 8 G) int32 per row x 256 / G rows = 24 KiB per workgroup for every G, 6 workgroups per CU of the
//    160 KiB; a cap of 1024 would halve that for rows no test or grid operator here reaches.
//    Bytes per round: each pass streams the pattern (5 B per entry: int32 column, uint8 level) and, per lower entry,
//    the upper part of the row it names (L2); the fill writes 5 B per entry of the new pattern.
//  * iluk_pad_kernel: G lanes per row merge S's row into the filled row: P's values are zero-filled, then every
//    entry of S finds its column by binary search and stores its value. iluk_lev_kernel: levels as doubles.
//
// Data movement: during the symbolic phase the host downloads, per round, ONE int32 (did a row ask for the wide
// instance) and ONE int64 (the new pattern's entry count, for its allocation), and at the end one int32 (the
// smallest row over the cap); before it, the structure flags of the sort. No index or value array leaves the device.
// The pattern download psk_csr_ilu0 makes for the host's level planner stays as it is.
#include "psk_internal.hpp"

#include <chrono>
#include <climits>
#include <cstdlib>

namespace psk {

static IlukTiming g_iluk;
const IlukTiming &iluk_last_timing() { return g_iluk; }

namespace {

constexpr int kCap = PSK_ILUK_ROW_CAP;
constexpr int32_t kFlagDup = 1, kFlagNoDiag = 2, kFlagRange = 4;
constexpr uint8_t kRowNarrow = 0, kRowWide = 1, kRowFrozen = 2;
// the hash set of one row: 16 slots per lane of its group, half of them usable, and the compacted list
constexpr int kSlotsPerLane = 16;
static_assert(64 * kSlotsPerLane / 2 == kCap, "the widest group's set must hold a whole row under the cap");

struct Tmp {
    std::vector<void *> p;
    ~Tmp() {
        for (void *q : p)
            if (q) (void)hipFree(q);
    }
    template <class T> int get(int64_t count, T **out) {
        void *q = nullptr;
        if (hipMalloc(&q, (size_t)(count > 0 ? count : 1) * sizeof(T)) != hipSuccess)
            return fail(PSK_ERR_ALLOC, "iluk: hipMalloc of a temporary failed");
        p.push_back(q);
        *out = static_cast<T *>(q);
        return PSK_OK;
    }
    void drop(void *q) {
        for (void *&r : p)
            if (r == q && q) {
                (void)hipFree(q);
                r = nullptr;
            }
    }
};

constexpr int64_t kGridX = (int64_t)1 << 20;
dim3 grid_for_blocks(int64_t nb) {
    return nb <= kGridX ? dim3((unsigned)(nb > 0 ? nb : 1)) : dim3((unsigned)kGridX, (unsigned)((nb + kGridX - 1) / kGridX));
}
__device__ __forceinline__ int64_t block_index() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__global__ __launch_bounds__(kBlock) void iluk_sort_kernel(int64_t n, const int32_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ col,
                                                           const double *__restrict__ val, int32_t *__restrict__ scol,
                                                           double *__restrict__ sval, int32_t *__restrict__ diag,
                                                           int32_t *words) {
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
        scol[s0 + rank] = c;
        sval[s0 + rank] = val[s0 + q];
        if (c == i) {
            diag[i] = s0 + rank;
            found = true;
        }
    }
    if (!__any(found ? 1 : 0) && lane == 0) bad |= kFlagNoDiag;
    if (bad) atomicOr(words, bad);
    if (L > kCap && lane == 0) atomicMin(words + 1, (int32_t)i);
}

// first position in [lo, hi) whose column is >= j
__device__ __forceinline__ int32_t lower_bound(const int32_t *__restrict__ col, int32_t lo, int32_t hi, int32_t j) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (col[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct Pattern {
    const int32_t *rp, *ci, *dg;
    const uint8_t *lv;
};

// One round (see the file comment). state: per row, which instance owns it; words[1] = smallest row over the cap,
// words[2] = a row asked for the wide instance. Count pass: counts[i] = the row's new length. Fill pass: the new
// pattern (rp2 already scanned from counts).
template <int G, bool FILL, bool SECOND>
__global__ __launch_bounds__(kBlock) void iluk_round_kernel(int64_t n, int32_t round, Pattern P, uint8_t *state,
                                                            int32_t *__restrict__ counts,
                                                            const int32_t *__restrict__ rp2, int32_t *__restrict__ ci2,
                                                            uint8_t *__restrict__ lv2, int32_t *__restrict__ dg2,
                                                            int32_t *words) {
    constexpr int R = kBlock / G, H = kSlotsPerLane * G, LIM = H / 2;
    __shared__ int32_t s_tab[R * H];
    __shared__ int32_t s_list[FILL ? R * LIM : 1];
    const int slot = threadIdx.x / G, t = threadIdx.x % G;
    const int64_t i = block_index() * R + slot;
    int32_t *tab = s_tab + slot * H;
    for (int s = t; s < H; s += G) tab[s] = -1;
    bool active = i < n;
    uint8_t st = kRowNarrow;
    if (active && (FILL || SECOND)) st = state[i];
    if (active) active = SECOND ? st == kRowWide : st != kRowWide;   // a count pass of the first instance: every row
    int32_t r0 = 0, r1 = 0, d = 0;
    if (active) {
        r0 = P.rp[i];
        r1 = P.rp[i + 1];
        d = P.dg[i];
    }
    const bool frozen = FILL && st == kRowFrozen;
    __syncthreads();
    if (active && !frozen) {
        for (int32_t e = r0; e < d; ++e) {   // the row's lower entries; bounds uniform over the group
            const int32_t c = P.ci[e], need = round - 1 - (int32_t)P.lv[e];
            const int32_t u1 = P.rp[c + 1];
            for (int32_t f = P.dg[c] + 1 + t; f < u1; f += G) {
                if ((int32_t)P.lv[f] != need) continue;
                const int32_t j = P.ci[f];
                const int32_t q = lower_bound(P.ci, r0, r1, j);
                if (q < r1 && P.ci[q] == j) continue;   // already in the row, with a level < round
                uint32_t h = ((uint32_t)j * 2654435761u) & (uint32_t)(H - 1);
                for (int probe = 0; probe < H; ++probe) {   // a full set drops the column: D > LIM is seen below
                    const int32_t old = atomicCAS(&tab[h], -1, j);
                    if (old == -1 || old == j) break;
                    h = (h + 1) & (uint32_t)(H - 1);
                }
            }
        }
    }
    __syncthreads();
    // D = the set's size: lane t counts its 16 slots, an inclusive scan over the group
    int32_t mine = 0;
    for (int s = 0; s < kSlotsPerLane; ++s) mine += tab[t * kSlotsPerLane + s] >= 0 ? 1 : 0;
    int32_t inc = mine;
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        const int32_t up = __shfl_up(inc, o, G);
        if (t >= o) inc += up;
    }
    const int32_t D = G > 1 ? __shfl(inc, G - 1, G) : inc;
    if constexpr (!FILL) {
        if (!active || t != 0) return;
        const int32_t len = r1 - r0;
        uint8_t ns = SECOND ? kRowWide : kRowNarrow;
        int32_t nl = len + D;
        if (D > LIM && G < 64) {
            ns = kRowWide;
            nl = len;   // the second instance overwrites it
            if (!(__hip_atomic_load(words + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1)) atomicOr(words + 2, 1);
        } else if (D > LIM || nl > kCap) {
            ns = kRowFrozen;
            nl = len;
            atomicMin(words + 1, (int32_t)i);
        }
        state[i] = ns;
        counts[i] = nl;
    } else {
        int32_t *list = s_list + slot * LIM;
        if (active && !frozen) {
            int32_t w = inc - mine;
            for (int s = 0; s < kSlotsPerLane; ++s) {
                const int32_t j = tab[t * kSlotsPerLane + s];
                if (j >= 0 && w < LIM) list[w++] = j;
            }
        }
        __syncthreads();
        if (!active) return;
        const int32_t o0 = rp2[i], o1 = rp2[i + 1];
        if (frozen) {
            for (int32_t q = r0 + t; q < r1; q += G) {
                const int32_t pos = o0 + (q - r0);
                if (pos < o1) {
                    ci2[pos] = P.ci[q];
                    lv2[pos] = P.lv[q];
                }
            }
            if (t == 0) dg2[i] = o0 + (d - r0);
            return;
        }
        const int32_t nd = D < LIM ? D : LIM;
        for (int32_t q = r0 + t; q < r1; q += G) {   // old entries
            const int32_t c = P.ci[q];
            int32_t below = 0;
            for (int32_t x = 0; x < nd; ++x) below += list[x] < c ? 1 : 0;
            const int32_t pos = o0 + (q - r0) + below;
            if (pos < o1) {
                ci2[pos] = c;
                lv2[pos] = P.lv[q];
                if (c == i) dg2[i] = pos;
            }
        }
        for (int32_t y = t; y < nd; y += G) {   // new entries, all of level `round`
            const int32_t j = list[y];
            int32_t below = 0;
            for (int32_t x = 0; x < nd; ++x) below += list[x] < j ? 1 : 0;
            const int32_t pos = o0 + (lower_bound(P.ci, r0, r1, j) - r0) + below;
            if (pos < o1) {
                ci2[pos] = j;
                lv2[pos] = (uint8_t)round;
            }
        }
    }
}

// S's row merged into the filled row: pval is zero-filled before; G lanes per row
template <int G>
__global__ __launch_bounds__(kBlock) void iluk_pad_kernel(int64_t n, const int32_t *__restrict__ srp,
                                                          const int32_t *__restrict__ scol,
                                                          const double *__restrict__ sval,
                                                          const int32_t *__restrict__ prp,
                                                          const int32_t *__restrict__ pcol, double *__restrict__ pval) {
    const int64_t gid = block_index() * kBlock + threadIdx.x;
    const int64_t i = gid / G;
    const int32_t t = (int32_t)(gid % G);
    if (i >= n) return;
    const int32_t s1 = srp[i + 1], p0 = prp[i], p1 = prp[i + 1];
    for (int32_t q = srp[i] + t; q < s1; q += G) {
        const int32_t j = scol[q];
        const int32_t pos = lower_bound(pcol, p0, p1, j);
        if (pos < p1 && pcol[pos] == j) pval[pos] = sval[q];
    }
}

__global__ __launch_bounds__(kBlock) void iluk_lev_kernel(int64_t nnz, const uint8_t *__restrict__ lv,
                                                          double *__restrict__ out) {
    const int64_t e = block_index() * kBlock + threadIdx.x;
    if (e < nnz) out[e] = (double)lv[e];
}

// lanes per row from the mean row length (PSK_ILUK_WIDTH=1|4|16|64 overrides: tests of the geometry independence)
int group_width(int64_t n, int64_t nnz) {
    if (const char *e = std::getenv("PSK_ILUK_WIDTH")) {
        const int w = std::atoi(e);
        if (w == 1 || w == 4 || w == 16 || w == 64) return w;
    }
    const double mean = n > 0 ? (double)nnz / (double)n : 0.0;
    return mean <= 2.0 ? 1 : mean <= 8.0 ? 4 : mean <= 32.0 ? 16 : 64;
}

template <int G, bool FILL, bool SECOND>
void launch_round(int64_t n, int32_t round, const Pattern &P, uint8_t *state, int32_t *counts, const int32_t *rp2,
                  int32_t *ci2, uint8_t *lv2, int32_t *dg2, int32_t *words, hipStream_t s) {
    constexpr int R = kBlock / G;
    hipLaunchKernelGGL((iluk_round_kernel<G, FILL, SECOND>), grid_for_blocks((n + R - 1) / R), dim3(kBlock), 0, s, n,
                       round, P, state, counts, rp2, ci2, lv2, dg2, words);
}

template <bool FILL>
void launch_first(int G, int64_t n, int32_t round, const Pattern &P, uint8_t *state, int32_t *counts,
                  const int32_t *rp2, int32_t *ci2, uint8_t *lv2, int32_t *dg2, int32_t *words, hipStream_t s) {
    switch (G) {
    case 1: launch_round<1, FILL, false>(n, round, P, state, counts, rp2, ci2, lv2, dg2, words, s); break;
    case 4: launch_round<4, FILL, false>(n, round, P, state, counts, rp2, ci2, lv2, dg2, words, s); break;
    case 16: launch_round<16, FILL, false>(n, round, P, state, counts, rp2, ci2, lv2, dg2, words, s); break;
    default: launch_round<64, FILL, false>(n, round, P, state, counts, rp2, ci2, lv2, dg2, words, s); break;
    }
}

template <int G>
void launch_pad(int64_t n, const int32_t *srp, const int32_t *scol, const double *sval, const psk_csr *P,
                hipStream_t s) {
    hipLaunchKernelGGL(iluk_pad_kernel<G>, grid_for_blocks((n * G + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, srp,
                       scol, sval, (const int32_t *)P->rowptr, (const int32_t *)P->colidx, P->vals);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// *Pout (and *Lout when asked for) are written only on success
int iluk_pattern(const psk_csr *A, int32_t k, psk_csr **Pout, psk_csr **Lout) {
    if (!A || !Pout) return fail(PSK_ERR_ARG, "psk_csr_iluk_pattern: NULL argument");
    if (k < 0 || k > PSK_ILUK_MAX_LEVEL)
        return fail(PSK_ERR_ARG, "psk_csr_iluk_pattern: the level k must lie in [0, " + std::to_string(PSK_ILUK_MAX_LEVEL) + "]");
    if (A->comm) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_iluk_pattern: sharded matrix");
    if (A->n != A->ncols) return fail(PSK_ERR_ARG, "psk_csr_iluk_pattern: A must be square");
    if (A->n == 0 || A->nnz == 0) return fail(PSK_ERR_ARG, "psk_csr_iluk_pattern: A is empty");
    Context *c;
    PSK_TRY(ctx(&c));
    hipStream_t s = c->stream;
    const int64_t n = A->n, nnz0 = A->nnz, nt = exscan_tiles(n);
    const auto t_start = std::chrono::steady_clock::now();
    g_iluk = IlukTiming();
    g_iluk.level = k;
    g_iluk.nnz_a = nnz0;
    Tmp tmp;
    int32_t *scol, *words, *counts, *dg, *rp = nullptr, *ci;
    uint8_t *lv, *state;
    double *sval;
    int64_t *tiles;
    PSK_TRY(tmp.get(nnz0, &scol));
    PSK_TRY(tmp.get(nnz0, &sval));
    PSK_TRY(tmp.get(nnz0, &lv));
    PSK_TRY(tmp.get(n, &dg));
    PSK_TRY(tmp.get(n, &state));
    PSK_TRY(tmp.get(n, &counts));
    PSK_TRY(tmp.get(nt + 1, &tiles));
    PSK_TRY(tmp.get(3, &words));   // [0] structure flags, [1] smallest row over the cap, [2] a row wants the wide instance
    const int32_t init[3] = {0, INT32_MAX, 0};
    PSK_HIP(hipMemcpyAsync(words, init, sizeof(init), hipMemcpyHostToDevice, s));
    PSK_HIP(hipMemsetAsync(lv, 0, (size_t)nnz0, s));
    hipLaunchKernelGGL(iluk_sort_kernel, grid_for_blocks((n + kWaves - 1) / kWaves), dim3(kBlock), 0, s, n,
                       (const int32_t *)A->rowptr, (const int32_t *)A->colidx, (const double *)A->vals, scol, sval, dg,
                       words);
    PSK_HIP(hipGetLastError());
    int32_t flags = 0;
    PSK_HIP(hipMemcpyAsync(&flags, words, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    if (flags & kFlagRange) return fail(PSK_ERR_ARG, "psk_csr_iluk_pattern: column index out of range");
    if (flags & kFlagDup) return fail(PSK_ERR_UNSUPPORTED, "psk_csr_iluk_pattern: duplicate column within a row");
    if (flags & kFlagNoDiag) return fail(PSK_ERR_ARG, "psk_csr_iluk_pattern: a row has no stored diagonal entry");
    // the current pattern: S's at first (A's row pointers, read only), then each round's
    Pattern cur{(const int32_t *)A->rowptr, scol, dg, lv};
    ci = scol;
    int64_t nnz = nnz0;
    for (int32_t t = 1; t <= k; ++t) {
        const int G = group_width(n, nnz);
        g_iluk.width = G;
        const int32_t zero = 0;
        PSK_HIP(hipMemcpyAsync(words + 2, &zero, sizeof(int32_t), hipMemcpyHostToDevice, s));
        launch_first<false>(G, n, t, cur, state, counts, nullptr, nullptr, nullptr, nullptr, words, s);
        PSK_HIP(hipGetLastError());
        int32_t wide = 0;
        if (G < 64) {
            PSK_HIP(hipMemcpyAsync(&wide, words + 2, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            PSK_HIP(hipStreamSynchronize(s));
            if (wide) {
                launch_round<64, false, true>(n, t, cur, state, counts, nullptr, nullptr, nullptr, nullptr, words, s);
                PSK_HIP(hipGetLastError());
                g_iluk.wide_rounds++;
            }
        }
        int64_t total = 0;
        PSK_TRY(exscan_total(n, counts, tiles, nt, s, &total));
        // nothing of level t: no new pattern to build, but later rounds still run — level t + 1 needs two levels
        // that sum to t, which may both lie below t (1 + 1 makes a level 3 where no level 2 exists)
        if (total == nnz) continue;
        if (total > kMaxNnz)
            return fail(PSK_ERR_UNSUPPORTED, "psk_csr_iluk_pattern: the pattern exceeds the int32 nnz limit");
        int32_t *rp2, *ci2, *dg2;
        uint8_t *lv2;
        PSK_TRY(tmp.get(n + 1, &rp2));
        PSK_TRY(tmp.get(total, &ci2));
        PSK_TRY(tmp.get(total, &lv2));
        PSK_TRY(tmp.get(n, &dg2));
        PSK_TRY(exscan_finish(n, counts, tiles, nt, rp2, s));
        launch_first<true>(G, n, t, cur, state, nullptr, rp2, ci2, lv2, dg2, words, s);
        if (wide) launch_round<64, true, true>(n, t, cur, state, nullptr, rp2, ci2, lv2, dg2, words, s);
        PSK_HIP(hipGetLastError());
        PSK_HIP(hipStreamSynchronize(s));
        if (ci != scol) tmp.drop(ci);   // S's columns are kept for the padding
        tmp.drop(rp);
        tmp.drop(lv);
        tmp.drop(dg);
        rp = rp2, ci = ci2, lv = lv2, dg = dg2;
        cur = Pattern{rp, ci, dg, lv};
        nnz = total;
        g_iluk.rounds = t;
    }
    int32_t bad = INT32_MAX;
    PSK_HIP(hipMemcpyAsync(&bad, words + 1, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PSK_HIP(hipStreamSynchronize(s));
    if (bad != INT32_MAX && k > 0)   // k = 0 builds no set in LDS: S of any row length, as psk_csr_ilu0 takes it
        return fail(PSK_ERR_UNSUPPORTED, "psk_csr_iluk_pattern: the filled row " + std::to_string(bad) +
                                             " is longer than PSK_ILUK_ROW_CAP = " + std::to_string(kCap) + " entries");
    psk_csr *P = nullptr, *Lv = nullptr;
    auto work = [&]() -> int {
        PSK_TRY(csr_new_device(n, n, nnz, &P));
        PSK_HIP(hipMemcpyAsync(P->rowptr, cur.rp, (size_t)(n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        PSK_HIP(hipMemcpyAsync(P->colidx, cur.ci, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        PSK_HIP(hipMemsetAsync(P->vals, 0, (size_t)nnz * sizeof(double), s));   // +0.0 at every fill entry
        switch (group_width(n, nnz0)) {
        case 1: launch_pad<1>(n, A->rowptr, scol, sval, P, s); break;
        case 4: launch_pad<4>(n, A->rowptr, scol, sval, P, s); break;
        case 16: launch_pad<16>(n, A->rowptr, scol, sval, P, s); break;
        default: launch_pad<64>(n, A->rowptr, scol, sval, P, s); break;
        }
        PSK_HIP(hipGetLastError());
        if (Lout) {
            PSK_TRY(csr_new_device(n, n, nnz, &Lv));
            PSK_HIP(hipMemcpyAsync(Lv->rowptr, cur.rp, (size_t)(n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
            PSK_HIP(hipMemcpyAsync(Lv->colidx, cur.ci, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(iluk_lev_kernel, grid_for_blocks((nnz + kBlock - 1) / kBlock), dim3(kBlock), 0, s, nnz,
                               (const uint8_t *)cur.lv, Lv->vals);
            PSK_HIP(hipGetLastError());
            PSK_TRY(csr_finish_device(Lv, s));
        }
        return csr_finish_device(P, s);
    };
    const int rc = work();
    if (rc != PSK_OK) {
        (void)hipStreamSynchronize(s);
        if (P) csr_discard(P);
        if (Lv) csr_discard(Lv);
        return rc;
    }
    g_iluk.nnz_p = nnz;
    g_iluk.symbolic_ms = ms_since(t_start);
    *Pout = P;
    if (Lout) *Lout = Lv;
    return PSK_OK;
}

}  // namespace
}  // namespace psk

using namespace psk;

extern "C" {

int psk_csr_iluk_pattern(const psk_csr *A, int32_t k, psk_csr **P, psk_csr **Lev) { return iluk_pattern(A, k, P, Lev); }

int psk_prec_create_iluk(const psk_csr *A, int32_t k, psk_prec **out) {
    if (!out) return fail(PSK_ERR_ARG, "psk_prec_create_iluk: NULL argument");
    psk_csr *P = nullptr;
    PSK_TRY(iluk_pattern(A, k, &P, nullptr));
    const int rc = psk_prec_create_ilu0(P, out);   // numeric phase, split and planner: ilu0.hip, unchanged
    (void)psk_csr_destroy(P);
    return rc;
}

}  // extern "C"
