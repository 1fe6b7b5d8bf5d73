// trisolve_plan.hip — the host planner of the triangular-solve schedules: pure host arithmetic (no HIP call,
// no Context). It simulates every schedule a factor is eligible for with measured per-level / per-row costs,
// keeps the fastest (TriFactor::schedule; psk_prec_trisolve_schedule reports and overrides it) and packs the
// layouts the kernels read (plan_factor; make_factor in trisolve.hip uploads them).
#include "trisolve.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <unordered_map>

namespace psk {

namespace {

constexpr int kGridDictMax = 64;

// Distinct records of the grid schedule's record blob (nsteps blocks of SB bytes: [64][K] codes at 0,
// [64][K] values at oc, [64] diagonals at od). With at most kGridDictMax of them: idx = each
// lane-step's record number in the kernel's access order (block-major, lane-minor), dict = [n][K]
// values, [n] diagonals, [n][K/2] code words packed two uint32 per double; ndict = n. Else ndict = 0.
void build_grid_dict(const unsigned char *gb, int64_t nsteps, int64_t SB, int K, int64_t oc, int64_t od,
                     std::vector<uint32_t> &idx, std::vector<double> &dict, int &ndict) {
    ndict = 0;
    const size_t rb = (size_t)K * 2 + (size_t)K * 8 + 8;   // key bytes: codes, values, diagonal
    std::vector<unsigned char> keys;                       // distinct records, rb bytes each
    std::unordered_map<uint64_t, std::vector<int>> by_hash;
    idx.assign((size_t)(nsteps * kGridLanes), 0);
    unsigned char key[2 * 8 + 8 * 8 + 8];
    for (int64_t t = 0; t < nsteps; ++t) {
        const unsigned char *blk = gb + t * SB;
        for (int l = 0; l < kGridLanes; ++l) {
            std::memcpy(key, blk + (size_t)l * K * 2, (size_t)K * 2);
            std::memcpy(key + K * 2, blk + oc + (size_t)l * K * 8, (size_t)K * 8);
            std::memcpy(key + K * 10, blk + od + (size_t)l * 8, 8);
            uint64_t h = 1469598103934665603ull;   // FNV-1a
            for (size_t i = 0; i < rb; ++i) h = (h ^ key[i]) * 1099511628211ull;
            int found = -1;
            auto &cand = by_hash[h];
            for (int c : cand)
                if (std::memcmp(keys.data() + (size_t)c * rb, key, rb) == 0) { found = c; break; }
            if (found < 0) {
                found = (int)(keys.size() / rb);
                if (found == kGridDictMax) {
                    idx.clear();
                    return;
                }
                keys.insert(keys.end(), key, key + rb);
                cand.push_back(found);
            }
            idx[(size_t)(t * kGridLanes + l)] = (uint32_t)found;
        }
    }
    const int nd = (int)(keys.size() / rb);
    const size_t ncw = (size_t)nd * K / 2;                  // code words
    dict.assign((size_t)nd * (K + 1) + (ncw + 1) / 2, 0.0);
    uint32_t *cw = reinterpret_cast<uint32_t *>(dict.data() + (size_t)nd * (K + 1));
    for (int r = 0; r < nd; ++r) {
        const unsigned char *k = keys.data() + (size_t)r * rb;
        std::memcpy(dict.data() + (size_t)r * K, k + K * 2, (size_t)K * 8);
        std::memcpy(dict.data() + (size_t)nd * K + r, k + K * 10, 8);
        std::memcpy(cw + (size_t)r * (K / 2), k, (size_t)K * 2);   // K uint16 codes = K/2 words, as in a record
    }
    ndict = nd;
}

// Cost model (us), fitted to measurements on MI355X (tools/bench_amg.py, tools/bench_gmres.py):
// sync-free: a row costs one agent-scope load round trip (~0.61) on its wave, plus a hand-off (~0.36)
// after its last dependency was published (FD m=1024 ILU with the DPP row total: 0.96 us per level,
// 12.1 ms for L + U); band: a local level
// costs ~0.9 us with the ring (it is paced by the one external load of the block's boundary row;
// FD 2048^2 Gauss-Seidel: 3.9 ms for ~4100 levels) and ~2.7 us without (AMG level 3 at 8192^2).
constexpr double kHopUs = 0.36, kRowUs = 0.61, kBandLevelRingUs = 1.0, kBandLevelMemUs = 2.7;
constexpr double kLdsLevelUs = 0.15, kLdsBytesPerUs = 40e3;   // LDS schedule (provisional)
// levels schedule: a step's barrier + LDS round trip, one CU's record stream (1708 steps, 31.5 MB: measured 0.615 ms)
constexpr double kLevelStepUs = 0.30, kLevelBytesPerUs = 200e3;   // fitted: AMG level 1 of -FD 8192^2, 0.615 ms
constexpr double kNarrowLevelUs = 0.8;    // narrow band local level (FD 8192^2 Gauss-Seidel: 12.6 ms / 16128 levels)

}  // namespace

// global dependency levels -> counting-sort the rows by level (stable: solve order inside a level); shared with
// the ILU(0) numeric phase (ilu0.hip), whose launches are the levels of strict-lower(A)
void level_order(const HostFactor &F, std::vector<int32_t> &order, std::vector<int32_t> &lev, int64_t &nlev) {
    const int64_t n = F.n;
    lev.assign(n, 0);
    int32_t maxl = -1;
    for (int64_t p = 0; p < n; ++p) {
        const int64_t i = F.row(p);
        int32_t l = 0;
        for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j) l = std::max(l, lev[F.ci[j]] + 1);
        lev[i] = l;
        maxl = std::max(maxl, l);
    }
    nlev = maxl + 1;
    std::vector<int64_t> cnt((size_t)nlev + 1, 0);
    for (int64_t i = 0; i < n; ++i) cnt[lev[i] + 1]++;
    for (int64_t l = 0; l < nlev; ++l) cnt[l + 1] += cnt[l];
    order.assign(n, 0);
    for (int64_t p = 0; p < n; ++p) {
        const int64_t i = F.row(p);
        order[cnt[lev[i]]++] = (int32_t)i;
    }
}

namespace {

// simulated time of the sync-free schedule: wave w processes order[w], order[w+W], ...
double simulate_syncfree(const HostFactor &F, const std::vector<int32_t> &order, int64_t waves) {
    std::vector<double> fin(F.n, 0.0), wave_free((size_t)std::max<int64_t>(waves, 1), 0.0);
    double tmax = 0.0;
    for (int64_t k = 0; k < F.n; ++k) {
        const int64_t i = order[k];
        double t = wave_free[k % waves];
        for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j) t = std::max(t, fin[F.ci[j]] + kHopUs);
        t += kRowUs;
        fin[i] = t;
        wave_free[k % waves] = t;
        tmax = std::max(tmax, t);
    }
    return tmax;
}

struct Band {
    int64_t B = 0, nblocks = 0, G = 0;
    std::vector<int32_t> rows;
    std::vector<int64_t> lvl_ptr, blk_lvl;
    int32_t ring_words = 0;
    double est = 0.0;
};

// band schedule with block size B: local levels, ring check, simulated time with the workgroups that
// fit (per_cu_max per CU, fewer when the LDS ring + chunk buffers of record width K need it)
void build_band(const HostFactor &F, int64_t B, int num_cus, int per_cu_max, int K, Band &bd) {
    const int64_t n = F.n;
    bd.B = B;
    bd.nblocks = (n + B - 1) / B;
    std::vector<int32_t> llev(n, 0);   // local level by row
    int64_t max_dist = 0;
    for (int64_t p = 0; p < n; ++p) {
        const int64_t i = F.row(p), p_lo = (p / B) * B;
        int32_t l = 0;
        for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j) {
            const int64_t pj = F.pos(F.ci[j]);
            if (pj >= p_lo) {
                l = std::max(l, llev[F.ci[j]] + 1);
                max_dist = std::max(max_dist, p - pj);
            }
        }
        llev[i] = l;
    }
    // rows of each block sorted by (local level, position)
    bd.rows.assign(n, 0);
    bd.blk_lvl.assign(bd.nblocks + 1, 0);
    bd.lvl_ptr.clear();
    std::vector<int64_t> cnt;
    for (int64_t b = 0; b < bd.nblocks; ++b) {
        const int64_t p_lo = b * B, p_hi = std::min(n, p_lo + B);
        int32_t maxl = 0;
        for (int64_t p = p_lo; p < p_hi; ++p) maxl = std::max(maxl, llev[F.row(p)]);
        cnt.assign((size_t)maxl + 2, 0);
        for (int64_t p = p_lo; p < p_hi; ++p) cnt[llev[F.row(p)] + 1]++;
        for (int32_t l = 0; l <= maxl; ++l) cnt[l + 1] += cnt[l];
        bd.blk_lvl[b] = (int64_t)bd.lvl_ptr.size();
        for (int32_t l = 0; l <= maxl; ++l) bd.lvl_ptr.push_back(p_lo + cnt[l]);
        std::vector<int64_t> fillp(cnt.begin(), cnt.end() - 1);
        for (int64_t p = p_lo; p < p_hi; ++p) {
            const int64_t i = F.row(p);
            bd.rows[p_lo + fillp[llev[i]]++] = (int32_t)i;
        }
    }
    bd.blk_lvl[bd.nblocks] = (int64_t)bd.lvl_ptr.size();
    bd.lvl_ptr.push_back(n);
    // LDS ring: W = pow2 >= max in-block dependency distance + 1; the slot of position p is next
    // written by position p+W, which must come at a later local level than p itself and than every
    // in-block reader of p
    bd.ring_words = 0;
    int64_t W = 1;
    while (W < max_dist + 1) W <<= 1;
    if (W <= kRingMaxWords) {
        std::vector<int32_t> maxcons(n, -1);   // by position
        for (int64_t p = 0; p < n; ++p) {
            const int64_t i = F.row(p), p_lo = (p / B) * B;
            for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j) {
                const int64_t pj = F.pos(F.ci[j]);
                if (pj >= p_lo) maxcons[pj] = std::max(maxcons[pj], llev[i]);
            }
        }
        bool safe = true;
        for (int64_t p = 0; p < n && safe; ++p) {
            const int64_t q = p + W;
            if (q >= n || q / B != p / B) continue;
            const int32_t lq = llev[F.row(q)];
            if (lq <= llev[F.row(p)] || lq <= maxcons[p]) safe = false;
        }
        if (safe) bd.ring_words = (int32_t)W;
    }
    // simulated time: G resident workgroups take blocks round-robin, in order
    const size_t lds = band_lds_bytes(bd.ring_words, K);
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(per_cu_max, (int64_t)(160 * 1024 / std::max<size_t>(lds, 1))));
    const int64_t G = (int64_t)num_cus * per_cu;
    bd.G = G;
    const double cl = bd.ring_words ? kBandLevelRingUs : kBandLevelMemUs;
    std::vector<double> fin(n, 0.0), wg_free((size_t)std::max<int64_t>(G, 1), 0.0);
    double tmax = 0.0;
    for (int64_t b = 0; b < bd.nblocks; ++b) {
        const int64_t p_lo = b * B;
        double t = wg_free[b % G];
        for (int64_t L = bd.blk_lvl[b]; L < bd.blk_lvl[b + 1]; ++L) {
            double tl = t;
            for (int64_t q = bd.lvl_ptr[L]; q < bd.lvl_ptr[L + 1]; ++q) {
                const int64_t i = bd.rows[q];
                for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j)
                    if (F.pos(F.ci[j]) < p_lo) tl = std::max(tl, fin[F.ci[j]] + kHopUs);
            }
            const int64_t width = bd.lvl_ptr[L + 1] - bd.lvl_ptr[L];
            tl += cl * (double)((width + kBlock - 1) / kBlock);
            for (int64_t q = bd.lvl_ptr[L]; q < bd.lvl_ptr[L + 1]; ++q) fin[bd.rows[q]] = tl;
            t = tl;
        }
        wg_free[b % G] = t;
        tmax = std::max(tmax, t);
    }
    bd.est = tmax;
}

// Grid schedule plan (sptrsv_grid_kernel): width w = the most frequent solve-order distance >= 2
// (the line length of a 2-D stencil), every dependency as (yd lines, xd positions) back, the
// smallest skew making ud = xd + g(y) - g(y - yd) >= 1 for all of them — the integer skew sigma
// (g(y) = sigma*y), then sigma - 1/2 (g(y) = ((2 sigma - 1) y + phase) >> 1, either phase) when that
// also holds — and the ring depth. Rejected
// (ok = false) when the factor is not such a stencil: wide rows (> 8 entries), a dependency 64 or
// more lines back, a skew above 8, more than kGridMaxPE patterns reaching into the band above, a
// ring deeper than kGridMaxRing, or too few dependencies at distance w to call it a grid.
// fitted: FD 8192^2 Gauss-Seidel factor (8192 + 8191 steps) 5.0 ms, SA level 3 of it (2731 + 3*4095) 3.9 ms
constexpr double kGridStepUs = 0.26, kGridLagUs = 2.0;
constexpr int64_t kGridMaxYd = 8;   // lines of the band above held in the poller's LDS ring

}  // namespace

void plan_grid(const HostFactor &F, GridPlan &g) {
    const int64_t n = F.n;
    g = GridPlan();
    if (n < 4096) return;
    int32_t kmax = 0;
    std::unordered_map<int64_t, int64_t> hist;
    int64_t ndeps = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t len = F.rp[i + 1] - F.rp[i];
        kmax = std::max(kmax, len);
        ndeps += len;
        if (i % 7) continue;   // a sample is enough for the histogram
        const int64_t p = F.pos(i);
        for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j) {
            const int64_t d = p - F.pos(F.ci[j]);
            if (d >= 2) hist[d]++;
        }
    }
    if (kmax == 0 || kmax > 8) return;
    // line-length candidates: the most frequent distances (a 9-point stencil ties w - 1, w and w + 1),
    // each holding at least ~1/8 of the rows; the first one that plans is taken
    std::vector<std::pair<int64_t, int64_t>> cand(hist.begin(), hist.end());   // (distance, count)
    std::sort(cand.begin(), cand.end(), [](const std::pair<int64_t, int64_t> &a, const std::pair<int64_t, int64_t> &b) {
        return a.second != b.second ? a.second > b.second : a.first < b.first;
    });
    int64_t w = 0;
    // patterns and skew, with grid position p + off: off = 0, or the offset that makes the solve order
    // START with a partial line (w - n mod w empty positions before it: an upper factor of a grid whose
    // last natural line is short, e.g. SA level 2 of -FD 8192^2, 1365 lines of 911 + one of 228)
    int64_t sigma2 = 0, phase = 0, maxyd = 0, maxud = 0, off = 0;
    std::vector<int32_t> ext_codes;
    // the dependency codes under g(y) = (s2 * y + ph) >> 1; false when a dependency is not >= 1 step back
    auto try_skew = [&](int64_t o, int64_t s2, int64_t ph) -> bool {
        maxud = 0;
        ext_codes.clear();
        for (int64_t i = 0; i < n; ++i) {
            const int64_t p = F.pos(i) + o, y = p / w, x = p % w;
            for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j) {
                const int64_t pd = F.pos(F.ci[j]) + o, yd = y - pd / w, xd = x - pd % w;
                const int64_t ud = xd + grid_g(s2, ph, y) - grid_g(s2, ph, y - yd);
                if (ud < 1 || ud >= 1023) return false;
                maxud = std::max(maxud, ud);
                const int32_t code = (int32_t)(ud * 64 + yd);
                if (yd >= 1 && std::find(ext_codes.begin(), ext_codes.end(), code) == ext_codes.end()) {
                    if ((int)ext_codes.size() == kGridMaxPE) return false;
                    ext_codes.push_back(code);
                }
            }
        }
        off = o;
        sigma2 = s2;
        phase = ph;
        return true;
    };
    auto try_off = [&](int64_t o) -> bool {
        int64_t sigma = 0;
        maxyd = 0;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t p = F.pos(i) + o, y = p / w, x = p % w;
            for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j) {
                const int64_t pd = F.pos(F.ci[j]) + o, yd = y - pd / w, xd = x - pd % w;
                if (yd > kGridMaxYd) return false;
                maxyd = std::max(maxyd, yd);
                if (yd >= 1 && xd < 1) sigma = std::max(sigma, (1 - xd + yd - 1) / yd);
            }
        }
        if (sigma > 8) return false;
        // half a step less skew when the dependencies that need sigma occur on every other line only
        // (round 4: AMG level 3 2.67 -> 2.20 ms, profiles/r4_half_skew_ab.txt)
        constexpr bool half = true;
        if (half && sigma >= 2 && (try_skew(o, 2 * sigma - 1, 0) || try_skew(o, 2 * sigma - 1, 1))) return true;
        return try_skew(o, 2 * sigma, 0);
    };
    bool planned = false;
    for (size_t ci = 0; ci < cand.size() && ci < 4 && !planned; ++ci) {
        w = cand[ci].first;
        if (w < 2 || cand[ci].second * 7 * 8 < n) break;
        planned = try_off(0) || (n % w != 0 && try_off(w - n % w));
    }
    if (!planned) return;
    // ring rows: the deepest dependency, and room for the poller to stay a 64-position chunk ahead
    int ring = ext_codes.empty() ? 1 : 2 * kGridLanes;
    while (ring < maxud + 1 + (ext_codes.empty() ? 0 : kGridLanes)) ring <<= 1;
    if (ring > kGridMaxRing) return;
    g.ok = true;
    g.w = w;
    g.off = off;
    g.H = (n + off + w - 1) / w;
    g.sigma2 = sigma2;
    g.phase = phase;
    g.K = kmax <= 2 ? 2 : (kmax <= 4 ? 4 : 8);
    g.pe = (int)ext_codes.size();
    g.maxyd = (int)maxyd;
    g.ring = ring;
    for (int e = 0; e < g.pe; ++e) {
        const int32_t yd = ext_codes[e] & 63;
        g.ext.delta[e] = ext_codes[e];
        g.ext.yd[e] = yd;
    }
    const int64_t nbands = (g.H + kGridLanes - 1) / kGridLanes;
    g.est = (double)((w - 1) + grid_g(sigma2, phase, g.H - 1) + 1) * kGridStepUs + (double)nbands * kGridLagUs;
    (void)ndeps;
}

namespace {

// Partitioned schedule (sptrsv_part_kernel). Strip of row i: its natural index nat[i] cut into P
// equal ranges; strip s runs on workgroup (s % 8) * (P / 8) + s / 8, so neighbouring strips share an
// XCD (dispatch deals workgroups round-robin over the 8 XCDs). Two cost models (us): the PRIORITY
// model orders each strip's rows (ASAP finish times: a dependency inside the strip a, across strips
// b, a row c), the ESTIMATE model simulates the resulting schedule with constants fitted to MI355X
// measurements of the kernel (tools/ilu_probe.py, tools/part_micro.py: a wave's row costs ~0.5 us
// of issue and memory latency even when its dependencies are done; an LDS hand-off ~0.2 us
// including the row total and division; a published-value hand-off between CUs ~2 us under load).
// Strips longer than kPartMaxStrip rows measured slower than sync-free (FD 2896^2 ILUT: 32.8k rows
// per strip, 31.4 vs ~27 ms) and are not planned.
constexpr double kPartPrioLocalUs = 0.10, kPartPrioRemoteUs = 1.2, kPartPrioRowUs = 0.15;
constexpr double kPartEstLocalUs = 0.20, kPartEstRemoteUs = 2.0, kPartEstRowUs = 0.5;
constexpr int64_t kPartMaxStrip = 16384;

struct PartPlan {
    int P = 0;
    double est = -1.0;
    std::vector<int32_t> wg, lpos;   // workgroup and local position of every row
    std::vector<int64_t> seg;        // P + 1
};

void plan_part(const HostFactor &F, const std::vector<int32_t> &nat, int P, PartPlan &pp) {
    const int64_t n = F.n;
    pp.P = P;
    pp.wg.assign(n, 0);
    const int per = std::max(1, P / 8);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t s = (nat.empty() ? i : nat[i]) * P / n;
        pp.wg[i] = (P % 8 == 0) ? (int32_t)((s % 8) * per + s / 8) : (int32_t)s;
    }
    // ASAP finish times in solve order (a topological order)
    std::vector<double> fin(n, 0.0);
    for (int64_t p = 0; p < n; ++p) {
        const int64_t i = F.row(p);
        double t = 0.0;
        for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j)
            t = std::max(t, fin[F.ci[j]] + (pp.wg[F.ci[j]] == pp.wg[i] ? kPartPrioLocalUs : kPartPrioRemoteUs));
        fin[i] = t + kPartPrioRowUs;
    }
    // every workgroup's rows in ASAP order (ties: solve order)
    std::vector<int32_t> idx(n);
    for (int64_t i = 0; i < n; ++i) idx[i] = (int32_t)i;
    std::sort(idx.begin(), idx.end(), [&](int32_t u, int32_t v) {
        if (pp.wg[u] != pp.wg[v]) return pp.wg[u] < pp.wg[v];
        if (fin[u] != fin[v]) return fin[u] < fin[v];
        return F.pos(u) < F.pos(v);
    });
    pp.seg.assign((size_t)P + 1, 0);
    pp.lpos.assign(n, 0);
    for (int64_t k = 0; k < n; ++k) pp.seg[(size_t)pp.wg[idx[k]] + 1]++;
    for (int w = 0; w < P; ++w) pp.seg[w + 1] += pp.seg[w];
    for (int64_t k = 0; k < n; ++k) pp.lpos[idx[k]] = (int32_t)(k - pp.seg[pp.wg[idx[k]]]);
    // simulate: rows in global ASAP order, wave lpos % 16 of their workgroup
    std::sort(idx.begin(), idx.end(), [&](int32_t u, int32_t v) { return fin[u] != fin[v] ? fin[u] < fin[v] : F.pos(u) < F.pos(v); });
    std::vector<double> done(n, 0.0), wfree((size_t)P * kPartWaves, 0.0);
    double tmax = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t i = idx[k];
        double &wf = wfree[(size_t)pp.wg[i] * kPartWaves + pp.lpos[i] % kPartWaves];
        double t = wf;
        for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j) {
            const int32_t d = F.ci[j];
            const bool loc = pp.wg[d] == pp.wg[i] && pp.lpos[i] - pp.lpos[d] < kPartSlots;
            t = std::max(t, done[d] + (loc ? kPartEstLocalUs : kPartEstRemoteUs));
        }
        done[i] = wf = t + kPartEstRowUs;
        tmax = std::max(tmax, done[i]);
    }
    pp.est = tmax;
}

}  // namespace

// Split one host CSR factor into off-diagonal entries + diagonal. lower: entries must have c <= i.
int split_factor(int64_t n, const int32_t *rp, const int32_t *ci, const double *va, bool lower, bool unit,
                        std::vector<int32_t> &orp, std::vector<int32_t> &oci, std::vector<double> &ova,
                        std::vector<double> &dg) {
    orp.assign(n + 1, 0);
    if (!unit) dg.assign(n, 0.0);
    const char *what = lower ? "lower factor" : "upper factor";
    if (rp[0] != 0) return fail(PSK_ERR_ARG, std::string(what) + ": rowptr[0] != 0");
    for (int64_t i = 0; i < n; ++i) {
        if (rp[i + 1] < rp[i]) return fail(PSK_ERR_ARG, std::string(what) + ": rowptr not monotone");
        bool has_diag = false;
        for (int32_t j = rp[i]; j < rp[i + 1]; ++j) {
            const int32_t c = ci[j];
            if (c < 0 || c >= n || (lower ? c > i : c < i))
                return fail(PSK_ERR_ARG, std::string(what) + ": entry on the wrong side of the diagonal");
            if (c == i) {
                if (!unit) dg[i] += va[j];
                has_diag = true;
                continue;
            }
            oci.push_back(c);
            ova.push_back(va[j]);
        }
        if (!unit && !has_diag) return fail(PSK_ERR_ARG, std::string(what) + ": missing diagonal entry");
        orp[i + 1] = (int32_t)oci.size();
    }
    return PSK_OK;
}

namespace {

// The 5-point grid signature of an upper factor (TriFactor::fd5_*): triu of a 5-point operator on an m x H grid
// with one value per diagonal. amg_gs_pair.hip fuses two Gauss-Seidel sweeps of such a level into one launch.
static void detect_fd5(int64_t n, const std::vector<int32_t> &rp, const std::vector<int32_t> &ci,
                       const std::vector<double> &va, const std::vector<double> &dg, TriFactor &T) {
    T.fd5_m = 0;
    if (n < 4 || dg.empty() || rp[1] - rp[0] != 2) return;
    const int64_t m = std::max(ci[rp[0]], ci[rp[0] + 1]);
    if (m < 2 || n % m != 0 || n / m < 2) return;
    auto same = [](double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; };
    const double d = dg[0];
    double a1 = 0.0, am = 0.0;
    bool h1 = false, hm = false;
    int mfirst = -1;
    for (int64_t i = 0; i < n; ++i) {
        if (!same(dg[i], d)) return;
        const bool e1 = i % m != m - 1, em = i + m < n;
        const int32_t a = rp[i], e = rp[i + 1];
        if (e - a != (int)e1 + (int)em) return;
        bool s1 = false, sm = false;
        for (int32_t k = a; k < e; ++k) {
            const int64_t c = ci[k];
            if (e1 && !s1 && c == i + 1) {
                s1 = true;
                if (!h1) a1 = va[k], h1 = true;
                else if (!same(va[k], a1)) return;
            } else if (em && !sm && c == i + m) {
                sm = true;
                if (!hm) am = va[k], hm = true;
                else if (!same(va[k], am)) return;
            } else {
                return;
            }
        }
        if (e1 && em) {
            const int f = ci[a] == i + m;
            if (mfirst < 0) mfirst = f;
            else if (f != mfirst) return;
        }
    }
    if (!h1 || !hm || mfirst < 0) return;
    T.fd5_m = m;
    T.fd5_d = d;
    T.fd5_a1 = a1;
    T.fd5_am = am;
    T.fd5_mfirst = mfirst;
}

// Band plan: candidates of one block per workgroup, and 2x / 4x / 8x more blocks; the cheapest eligible one in
// `best` (false: none). Eligible: at most 8 off-diagonal entries per row (record width K), levels at most one
// chunk wide, LDS fits a CU. narrow (one solving wave, staging waves): every local level at most one wave
// wide, ring present; the estimate is then the narrow kernel's.
bool plan_band(const HostFactor &F, int32_t kmax, int num_cus, Band &best, int &K, bool &narrow) {
    const int64_t n = F.n;
    K = 1;
    while (K < kmax) K <<= 1;
    best = Band();
    best.est = -1.0;
    bool band_ok = false;
    auto widest = [](const Band &bd) {
        int64_t wmax = 0;
        for (size_t L = 0; L + 1 < bd.lvl_ptr.size(); ++L) wmax = std::max(wmax, bd.lvl_ptr[L + 1] - bd.lvl_ptr[L]);
        return wmax;
    };
    for (int64_t nb : {(int64_t)num_cus, 2 * (int64_t)num_cus, 4 * (int64_t)num_cus, 8 * (int64_t)num_cus}) {
        if (n == 0 || kmax > 8) break;
        const int64_t B = std::max<int64_t>(64, (n + nb - 1) / nb);
        Band bd;
        build_band(F, B, num_cus, 2, K, bd);
        const bool ok = widest(bd) <= kBandChunk && band_lds_bytes(bd.ring_words, K) <= 160 * 1024 - 64;   // + the static block ticket
        if (ok && (!band_ok || bd.est < best.est)) {
            best = std::move(bd);
            band_ok = true;
        }
        if (B == 64) break;
    }
    narrow = false;
    if (band_ok && best.ring_words > 0 && narrow_lds_bytes(best.ring_words, K) <= 160 * 1024 - 64) {
        const char *ne = std::getenv("PSK_BAND_NARROW");
        narrow = widest(best) <= kNarrowWidth && !(ne && std::atoi(ne) == 0);
        if (narrow) best.est *= kNarrowLevelUs / kBandLevelRingUs;   // levels dominate the simulated time
    }
    return band_ok;
}

// the band record stream of plan `best` (kept whenever a band is feasible: psk_prec_trisolve_schedule may select
// it later)
void pack_band(const HostFactor &F, const std::vector<double> &ova, const Band &best, int K, bool narrow, FactorPlan &out) {
    const int64_t n = F.n;
    const std::vector<double> &dg = out.dg;
    std::vector<int32_t> &rrow = out.rec_row, &rend = out.rec_end, &rc_ = out.rec_c;
    std::vector<double> &rv = out.rec_v, &rd = out.rec_d;
    TriFactor::Band &b = out.T.band;
    b.K = K;
    b.B = best.B;
    b.nblocks = best.nblocks;
    b.ring_words = best.ring_words;
    b.narrow = narrow;
    rrow.assign(n, 0);
    rend.assign(n, 0);
    rc_.assign((size_t)K * n, -1);
    rv.assign((size_t)K * n, 0.0);
    if (!dg.empty()) rd.assign(n, 1.0);
    for (int64_t b = 0; b < best.nblocks; ++b) {
        const int64_t p_lo = b * best.B;
        for (int64_t L = best.blk_lvl[b]; L < best.blk_lvl[b + 1]; ++L)
            for (int64_t q = best.lvl_ptr[L]; q < best.lvl_ptr[L + 1]; ++q) {
                const int32_t i = best.rows[q];
                rrow[q] = i;
                rend[q] = (int32_t)(best.lvl_ptr[L + 1] - p_lo);
                int k = 0;
                for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j, ++k) {
                    rc_[(size_t)k * n + q] = F.ci[j];
                    rv[(size_t)k * n + q] = ova[j];
                }
                if (!dg.empty()) rd[q] = dg[i];
            }
    }
}

// the grid layout of plan gp (kept whenever plan_grid succeeds): per-step records, or their dictionary
void pack_grid(const HostFactor &F, const std::vector<double> &ova, const GridPlan &gp, FactorPlan &out) {
    const int64_t n = F.n;
    const std::vector<double> &dg = out.dg;
    std::vector<double> &gcoef = out.gcoef, &gdict = out.gdict;
    std::vector<uint32_t> &gidx = out.gidx;
    TriFactor::Grid &G = out.T.grid;
    G.K = gp.K;
    G.pe = gp.pe;
    G.maxyd = gp.maxyd;
    G.w = gp.w;
    G.H = gp.H;
    G.sigma = gp.sigma2;
    G.phase = gp.phase;
    G.off = gp.off;
    G.ext = gp.ext;
    // grid position p + off = (y*w + x): band b = y / 64, lane y % 64, step u - g(64b) with u = x + g(y);
    // one GridStep block per (band, step): codes (ud*64 + yd), values in stored order, diagonal.
    // Padding: value 0, code 0 (the lane's own column of the current row); empty lanes: diagonal 1
    // so the wave's unused results stay finite (padding entries read them times 0.0)
    // steps per band: g(y0 + 63) - g(y0) is the same for every band (sigma2 * y0 is even)
    G.S = (gp.w - 1) + grid_g(gp.sigma2, gp.phase, kGridLanes - 1) - grid_g(gp.sigma2, gp.phase, 0) + 1;
    const int64_t SB = gp.K == 2 ? GridStep<2>::kBytes : gp.K == 4 ? GridStep<4>::kBytes : GridStep<8>::kBytes;
    const int64_t nb = (gp.H + kGridLanes - 1) / kGridLanes, nsteps = nb * G.S;
    const int64_t oc = kGridLanes * 2 * gp.K, od = oc + kGridLanes * 8 * gp.K;
    gcoef.assign((size_t)(nsteps * SB / 8), 0.0);
    unsigned char *gb = reinterpret_cast<unsigned char *>(gcoef.data());
    for (int64_t t = 0; t < nsteps; ++t)
        for (int l = 0; l < kGridLanes; ++l) reinterpret_cast<double *>(gb + t * SB + od)[l] = 1.0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t p = F.pos(i) + gp.off, y = p / gp.w, x = p % gp.w, b = y / kGridLanes, l = y % kGridLanes;
        const int64_t st = x + grid_g(gp.sigma2, gp.phase, y) - grid_g(gp.sigma2, gp.phase, kGridLanes * b);
        unsigned char *blk = gb + (b * G.S + st) * SB;
        uint16_t *codes = reinterpret_cast<uint16_t *>(blk) + l * gp.K;
        double *vals = reinterpret_cast<double *>(blk + oc) + l * gp.K;
        int k = 0;
        for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j, ++k) {
            const int64_t pd = F.pos(F.ci[j]) + gp.off, yd = y - pd / gp.w, xd = x - pd % gp.w;
            codes[k] = (uint16_t)((xd + grid_g(gp.sigma2, gp.phase, y) - grid_g(gp.sigma2, gp.phase, y - yd)) * 64 + yd);
            vals[k] = ova[j];
        }
        reinterpret_cast<double *>(blk + od)[l] = dg.empty() ? 1.0 : dg[i];
    }
    // record dictionary: when the lane-steps hold at most kGridDictMax distinct records (stencil
    // factors: the interior record, the boundary variants, the empty lanes), the kernel loads one
    // 32-bit index per lane-step instead of the record (PSK_TRISOLVE_GRID_DICT=0: never)
    const char *gde = std::getenv("PSK_TRISOLVE_GRID_DICT");
    if (!(gde && std::atoi(gde) == 0))
        build_grid_dict(gb, nsteps, SB, gp.K, oc, od, gidx, gdict, G.dict_n);
    // the dictionary kernel divides by Markstein correction from RN(1/d) (div_markstein), which
    // equals IEEE r / d only while 1/d, the quotient and the remainder stay normal: keep the
    // dictionary only for diagonals with 2^-100 <= |d| <= 2^100 (the kernel itself falls back to
    // r / d for right-hand sides outside [2^-900, 2^900]); otherwise the per-step records
    for (int i = 0; i < G.dict_n; ++i) {
        const double d = std::fabs(gdict[(size_t)G.dict_n * gp.K + (size_t)i]);
        if (!(d >= 0x1p-100 && d <= 0x1p+100)) {
            G.dict_n = 0;
            std::vector<double>().swap(gdict);
            std::vector<uint32_t>().swap(gidx);
            break;
        }
    }
    if (G.dict_n > 0) std::vector<double>().swap(gcoef);   // the records are not uploaded
}

// plan_levels: positions, slots and the estimate; false when the live values or the records do not fit.
struct LevelPlan {
    int W = 0, KM = 0;
    int64_t steps = 0;
    int32_t nslots = 0;
    std::vector<int64_t> pos;     // step * W + lane of every row
    std::vector<int32_t> slot;    // LDS slot of every row's value (-1: nobody reads it)
    double est = -1.0;
};

bool plan_levels(const HostFactor &F, const std::vector<int32_t> &order, const std::vector<int32_t> &lev, int64_t nlev,
                 int32_t kmax, LevelPlan &lp) {
    const int64_t n = F.n;
    std::vector<int64_t> &pos = lp.pos;
    std::vector<int32_t> &slot = lp.slot;
    int32_t &nslots = lp.nslots;
    std::vector<int64_t> lw((size_t)nlev, 0);
    for (int64_t i = 0; i < n; ++i) lw[(size_t)lev[(size_t)i]]++;
    int64_t wmax = 1;
    for (int64_t w : lw) wmax = std::max(wmax, w);
    const int W = (int)std::min<int64_t>(kLevelMaxW, (wmax + 63) / 64 * 64);
    // positions: level by level in `order`, each level padded to whole steps of W
    pos.assign((size_t)n, 0);
    int64_t steps = 0;
    {
        int64_t q = 0;
        for (int64_t L = 0; L < nlev; ++L) {
            const int64_t cntL = lw[(size_t)L], st = (cntL + W - 1) / W;
            for (int64_t j = 0; j < cntL; ++j) pos[(size_t)order[(size_t)(q + j)]] = steps * W + j;
            q += cntL;
            steps += st;
        }
    }
    steps = (steps + kLevelPad - 1) / kLevelPad * kLevelPad;   // the kernel's loop: whole groups of D steps
    // slot of every value: the step of its last reader, then greedy interval allocation in step order
    std::vector<int64_t> last((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t j = F.rp[(size_t)i]; j < F.rp[(size_t)i + 1]; ++j)
            last[(size_t)F.ci[(size_t)j]] = std::max(last[(size_t)F.ci[(size_t)j]], pos[(size_t)i] / W);
    std::vector<int32_t> by_pos((size_t)steps * W, -1);
    slot.assign((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i) by_pos[(size_t)pos[(size_t)i]] = (int32_t)i;
    std::priority_queue<std::pair<int64_t, int32_t>, std::vector<std::pair<int64_t, int32_t>>,
                        std::greater<std::pair<int64_t, int32_t>>> live;   // (last reader step, slot)
    std::vector<int32_t> freed;
    nslots = 0;
    bool fits = true;
    for (int64_t st = 0; st < steps && fits; ++st) {
        while (!live.empty() && live.top().first < st) {   // its last reader ran in an earlier step
            freed.push_back(live.top().second);
            live.pop();
        }
        for (int64_t t = 0; t < W; ++t) {
            const int32_t i = by_pos[(size_t)(st * W + t)];
            if (i < 0 || last[(size_t)i] < 0) continue;   // idle lane / nobody reads it: the trash slot
            int32_t sl;
            if (!freed.empty()) {
                sl = freed.back();
                freed.pop_back();
            } else {
                sl = nslots++;
            }
            slot[(size_t)i] = sl;
            live.push({last[(size_t)i], sl});
        }
        fits = nslots + 2 <= kLevelMaxSlots;
    }
    const int KM = kmax <= 4 ? 4 : kmax <= 8 ? 8 : kmax <= 12 ? 12 : 16;
    fits = fits && steps * W * KM * 8 < ((int64_t)1 << 32);
    lp.W = W;
    lp.KM = KM;
    lp.steps = steps;
    lp.est = (double)steps * kLevelStepUs + (double)steps * W * (24.0 + 10.0 * KM) / kLevelBytesPerUs;
    return fits;
}

// the levels layout of plan lp (kept only when the schedule is chosen or forced)
void pack_levels(const HostFactor &F, const std::vector<double> &ova, const LevelPlan &lp, FactorPlan &out) {
    const int64_t n = F.n, steps = lp.steps, R = lp.nslots, zero = R, trash = R + 1;
    const int W = lp.W, KM = lp.KM;
    const std::vector<int64_t> &pos = lp.pos;
    const std::vector<int32_t> &slot = lp.slot;
    const std::vector<double> &dg = out.dg;
    std::vector<uint64_t> &lrc = out.lrc, &lsl = out.lsl;
    std::vector<double> &lcf = out.lcf, &ldg = out.ldg;
    out.T.lv.steps = steps;
    out.T.lv.W = W;
    out.T.lv.R = (int)R;
    out.T.lv.KM = KM;
    const size_t NP = (size_t)steps * W;
    lrc.assign(NP, (uint64_t)kLevelIdle | ((uint64_t)trash << 40));
    lsl.assign(NP * (KM / 4), (uint64_t)zero * 0x0001000100010001ull);
    lcf.assign(NP * KM, -0.0);
    ldg.assign(NP, 1.0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t p = pos[(size_t)i], st = p / W, t = p % W;
        const int32_t a = F.rp[(size_t)i], e = F.rp[(size_t)i + 1];
        const uint64_t ws = slot[(size_t)i] >= 0 ? (uint64_t)slot[(size_t)i] : (uint64_t)trash;
        lrc[(size_t)p] = (uint64_t)(uint32_t)i | (ws << 40);
        for (int32_t j = a; j < e; ++j) {
            const int k = j - a;
            const uint64_t ds = (uint64_t)slot[(size_t)F.ci[(size_t)j]];   // read: it has a reader
            uint64_t &w = lsl[((size_t)st * (KM / 4) + (size_t)(k / 4)) * W + (size_t)t];
            w = (w & ~((uint64_t)0xFFFF << (16 * (k % 4)))) | (ds << (16 * (k % 4)));
            // coefficient pairs (2k2, 2k2 + 1) of lane t: one 16-byte load
            lcf[(((size_t)st * (KM / 2) + (size_t)(k / 2)) * W + (size_t)t) * 2 + (size_t)(k % 2)] = ova[(size_t)j];
        }
        if (!dg.empty()) ldg[(size_t)p] = dg[(size_t)i];
    }
}

// the partitioned layout of plan pp (kept only when the schedule is chosen or forced)
void pack_part(const HostFactor &F, const std::vector<double> &ova, const PartPlan &pp, FactorPlan &out) {
    const int64_t n = F.n;
    std::vector<int32_t> &prp = out.prp, &pcode = out.pcode, &prow = out.prow;
    std::vector<double> &pva = out.pva;
    out.T.part.P = pp.P;
    out.pseg = pp.seg;
    prow.assign(n, 0);
    prp.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t k = pp.seg[pp.wg[i]] + pp.lpos[i];
        prow[k] = (int32_t)i;
        prp[k + 1] = F.rp[i + 1] - F.rp[i];
    }
    for (int64_t k = 0; k < n; ++k) prp[k + 1] += prp[k];
    pcode.assign(F.ci.size() + kPartPadEntries, 0);   // padding: the kernel's unconditional loads
    pva.assign(F.ci.size() + kPartPadEntries, 0.0);
    for (int64_t k = 0; k < n; ++k) {
        const int32_t i = prow[k];
        int32_t o = prp[k];
        for (int32_t j = F.rp[i]; j < F.rp[i + 1]; ++j, ++o) {
            const int32_t d = F.ci[j];
            const bool loc = pp.wg[d] == pp.wg[i] && pp.lpos[i] - pp.lpos[d] < kPartSlots;
            pcode[o] = loc ? ~pp.lpos[d] : d;   // ~q = -q-1 < 0: the strip's q-th row
            pva[o] = ova[j];
        }
    }
}

// the sync-free kernel's copy of the factor, in solve order (position k = row order[k])
void pack_syncfree(const HostFactor &F, const std::vector<double> &ova, FactorPlan &out) {
    const int64_t n = F.n;
    const std::vector<int32_t> &order = out.order;
    std::vector<int32_t> &krp = out.krp, &kci = out.kci;
    std::vector<double> &kva = out.kva;
    krp.assign((size_t)n + 1, 0);
    kci.resize(F.ci.size());
    kva.resize(ova.size());
    for (int64_t k = 0; k < n; ++k) {
        const int32_t i = order[(size_t)k], a = F.rp[(size_t)i], e = F.rp[(size_t)i + 1];
        std::copy(F.ci.begin() + a, F.ci.begin() + e, kci.begin() + krp[(size_t)k]);
        std::copy(ova.begin() + a, ova.begin() + e, kva.begin() + krp[(size_t)k]);
        krp[(size_t)k + 1] = krp[(size_t)k] + (e - a);
    }
}

}  // namespace

// Plan one factor: split it, estimate every schedule it is eligible for, choose, pack the layouts.
// Candidates in the order sync-free, band, LDS, grid, levels, partitioned; each takes over on a strictly
// smaller estimate than the schedule chosen so far (or when its environment variable forces it).
int plan_factor(int64_t n, const int32_t *rp, const int32_t *ci, const double *va, bool upper, bool unit,
                const std::vector<int32_t> &nat, int num_cus, int64_t syncfree_waves, FactorPlan &out) {
    out = FactorPlan();
    TriFactor &T = out.T;
    HostFactor F;
    F.n = n;
    F.upper = upper;
    std::vector<double> ova;
    PSK_TRY(split_factor(n, rp, ci, va, !upper, unit, F.rp, F.ci, ova, out.dg));
    if (upper && !unit && nat.empty()) detect_fd5(n, F.rp, F.ci, ova, out.dg, T);
    std::vector<int32_t> lev;
    int64_t nlev = 0;
    level_order(F, out.order, lev, nlev);
    int32_t kmax = 0;
    for (int64_t i = 0; i < n; ++i) kmax = std::max(kmax, F.rp[i + 1] - F.rp[i]);
    double(&est)[6] = T.est_us;
    std::fill(est, est + 6, -1.0);
    // a candidate's estimate; true when it is now the chosen schedule
    auto offer = [&](int sched, double us, bool force = false) {
        est[sched] = us;
        if (force || us < est[T.schedule]) T.schedule = sched;
        return T.schedule == sched;
    };
    T.schedule = kSchedSyncFree;
    est[kSchedSyncFree] = simulate_syncfree(F, out.order, syncfree_waves);
    Band band;
    int K = 0;
    bool narrow = false;
    if (plan_band(F, kmax, num_cus, band, K, narrow)) {
        offer(kSchedBand, band.est);
        pack_band(F, ova, band, K, narrow, out);
    }
    // one workgroup with x in LDS: a level costs an LDS hand-off, the entries stream through one CU
    if (n > 0 && n <= kLdsMaxRows) offer(kSchedLds, (double)nlev * kLdsLevelUs + (double)F.ci.size() * 12.0 / kLdsBytesPerUs);
    // grid schedule (2-D stencil factors): records in solve order
    GridPlan gp;
    plan_grid(F, gp);
    if (n > kGridMaxRows) gp.ok = false;   // the grid kernel's 32-bit buffer offsets
    if (gp.ok) {
        offer(kSchedGrid, gp.est);
        pack_grid(F, ova, gp, out);
    }
    // levels schedule (sptrsv_levels_kernel): one workgroup of W = 64..256 lanes, one level (or a W-row
    // piece of one) per step, x in host-assigned LDS slots. Eligible: at most 16 entries per row, the values
    // alive at once (written, a reader still to come) within kLevelMaxSlots, records < 4 GB.
    // PSK_TRISOLVE_LEVELS=0 never plans it, =1 builds it and selects it whenever eligible.
    bool lv_forced = false;
    {
        const char *le = std::getenv("PSK_TRISOLVE_LEVELS");
        const bool force = le && std::atoi(le) == 1, off = le && std::atoi(le) == 0;
        LevelPlan lp;
        if (!off && n > 0 && n < (int64_t)kLevelIdle && kmax <= kLevelMaxK && plan_levels(F, out.order, lev, nlev, kmax, lp) &&
            offer(kSchedLevel, lp.est, force)) {
            lv_forced = force;
            pack_levels(F, ova, lp, out);
        }
    }
    // partitioned schedule: planned for factors too large for one CU and not solved by the grid
    // schedule (PSK_TRISOLVE_PART=0 disables it, =1 builds it and selects it whatever the estimate)
    {
        const char *pe = std::getenv("PSK_TRISOLVE_PART");
        const bool force = pe && std::atoi(pe) == 1, off = pe && std::atoi(pe) == 0;
        const int P = num_cus;   // one strip per CU (16-64 strips measured slower, round 5)
        const int64_t strip = (n + P - 1) / std::max(1, P);
        if (!off && !lv_forced && n > kLdsMaxRows && n >= (int64_t)P * kPartWaves &&
            (force || (T.schedule != kSchedGrid && strip <= kPartMaxStrip))) {
            PartPlan pp;
            plan_part(F, nat, P, pp);
            if (offer(kSchedPart, pp.est, force)) pack_part(F, ova, pp, out);
        }
    }
    if (const char *ve = std::getenv("PSK_TRISOLVE_VERBOSE"))   // development: the cost model's view
        if (std::atoi(ve))
            std::fprintf(stderr, "psk trisolve %s n=%lld levels=%lld est_us syncfree=%.0f band=%.0f lds=%.0f grid=%.0f "
                                 "part=%.0f levels=%.0f -> schedule %d\n",
                         upper ? "U" : "L", (long long)n, (long long)nlev, est[kSchedSyncFree], est[kSchedBand],
                         est[kSchedLds], est[kSchedGrid], est[kSchedPart], est[kSchedLevel], T.schedule);
    T.present = true;
    T.upper = upper;
    T.nnz = (int64_t)F.ci.size();
    T.levels = nlev;
    pack_syncfree(F, ova, out);
    return PSK_OK;
}

}  // namespace psk
