// asan_host.cpp — AddressSanitizer / UBSan run of libpsk's host-only C++ (no GPU touched):
// the MatrixMarket reader (psk_mm_info / psk_mm_read, mmio.hip), the smoothed-aggregation setup
// (psk_sa_aggregate, amg_aggregate.hip) and the row-block sharding plan (psk_fd2d_dist_plan, dist_plan.hip), on
// valid inputs and on malformed ones (every malformed file must be refused with an error code, never
// read out of bounds). Built and run by scripts/asan_host.sh against a libpsk whose host code is
// compiled with -fsanitize=address,undefined (device code unchanged); the log goes to profiles/.
// Development / verification tool only — not part of the product path.
#include "psk.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static int g_fail = 0;
#define CHECK(c, ...)                                    \
    do {                                                 \
        if (!(c)) {                                      \
            std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                    \
            std::printf("\n");                           \
            ++g_fail;                                    \
        }                                                \
    } while (0)

static std::string write_tmp(const std::string &name, const std::string &text) {
    const std::string p = "/tmp/psk_asan_" + name + ".mtx";
    FILE *f = std::fopen(p.c_str(), "wb");
    std::fwrite(text.data(), 1, text.size(), f);
    std::fclose(f);
    return p;
}

// read a file; returns psk status; nnz/n through the out parameters
static int mm_roundtrip(const std::string &path, int64_t *nr_out = nullptr, int64_t *nnz_out = nullptr) {
    int64_t nr = 0, nc = 0, nmax = 0;
    int rc = psk_mm_info(path.c_str(), &nr, &nc, &nmax);
    if (rc != PSK_OK) return rc;
    std::vector<int32_t> rp((size_t)nr + 1), ci((size_t)(nmax > 0 ? nmax : 1));
    std::vector<double> va((size_t)(nmax > 0 ? nmax : 1));
    int64_t nnz = 0;
    rc = psk_mm_read(path.c_str(), rp.data(), ci.data(), va.data(), &nnz);
    if (rc != PSK_OK) return rc;
    CHECK(nnz <= nmax, "%s: nnz %lld > nnz_max %lld", path.c_str(), (long long)nnz, (long long)nmax);
    CHECK(rp[0] == 0 && rp[(size_t)nr] == nnz, "%s: rowptr ends", path.c_str());
    for (int64_t i = 0; i < nr; ++i) {
        CHECK(rp[i] <= rp[i + 1], "%s: rowptr not monotone", path.c_str());
        for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
            CHECK(ci[k] >= 0 && ci[k] < nc, "%s: column out of range", path.c_str());
            if (k > rp[i]) CHECK(ci[k] > ci[k - 1], "%s: columns not sorted/unique", path.c_str());
        }
    }
    if (nr_out) *nr_out = nr;
    if (nnz_out) *nnz_out = nnz;
    return PSK_OK;
}

static void test_mmio(const char *golden_dir) {
    int ok = 0, refused = 0;
    for (const char *f : {"DH-Matrix-8.mtx", "DH-Matrix-10.mtx"}) {
        const std::string p = std::string(golden_dir) + "/" + f;
        int64_t nr = 0, nnz = 0;
        const int rc = mm_roundtrip(p, &nr, &nnz);
        CHECK(rc == PSK_OK && nr > 0 && nnz > 0, "%s rc %d", f, rc);
        ok += rc == PSK_OK;
    }
    const char *H = "%%MatrixMarket matrix coordinate real general\n";
    const std::vector<std::pair<std::string, std::string>> valid = {
        {"general", std::string(H) + "% comment\n\n3 3 4\n1 1 2.0\n3 1 -1e3\n2 2 .5\n1 1 1.0\n"},
        {"symmetric", "%%MatrixMarket matrix coordinate real symmetric\n3 3 3\n1 1 4\n2 1 -1\n3 3 4\n"},
        {"skew", "%%MatrixMarket matrix coordinate real skew-symmetric\n3 3 2\n2 1 1.5\n3 2 -2\n"},
        {"pattern", "%%MatrixMarket matrix coordinate pattern general\n2 3 2\n1 3\n2 1\n"},
        {"integer", "%%MatrixMarket matrix coordinate integer symmetric\n2 2 2\n1 1 7\n2 1 -3\n"},
        {"zeros", std::string(H) + "2 2 2\n1 1 0\n2 2 0.0\n"},
        {"empty", std::string(H) + "4 4 0\n"},
        {"crlf", "%%MatrixMarket matrix coordinate real general\r\n2 2 1\r\n2 2 3.5\r\n"},
    };
    for (const auto &t : valid) {
        const int rc = mm_roundtrip(write_tmp(t.first, t.second));
        CHECK(rc == PSK_OK, "valid file %s refused (rc %d)", t.first.c_str(), rc);
        ok += rc == PSK_OK;
    }
    // malformed: each must come back as an error (or, where scipy would accept it, a well-formed CSR)
    const std::vector<std::pair<std::string, std::string>> bad = {
        {"nofile_header", "3 3 1\n1 1 1\n"},
        {"array_format", "%%MatrixMarket matrix array real general\n2 2\n1\n2\n3\n4\n"},
        {"complex", "%%MatrixMarket matrix coordinate complex general\n1 1 1\n1 1 1 2\n"},
        {"truncated_entries", std::string(H) + "3 3 4\n1 1 2.0\n2 2\n"},
        {"row_oob", std::string(H) + "3 3 1\n4 1 1.0\n"},
        {"col_oob", std::string(H) + "3 3 1\n1 9 1.0\n"},
        {"row_zero", std::string(H) + "3 3 1\n0 1 1.0\n"},
        {"negative_size", std::string(H) + "-3 3 1\n1 1 1.0\n"},
        {"negative_nnz", std::string(H) + "3 3 -1\n"},
        {"huge_nnz", std::string(H) + "3 3 9000000000000000000\n1 1 1\n"},
        {"huge_dims", std::string(H) + "99999999999 3 1\n1 1 1\n"},
        {"garbage_value", std::string(H) + "2 2 1\n1 1 abc\n"},
        {"no_size_line", std::string(H)},
        {"empty_file", ""},
        {"symmetric_nonsquare", "%%MatrixMarket matrix coordinate real symmetric\n2 3 1\n1 1 1\n"},
        {"extra_entries", std::string(H) + "2 2 1\n1 1 1\n2 2 2\n"},
        {"long_line", std::string(H) + "2 2 1\n1 1 " + std::string(100000, '9') + "\n"},
    };
    for (const auto &t : bad) {
        const int rc = mm_roundtrip(write_tmp(t.first, t.second));
        refused += rc != PSK_OK;
        std::printf("  malformed %-22s -> %s\n", t.first.c_str(), rc == PSK_OK ? "read (well-formed CSR checked)" : "refused");
    }
    CHECK(mm_roundtrip("/tmp/psk_asan_does_not_exist.mtx") != PSK_OK, "missing file accepted");
    std::printf("mmio: %d valid files read, %d of %zu malformed refused\n", ok, refused, bad.size());
}

// 5-point FD Laplacian (m x m), rows sorted
static void fd2d(int m, std::vector<int32_t> &rp, std::vector<int32_t> &ci, std::vector<double> &va) {
    const int64_t n = (int64_t)m * m;
    rp.assign((size_t)n + 1, 0);
    ci.clear();
    va.clear();
    for (int64_t i = 0; i < n; ++i) {
        const int64_t y = i / m, x = i % m;
        const int64_t nb[5] = {i - m, i - 1, i, i + 1, i + m};
        const bool okb[5] = {y > 0, x > 0, true, x < m - 1, y < m - 1};
        for (int k = 0; k < 5; ++k)
            if (okb[k]) {
                ci.push_back((int32_t)nb[k]);
                va.push_back(k == 2 ? 4.0 : -1.0);
            }
        rp[(size_t)i + 1] = (int32_t)ci.size();
    }
}

static void test_sa() {
    int runs = 0;
    for (int m : {1, 2, 3, 17, 64, 200}) {
        std::vector<int32_t> rp, ci, agg;
        std::vector<double> va, af;
        fd2d(m, rp, ci, va);
        const int64_t n = (int64_t)m * m;
        agg.assign((size_t)n, -7);
        af.assign(va.size(), 0.0);
        int64_t count = 0;
        for (double tol : {0.08, 0.04, 0.0, 10.0}) {
            const int rc = psk_sa_aggregate(n, rp.data(), ci.data(), va.data(), tol, agg.data(), &count, af.data());
            CHECK(rc == PSK_OK, "sa fd m=%d tol=%g rc %d", m, tol, rc);
            if (rc != PSK_OK) continue;
            ++runs;
            CHECK(count >= 1 && count <= n, "sa count %lld", (long long)count);
            for (int64_t i = 0; i < n; ++i) CHECK(agg[i] >= 0 && agg[i] < count, "agg[%lld] = %d", (long long)i, agg[i]);
            double s = 0;
            for (double v : af) s += v;
            CHECK(std::isfinite(s), "af not finite");
        }
    }
    // random structurally symmetric matrices with a dominant diagonal
    uint64_t st = 12345;
    auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 33); };
    for (int trial = 0; trial < 40; ++trial) {
        const int n = 1 + (int)(rnd() % 400);
        std::vector<std::vector<std::pair<int, double>>> rows((size_t)n);
        for (int i = 0; i < n; ++i) rows[(size_t)i].push_back({i, 8.0 + (rnd() % 100) / 10.0});
        const int extra = (int)(rnd() % (3 * n + 1));
        for (int e = 0; e < extra; ++e) {
            const int i = (int)(rnd() % n), j = (int)(rnd() % n);
            if (i == j) continue;
            const double v = -((double)(rnd() % 1000) + 1) / 500.0;
            rows[(size_t)i].push_back({j, v});
            rows[(size_t)j].push_back({i, v});
        }
        std::vector<int32_t> rp(1, 0), ci, agg((size_t)n);
        std::vector<double> va;
        for (auto &r : rows) {
            std::sort(r.begin(), r.end());
            for (size_t k = 0; k < r.size(); ++k) {
                if (k && r[k].first == r[k - 1].first) { va.back() += r[k].second; continue; }
                ci.push_back(r[k].first);
                va.push_back(r[k].second);
            }
            rp.push_back((int32_t)ci.size());
        }
        std::vector<double> af(va.size());
        int64_t count = 0;
        const int rc = psk_sa_aggregate(n, rp.data(), ci.data(), va.data(), 0.08, agg.data(), &count, af.data());
        CHECK(rc == PSK_OK, "sa random n=%d rc %d", n, rc);
        if (rc == PSK_OK) ++runs;
    }
    // refused inputs: a row without its diagonal, a column out of range, rowptr not monotone
    {
        std::vector<int32_t> rp = {0, 1, 2}, ci = {1, 0}, agg(2);
        std::vector<double> va = {-1, -1}, af(2);
        int64_t count = 0;
        // the reference fails (NameError) only when such a row has an entry to lump; here every
        // entry is strong, so either outcome is the reference's: reported, not asserted
        const int rd = psk_sa_aggregate(2, rp.data(), ci.data(), va.data(), 0.08, agg.data(), &count, af.data());
        std::printf("  rows without a diagonal, nothing to lump -> %s\n", rd == PSK_OK ? "accepted" : "refused");
        ci = {0, 5};
        CHECK(psk_sa_aggregate(2, rp.data(), ci.data(), va.data(), 0.08, agg.data(), &count, af.data()) != PSK_OK,
              "column out of range accepted");
        rp = {0, 2, 1};
        ci = {0, 1};
        CHECK(psk_sa_aggregate(2, rp.data(), ci.data(), va.data(), 0.08, agg.data(), &count, af.data()) != PSK_OK,
              "rowptr not monotone accepted");
    }
    std::printf("sa_aggregate: %d runs, refused-input checks done\n", runs);
}

static void test_plan() {
    int plans = 0;
    for (int64_t m : {1, 2, 3, 7, 100, 3163, 16384}) {
        for (int P = 1; P <= 9; ++P) {
            int64_t prev_end = 0;
            for (int r = 0; r < P; ++r) {
                int64_t rb = -1, re = -1, nc = -1, hlo = -1, hhi = -1;
                const int rc = psk_fd2d_dist_plan(m, P, r, &rb, &re, &nc, &hlo, &hhi);
                if (rc != PSK_OK) { CHECK(P > m, "plan m=%lld P=%d refused", (long long)m, P); continue; }
                ++plans;
                CHECK(rb == prev_end && re >= rb && rb % m == 0 && re % m == 0, "plan rows");
                CHECK(nc == (re - rb) + hlo + hhi, "plan ncols");
                prev_end = re;
            }
            if (P <= m) CHECK(prev_end == m * m, "plan cover m=%lld P=%d", (long long)m, P);
        }
    }
    int64_t a, b, c, d, e;
    CHECK(psk_fd2d_dist_plan(10, 0, 0, &a, &b, &c, &d, &e) != PSK_OK, "P = 0 accepted");
    CHECK(psk_fd2d_dist_plan(10, 2, 2, &a, &b, &c, &d, &e) != PSK_OK, "rank >= P accepted");
    CHECK(psk_fd2d_dist_plan(-1, 2, 0, &a, &b, &c, &d, &e) != PSK_OK, "m < 0 accepted");
    std::printf("fd2d_dist_plan: %d plans checked\n", plans);
}

int main(int argc, char **argv) {
    const char *golden = argc > 1 ? argv[1] : "tests/golden/mtx";
    test_mmio(golden);
    test_sa();
    test_plan();
    std::printf("%s: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
    return g_fail ? 1 : 0;
}
