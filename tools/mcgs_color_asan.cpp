// mcgs_color_asan.cpp — AddressSanitizer / UBSan run of the multicolour Gauss-Seidel planner (psk_color_plan,
// pysolvers_amd/csrc/color_plan.hip), which is plain host C++: a stand-alone program with its own main that colours a
// few generated matrices and checks every colouring (proper on A + A^T, first-fit: every row's colour is the smallest
// its earlier neighbours leave free) and every refusal. No GPU is touched and nothing of libpsk is linked; the one
// symbol the planner needs from the library (psk::fail) is defined here. Build and run (CPU only):
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude \
//       tools/mcgs_color_asan.cpp pysolvers_amd/csrc/color_plan.hip -o tools/bin/mcgs_color_asan
//   tools/bin/mcgs_color_asan > profiles/mcgs_color_asan.txt
// Development / verification tool only — not part of the product path.
#include "psk.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <string>
#include <vector>

namespace psk {
static std::string g_last;
int fail(int code, const std::string &msg) {
    g_last = msg;
    return code;
}
}  // namespace psk

static int g_fail = 0;
#define CHECK(c, ...)                                       \
    do {                                                    \
        if (!(c)) {                                         \
            std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                       \
            std::printf("\n");                              \
            ++g_fail;                                       \
        }                                                   \
    } while (0)

struct Csr {
    int64_t n = 0;
    std::vector<int32_t> rp, ci;
};

static Csr from_rows(const std::vector<std::vector<int32_t>> &rows) {
    Csr A;
    A.n = (int64_t)rows.size();
    A.rp.push_back(0);
    for (const auto &r : rows) {
        A.ci.insert(A.ci.end(), r.begin(), r.end());
        A.rp.push_back((int32_t)A.ci.size());
    }
    return A;
}

// colours A with exactly-sized arrays (so that any access past them is caught) and checks the result against the rule
static int color_and_check(const char *name, const Csr &A, int32_t want_colors) {
    std::vector<int32_t> color((size_t)A.n, -1);
    int32_t nc = -1;
    const int rc = psk_color_plan(A.n, A.rp.data(), A.ci.empty() ? nullptr : A.ci.data(), color.data(), &nc);
    CHECK(rc == PSK_OK, "%s: rc %d (%s)", name, rc, psk::g_last.c_str());
    if (rc != PSK_OK) return rc;
    std::vector<std::set<int32_t>> nb((size_t)A.n);
    for (int64_t i = 0; i < A.n; ++i)
        for (int32_t e = A.rp[i]; e < A.rp[i + 1]; ++e)
            if (A.ci[e] != i) {
                nb[(size_t)i].insert(A.ci[e]);
                nb[(size_t)A.ci[e]].insert((int32_t)i);
            }
    int32_t mx = -1;
    for (int64_t i = 0; i < A.n; ++i) {
        std::set<int32_t> used;
        for (int32_t j : nb[(size_t)i]) {
            CHECK(color[j] != color[i], "%s: rows %lld and %d share colour %d", name, (long long)i, j, color[i]);
            if (j < i) used.insert(color[j]);
        }
        int32_t c = 0;
        while (used.count(c)) ++c;
        CHECK(color[i] == c, "%s: row %lld has colour %d, first fit is %d", name, (long long)i, color[i], c);
        mx = std::max(mx, color[i]);
    }
    CHECK(nc == mx + 1, "%s: ncolors %d, max colour %d", name, nc, mx);
    if (want_colors > 0) CHECK(nc == want_colors, "%s: %d colours, expected %d", name, nc, want_colors);
    std::printf("%-28s n %7lld nnz %8zu colours %d\n", name, (long long)A.n, A.ci.size(), nc);
    return rc;
}

static Csr grid5(int m) {
    std::vector<std::vector<int32_t>> rows((size_t)m * m);
    for (int y = 0; y < m; ++y)
        for (int x = 0; x < m; ++x) {
            auto &r = rows[(size_t)y * m + x];
            const int32_t i = y * m + x;
            r.push_back(i);   // the stencil generator's stored order: diagonal first, unsorted
            if (y > 0) r.push_back(i - m);
            if (y < m - 1) r.push_back(i + m);
            if (x > 0) r.push_back(i - 1);
            if (x < m - 1) r.push_back(i + 1);
        }
    return from_rows(rows);
}

int main() {
    std::mt19937_64 rng(12345);
    color_and_check("5-point 16^2", grid5(16), 2);
    color_and_check("5-point 33^2", grid5(33), 2);
    color_and_check("5-point 301^2", grid5(301), 2);
    {
        std::vector<std::vector<int32_t>> rows(37);
        for (int i = 0; i < 37; ++i) rows[(size_t)i] = {i};
        color_and_check("diagonal 37", from_rows(rows), 1);
    }
    color_and_check("1 x 1", from_rows({{0}}), 1);
    color_and_check("1 x 1, no entry", from_rows({{}}), 1);
    {
        std::vector<std::vector<int32_t>> rows(70);
        for (int i = 0; i < 70; ++i)
            for (int j = 0; j < 70; ++j) rows[(size_t)i].push_back(j);
        color_and_check("dense 70", from_rows(rows), 70);
    }
    for (int n : {2, 17, 300, 5000}) {   // random, pattern not symmetric, unsorted rows, duplicate columns, empty rows
        std::vector<std::vector<int32_t>> rows((size_t)n);
        std::uniform_int_distribution<int> len(0, 9), col(0, n - 1);
        for (int i = 0; i < n; ++i) {
            const int k = len(rng);
            for (int e = 0; e < k; ++e) rows[(size_t)i].push_back(col(rng));
            if (k > 2) rows[(size_t)i].push_back(rows[(size_t)i][0]);   // a duplicate
        }
        color_and_check(("random " + std::to_string(n)).c_str(), from_rows(rows), 0);
    }
    {   // an arrow: row 0 and column 0 full, so row 0's degree is n - 1 and every other row's is small
        const int n = 2000;
        std::vector<std::vector<int32_t>> rows((size_t)n);
        for (int j = n - 1; j >= 0; --j) rows[0].push_back(j);
        for (int i = 1; i < n; ++i) rows[(size_t)i] = {i, i - 1};
        color_and_check("arrow 2000", from_rows(rows), 0);
    }
    // refusals: nothing may be read out of bounds on the way to the error
    {
        Csr A = grid5(4);
        std::vector<int32_t> color((size_t)A.n);
        int32_t nc = 0;
        CHECK(psk_color_plan(0, A.rp.data(), A.ci.data(), color.data(), &nc) == PSK_ERR_ARG, "n = 0");
        CHECK(psk_color_plan(-5, A.rp.data(), A.ci.data(), color.data(), &nc) == PSK_ERR_ARG, "n < 0");
        CHECK(psk_color_plan(A.n, nullptr, A.ci.data(), color.data(), &nc) == PSK_ERR_ARG, "NULL rowptr");
        CHECK(psk_color_plan(A.n, A.rp.data(), A.ci.data(), nullptr, &nc) == PSK_ERR_ARG, "NULL color");
        Csr B = A;
        B.ci[7] = (int32_t)A.n;
        CHECK(psk_color_plan(B.n, B.rp.data(), B.ci.data(), color.data(), &nc) == PSK_ERR_ARG, "column == n");
        B.ci[7] = -1;
        CHECK(psk_color_plan(B.n, B.rp.data(), B.ci.data(), color.data(), &nc) == PSK_ERR_ARG, "column < 0");
        B = A;
        for (auto &p : B.rp) p += 5;
        CHECK(psk_color_plan(B.n, B.rp.data(), B.ci.data(), color.data(), &nc) == PSK_ERR_ARG, "rowptr[0] != 0");
        B = A;
        B.rp[3] = B.rp[2] - 1;
        CHECK(psk_color_plan(B.n, B.rp.data(), B.ci.data(), color.data(), &nc) == PSK_ERR_ARG, "decreasing rowptr");
    }
    std::printf(g_fail ? "FAILED: %d checks\n" : "all checks passed (%d failures)\n", g_fail);
    return g_fail ? 1 : 0;
}
