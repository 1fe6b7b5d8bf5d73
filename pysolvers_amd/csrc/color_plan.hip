// color_plan.hip — host colouring of a sparse matrix's rows for the multicolour Gauss-Seidel preconditioner
// (mcgs.hip): first-fit greedy in natural row order on the structure of A + A^T. Pure index arithmetic on host
// arrays: no HIP call and no Context, so the planner runs (and is tested, tests/test_mcgs_cpu.py through
// psk_color_plan) on a machine without a GPU, like trisolve_plan.hip and dist_plan.hip. Replaces nothing in the
// reference.
//
// The rule, fixed to the last detail (include/psk.h states the same; tests/mcgs_oracle.py restates it in Python):
// the neighbours of row i are the columns j != i stored in row i plus the rows j != i that store column i (stored
// zeros count); for i = 0..n-1 ascending, color[i] = the smallest c >= 0 that no neighbour j < i holds. O(nnz): A^T's
// structure by a counting sort, and per row a stamp array over colours (a row of degree d is given a colour <= d, so
// stamps[0..d] suffice and the search for the first free colour ends within d + 1 steps).
#include "../../include/psk.h"

#include <cstdint>
#include <string>
#include <vector>

namespace psk {
int fail(int code, const std::string &msg);   // runtime.hip
}

using namespace psk;

extern "C" int psk_color_plan(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t *color,
                              int32_t *ncolors) {
    if (!rowptr || !color || !ncolors) return fail(PSK_ERR_ARG, "psk_color_plan: NULL argument");
    if (n <= 0 || n >= INT32_MAX) return fail(PSK_ERR_ARG, "psk_color_plan: n must be in [1, 2^31 - 1)");
    if (rowptr[0] != 0) return fail(PSK_ERR_ARG, "psk_color_plan: row pointers must start at 0");
    const int64_t e0 = 0, nnz = rowptr[n];
    if (nnz < 0 || (nnz > 0 && !colidx)) return fail(PSK_ERR_ARG, "psk_color_plan: bad row pointers");
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(PSK_ERR_ARG, "psk_color_plan: row pointers decrease");
    // A^T's structure restricted to what the greedy pass reads: for column c the rows i < c that store it (a
    // neighbour j > i has no colour yet when row i is coloured). Counting sort by column.
    std::vector<int64_t> tptr((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = rowptr[i] - e0; e < rowptr[i + 1] - e0; ++e) {
            const int64_t c = colidx[e];
            if (c < 0 || c >= n) return fail(PSK_ERR_ARG, "psk_color_plan: column index out of range");
            if (i < c) ++tptr[(size_t)c + 1];
        }
    for (int64_t c = 0; c < n; ++c) tptr[(size_t)c + 1] += tptr[(size_t)c];
    std::vector<int32_t> trow((size_t)tptr[(size_t)n]);
    {
        std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
        for (int64_t i = 0; i < n; ++i)
            for (int64_t e = rowptr[i] - e0; e < rowptr[i + 1] - e0; ++e) {
                const int64_t c = colidx[e];
                if (i < c) trow[(size_t)fill[(size_t)c]++] = (int32_t)i;
            }
    }
    // stamp[c] == i + 1: colour c is held by a coloured neighbour of row i
    std::vector<int64_t> stamp;
    int32_t nc = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r0 = rowptr[i] - e0, r1 = rowptr[i + 1] - e0, t0 = tptr[(size_t)i], t1 = tptr[(size_t)i + 1];
        const size_t deg = (size_t)((r1 - r0) + (t1 - t0));
        if (stamp.size() < deg + 1) stamp.resize(deg + 1, 0);
        for (int64_t e = r0; e < r1; ++e) {
            const int64_t j = colidx[e];
            if (j < i && (size_t)color[j] <= deg) stamp[(size_t)color[j]] = i + 1;
        }
        for (int64_t e = t0; e < t1; ++e) {
            const int64_t j = trow[(size_t)e];   // j < i by construction
            if ((size_t)color[j] <= deg) stamp[(size_t)color[j]] = i + 1;
        }
        int32_t c = 0;
        while (stamp[(size_t)c] == i + 1) ++c;   // ends by c = deg: at most deg colours are stamped
        color[i] = c;
        if (c + 1 > nc) nc = c + 1;
    }
    *ncolors = nc;
    return PSK_OK;
}
