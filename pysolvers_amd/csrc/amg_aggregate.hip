// amg_aggregate.hip — the smoothed-aggregation setup of the AMG hierarchy: pure host arithmetic (no HIP call, no
// Context). psk_sa_aggregate restates BuildAggregates + BuildFilteredMatrix (SmoothedAggregation.py:41-183) in O(nnz)
// instead of the reference's set loops (quadratic in phase 2), with identical results (oracle/amg.py pins both).
#include "psk_internal.hpp"

#include <algorithm>
#include <cmath>

using namespace psk;

namespace {

struct SaState {
    int64_t n, nnz;   // the matrix: CSR, entries in stored order
    const int32_t *rowptr, *colidx;
    const double *vals;
    std::vector<double> d;               // A.diagonal()
    std::vector<uint8_t> strong;         // per entry: a strong coupling
    std::vector<int32_t> agg;            // per node: its aggregate, -1 while it has none
    std::vector<uint8_t> in_r, late;     // per node: not aggregated yet; aggregated by phase 2
    std::vector<int64_t> root;           // per aggregate: the node whose neighbourhood founded it
};

int sa_check_args(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const int32_t *agg_out,
                  const int64_t *count_out) {
    if (n < 0 || !rowptr || !agg_out || !count_out || (n > 0 && rowptr[n] > 0 && (!colidx || !vals)))
        return fail(PSK_ERR_ARG, "psk_sa_aggregate: bad arguments");
    const int64_t nnz = n > 0 ? rowptr[n] : 0;
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(PSK_ERR_ARG, "psk_sa_aggregate: rowptr not monotone");
    for (int64_t k = 0; k < nnz; ++k)
        if (colidx[k] < 0 || colidx[k] >= n) return fail(PSK_ERR_ARG, "psk_sa_aggregate: column out of range");
    return PSK_OK;
}

// strength (getNeighborhood, :49-54): abs(a_ij) >= tol*sqrt(a_ii*a_jj); N_i = {i} U strong
void sa_strength(SaState &S, double tol) {
    // A.diagonal(): sum of the row's diagonal entries in stored order (scipy csr_diagonal)
    S.d.assign(S.n, 0.0);
    for (int64_t i = 0; i < S.n; ++i)
        for (int32_t k = S.rowptr[i]; k < S.rowptr[i + 1]; ++k)
            if (S.colidx[k] == i) S.d[i] += S.vals[k];
    S.strong.assign(S.nnz, 0);
    for (int64_t i = 0; i < S.n; ++i)
        for (int32_t k = S.rowptr[i]; k < S.rowptr[i + 1]; ++k)
            S.strong[k] = std::fabs(S.vals[k]) >= tol * std::sqrt(S.d[i] * S.d[S.colidx[k]]);
}

template <class Pred>   // iterate N_i: i itself, then strong columns
bool sa_in_n(const SaState &S, int64_t i, Pred &&pred) {
    if (!pred((int32_t)i)) return false;
    for (int32_t k = S.rowptr[i]; k < S.rowptr[i + 1]; ++k)
        if (S.strong[k] && !pred(S.colidx[k])) return false;
    return true;
}

int sa_phase1(SaState &S) {
    S.agg.assign(S.n, -1);
    S.in_r.assign(S.n, 1);
    S.late.assign(S.n, 0);
    // isolated nodes: |N_i| == 1 (:73-77)
    for (int64_t i = 0; i < S.n; ++i) {
        bool iso = true;
        for (int32_t k = S.rowptr[i]; k < S.rowptr[i + 1] && iso; ++k)
            if (S.strong[k] && S.colidx[k] != i) iso = false;
        if (iso) {
            S.agg[i] = (int32_t)S.root.size();
            S.in_r[i] = 0;
            S.root.push_back(i);
        }
    }
    // phase 1 (:84-89): N_i entirely unaggregated -> new aggregate N_i
    for (int64_t i = 0; i < S.n; ++i) {
        if (!S.in_r[i]) continue;
        if (!sa_in_n(S, i, [&](int32_t j) { return S.in_r[j] != 0; })) continue;
        const int32_t id = (int32_t)S.root.size();
        sa_in_n(S, i, [&](int32_t j) {
            S.agg[j] = id;
            S.in_r[j] = 0;
            return true;
        });
        S.root.push_back(i);
    }
    const int64_t count = (int64_t)S.root.size();
    if (count == 0 && S.n > 0) return fail(PSK_ERR_ARG, "psk_sa_aggregate: no aggregates (reference: aggregates[-1] IndexError)");
    if (count >= INT32_MAX) return fail(PSK_ERR_UNSUPPORTED, "psk_sa_aggregate: too many aggregates");
    return PSK_OK;
}

// phase 2 (:104-127) against the phase-1 snapshot: candidates = aggregates meeting N_i; strength
// of a candidate = max |A[i,k]| over its members k (A[i,k] sums duplicate entries); strictly
// largest wins, first in list order on ties; none positive -> aggregates[-1]
void sa_phase2(SaState &S) {
    const int32_t *rowptr = S.rowptr, *colidx = S.colidx;
    const int64_t count = (int64_t)S.root.size();
    std::vector<int32_t> snap(S.agg);
    std::vector<int32_t> cand;
    std::vector<std::pair<int32_t, double>> colsum;   // (k, A[i,k]) for members of candidates
    for (int64_t i = 0; i < S.n; ++i) {
        if (!S.in_r[i]) continue;
        cand.clear();
        for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
            if (S.strong[k] && snap[colidx[k]] >= 0) cand.push_back(snap[colidx[k]]);
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        colsum.clear();
        for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            const int32_t j = colidx[k];
            if (snap[j] < 0 || !std::binary_search(cand.begin(), cand.end(), snap[j])) continue;
            bool merged = false;
            for (auto &e : colsum)
                if (e.first == j) {
                    e.second += S.vals[k];
                    merged = true;
                    break;
                }
            if (!merged) colsum.emplace_back(j, S.vals[k]);
        }
        double best = 0.0;
        int32_t best_c = -1;
        for (const int32_t cc : cand)   // list order
            for (const auto &e : colsum)
                if (snap[e.first] == cc && std::fabs(e.second) > best) {
                    best = std::fabs(e.second);
                    best_c = cc;
                }
        S.agg[i] = best_c >= 0 ? best_c : (int32_t)(count - 1);
        S.late[i] = 1;
    }
}

// BuildFilteredMatrix (:157-183). neighborhoods[i] as it reads them: the original N_i, grown by
// the phase-2 members of aggregate c when i is c's root (the reference's aggregate list holds
// the neighbourhood set objects themselves, :75/:88, and phase 2 adds to them, :126).
int sa_filter(const SaState &S, double *af_vals) {
    const int32_t *rowptr = S.rowptr, *colidx = S.colidx;
    std::vector<int32_t> root_of(S.n, -1);
    for (int64_t cidx = 0; cidx < (int64_t)S.root.size(); ++cidx) root_of[S.root[cidx]] = (int32_t)cidx;
    std::copy(S.vals, S.vals + S.nnz, af_vals);
    int64_t iptr = -1;
    for (int64_t i = 0; i < S.n; ++i) {
        const int32_t s = rowptr[i], e = rowptr[i + 1];
        for (int32_t k = s; k < e; ++k)
            if (colidx[k] == i) {
                iptr = k;
                break;
            }
        for (int32_t k = s; k < e; ++k) {
            const int32_t j = colidx[k];
            bool keep = (j == i);
            for (int32_t q = s; q < e && !keep; ++q) keep = S.strong[q] && colidx[q] == j;
            if (!keep && root_of[i] >= 0 && S.late[j] && S.agg[j] == root_of[i]) keep = true;
            if (keep) continue;
            if (iptr < 0) return fail(PSK_ERR_ARG, "psk_sa_aggregate: row without a diagonal entry (reference: NameError)");
            af_vals[iptr] -= af_vals[k];
            af_vals[k] = 0.0;
        }
    }
    return PSK_OK;
}

}  // namespace

extern "C" int psk_sa_aggregate(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                                double tol, int32_t *agg_out, int64_t *count_out, double *af_vals) {
    PSK_TRY(sa_check_args(n, rowptr, colidx, vals, agg_out, count_out));
    SaState S{n, n > 0 ? rowptr[n] : 0, rowptr, colidx, vals, {}, {}, {}, {}, {}, {}};
    sa_strength(S, tol);
    PSK_TRY(sa_phase1(S));
    sa_phase2(S);
    std::copy(S.agg.begin(), S.agg.end(), agg_out);
    *count_out = (int64_t)S.root.size();
    return af_vals ? sa_filter(S, af_vals) : PSK_OK;
}
