// dist_plan.hip — host planning of row-block shards: which rows a rank owns, how its columns map to
// [owned | halo], and what it sends to and receives from which peer. Pure index arithmetic on host arrays: no HIP
// or RCCL call and no Context, so the planner runs (and is tested, tests/test_dist_plan.py through
// psk_lab_dist_plan) on a machine without a GPU. dist.hip uploads what is planned here.
#include "dist.hpp"

#include <algorithm>
#include <climits>

namespace psk {

int fd2d_plan(int64_t m, int P, int r, FdPlan &p) {
    if (m < 1 || P < 1 || r < 0 || r >= P) return fail(PSK_ERR_ARG, "fd2d plan: bad arguments");
    if (P > m) return fail(PSK_ERR_ARG, "fd2d_dist: more ranks than grid lines");
    const int64_t l0 = m * r / P, l1 = m * (r + 1) / P;
    p.rb = l0 * m;
    p.re = l1 * m;
    p.nloc = p.re - p.rb;
    p.halo_lo = l0 > 0 ? m : 0;
    p.halo_hi = l1 < m ? m : 0;
    p.ncols = p.nloc + p.halo_lo + p.halo_hi;
    return PSK_OK;
}

void fd2d_peers(int64_t m, int r, const FdPlan &pl, std::vector<HaloPeer> &peers, std::vector<int64_t> &halo_cols) {
    peers.clear();
    halo_cols.clear();
    if (pl.halo_lo > 0) {
        HaloPeer p{};
        p.rank = r - 1;
        p.send_count = m;        // our first grid line
        p.send_begin = 0;
        p.recv_count = m;        // their last grid line -> halo_lo
        p.recv_offset = 0;
        peers.push_back(p);
        for (int64_t j = pl.rb - m; j < pl.rb; ++j) halo_cols.push_back(j);
    }
    if (pl.halo_hi > 0) {
        HaloPeer p{};
        p.rank = r + 1;
        p.send_count = m;        // our last grid line
        p.send_begin = pl.nloc - m;
        p.recv_count = m;        // their first grid line -> halo_hi
        p.recv_offset = pl.halo_lo;
        peers.push_back(p);
        for (int64_t j = pl.re; j < pl.re + m; ++j) halo_cols.push_back(j);
    }
}

// ---- general row-block sharding (psk_csr_create_dist) --------------------------------------
// Host plan of rank r's block, rows [rs[r], rs[r+1]) of a global CSR:
//  * local columns: owned c -> c - rb; every other referenced column -> nloc + its position in the
//    ascending list of distinct off-block columns (the halo), which is therefore grouped by owner
//    rank in rank order: the segment received from rank q is contiguous;
//  * send to q: the owned rows that have an entry in q's block, ascending. For a structurally
//    symmetric pattern that is exactly the list q receives from us (A[j][c] != 0 <=> A[c][j] != 0),
//    so it is built without communication; under RCCL the lists are exchanged once at creation and
//    compared (dist_verify, dist.hip), and every rank refuses a pattern that is not symmetric across ranks.
static int owner_of(const int64_t *rs, int P, int64_t c) {
    return (int)(std::upper_bound(rs, rs + P + 1, c) - rs) - 1;   // largest q with rs[q] <= c
}

int dist_plan(int64_t n_global, const int64_t *rs, int P, int r, const int64_t *rowptr, const int32_t *colidx,
              DistPlan &pl) {
    pl.rb = rs[r];
    pl.re = rs[r + 1];
    pl.nloc = pl.re - pl.rb;
    const int64_t e0 = rowptr[0], nnz = rowptr[pl.nloc] - e0;
    std::vector<int64_t> off;
    for (int64_t j = 0; j < nnz; ++j) {
        const int64_t c = colidx[j];
        if (c < 0 || c >= n_global) return fail(PSK_ERR_ARG, "psk_csr_create_dist: column index out of range");
        if (c < pl.rb || c >= pl.re) off.push_back(c);
    }
    std::sort(off.begin(), off.end());
    off.erase(std::unique(off.begin(), off.end()), off.end());
    pl.halo.swap(off);
    if (pl.nloc + (int64_t)pl.halo.size() >= INT32_MAX) return fail(PSK_ERR_UNSUPPORTED, "local columns exceed int32");
    pl.lcol.resize((size_t)nnz);
    pl.recv_off.assign((size_t)P, 0);
    pl.recv_cnt.assign((size_t)P, 0);
    pl.send_rows.assign((size_t)P, {});
    for (size_t k = 0; k < pl.halo.size(); ++k) {
        const int q = owner_of(rs, P, pl.halo[k]);
        if (pl.recv_cnt[(size_t)q] == 0) pl.recv_off[(size_t)q] = (int64_t)k;
        ++pl.recv_cnt[(size_t)q];
    }
    for (int64_t i = 0; i < pl.nloc; ++i)
        for (int64_t j = rowptr[i] - e0; j < rowptr[i + 1] - e0; ++j) {
            const int64_t c = colidx[j];
            if (c >= pl.rb && c < pl.re) {
                pl.lcol[(size_t)j] = (int32_t)(c - pl.rb);
                continue;
            }
            const int64_t k = std::lower_bound(pl.halo.begin(), pl.halo.end(), c) - pl.halo.begin();
            pl.lcol[(size_t)j] = (int32_t)(pl.nloc + k);
            std::vector<int32_t> &sr = pl.send_rows[(size_t)owner_of(rs, P, c)];
            if (sr.empty() || sr.back() != (int32_t)i) sr.push_back((int32_t)i);
        }
    return PSK_OK;
}

// A peer is every rank we send to or receive from. Rows sent as one contiguous run (row blocks of banded
// matrices) go straight from the vector; any other list is gathered through the pack list first.
void dist_peers(const DistPlan &pl, std::vector<HaloPeer> &peers, std::vector<int32_t> &pack) {
    peers.clear();
    pack.clear();
    for (size_t q = 0; q < pl.send_rows.size(); ++q) {
        const std::vector<int32_t> &sr = pl.send_rows[q];
        if (pl.recv_cnt[q] == 0 && sr.empty()) continue;
        HaloPeer p{};
        p.rank = (int)q;
        p.recv_count = pl.recv_cnt[q];
        p.recv_offset = pl.recv_off[q];
        p.send_count = (int64_t)sr.size();
        p.send_begin = sr.empty() ? 0 : sr[0];
        p.packed = !sr.empty() && (int64_t)sr.back() - sr.front() + 1 != (int64_t)sr.size();
        if (p.packed) {
            p.pack_off = (int64_t)pack.size();
            pack.insert(pack.end(), sr.begin(), sr.end());
        }
        peers.push_back(p);
    }
}

}  // namespace psk

using namespace psk;

extern "C" int psk_fd2d_dist_plan(int64_t m, int32_t nranks, int32_t rank, int64_t *row_begin, int64_t *row_end,
                                  int64_t *ncols, int64_t *halo_lo, int64_t *halo_hi) {
    FdPlan p;
    PSK_TRY(fd2d_plan(m, nranks, rank, p));
    if (row_begin) *row_begin = p.rb;
    if (row_end) *row_end = p.re;
    if (ncols) *ncols = p.ncols;
    if (halo_lo) *halo_lo = p.halo_lo;
    if (halo_hi) *halo_hi = p.halo_hi;
    return PSK_OK;
}
