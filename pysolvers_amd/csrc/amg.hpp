// amg.hpp — what the AMG files share (amg.hip, amg_gs_pair.hip) and what prec.hip, vcycle.hip and lab.hip call.
#pragma once
#include "psk_internal.hpp"

namespace psk {

// A level whose two consecutive Gauss-Seidel sweeps run as one launch (amg_gs_pair.hip gs_pair_kernel)
struct GsPairLevel {
    bool eligible = false, on = false;
    int64_t m = 0, H = 0, nbands = 0;
    int role[5] = {};     // A's stored diagonals in stored order: 0 = d, 1 = -m, 2 = +m, 3 = -1, 4 = +1
    int ord = -1;         // gs_pair_kernel's ORD: role == gp_role(ord, .)
    double v[5] = {};
    DevBuf pub;           // [nbands][3][m] publications of each band's last owned line
};

struct AmgHierarchy {
    int L = 0, num_iters = 0, nu_pre = 0, nu_post = 0;
    double tau = 0.0;
    std::vector<psk_csr *> A, P, R;
    std::vector<psk_prec *> S;
    psk_prec *coarse = nullptr;
    std::vector<DevBuf> x, f, r, t;   // per level (f unused on the finest level: f = v)
    DevBuf scal;                      // [0] = ||v||^2, [1] = flag (as int64), partials after
    std::vector<GsPairLevel> gp;      // per level
    DevBuf loop;                      // the standalone solver's device words (vcycle.hip), grow-only
};

// the pair's eligibility (host, at AMG creation), and x <- two sweeps from x, given r = f - A x
int gs_pair_setup(psk_csr *A, psk_prec *S, GsPairLevel &g, hipStream_t s);
int gs_pair_launch(const Context *c, const GsPairLevel &gl, const psk_prec *S, const double *f, const double *r,
                   double *x, hipStream_t s);
// AMG paired Gauss-Seidel sweeps (the lab library's switch): set -1 / 0 / 1, counts out
int amg_gs_pair(psk_prec *M, int set, int *on, int *eligible);
int amg_apply(const psk_prec *M, const double *v, double *out, hipStream_t s);
void amg_free(AmgHierarchy *h);
// the V-cycle loop's pieces, shared by amg_apply and psk_vcycle (vcycle.hip): the finest level's matrix, iterate
// and residual, ||b||^2 (normb2[0]), the residual SpMV's sum (sum[0]) and the solver's own grow-only device words
struct AmgLoop {
    psk_csr *A;
    double *x, *r, *normb2, *sum;
    DevBuf *work;
};
int amg_loop_view(const psk_prec *M, AmgLoop *out);
int amg_loop_start(const psk_prec *M, const Context *c, const double *v, hipStream_t s);   // ||v||^2, x = copy(v)
int amg_cycle(const psk_prec *M, const Context *c, const double *v, hipStream_t s);        // x = runCycle(v, x)
int amg_residual(const psk_prec *M, const double *v, hipStream_t s);                       // r = v - A x, ||r||^2

}  // namespace psk
