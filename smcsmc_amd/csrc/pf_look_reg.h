// smcsmc_amd/csrc/pf_look_reg.h -- the look-ahead factor of the auxiliary particle filter on the register tree.
//
// ForestState::includeLookaheadLikelihood (particle.cpp:439-617) for one particle, of one population or of a structured model: k_lookahead's
// arithmetic (pf_hip.hip), statement for statement and in the same operation order, and therefore its bits.  Only the
// storage differs: the tree is RTree<NM>, and the per-lane scratch of k_lookahead -- n parent heights, n mutation
// probabilities, n parent ranks, LDS columns there -- is three register arrays here.  Their run-time indices (the
// haplotypes of a row's singletons and doubletons) are the same for every lane, and are taken with the bit-mask
// selects of RTree (a `?:` chain is folded back into an indexed load, and the arrays into scratch memory).  The
// split term goes through the register form of the site likelihood (r_site_branch_probs / r_site_lik_from), which
// tests/test_gpu_parity.py holds equal to site_lik_lane.
// With several populations the first node above a leaf may be a migration event on its branch (k_lookahead's A.P > 1 branch): the
// caller hands in its event list as a small functor (count / branch / time, sorted by time as the state keeps it), and the leaf's
// height and parent id come from the lowest event on the branch.  Without one (LookNoMig, the default) that code is not there.
// Used by extend_reg_body<..., LOOK> (pf_hip.hip, one population) and extend_mpr_body<..., LOOK> (pf_mp.hip, LookMigR), nothing else.
#pragma once
#include "pf_tree_reg.h"

namespace pf {

template <int N>
__device__ __forceinline__ double la_get(const double (&v)[N], int i) {
    long long bits = __double_as_longlong(v[0]);
#pragma unroll
    for (int k = 1; k < N; ++k) {
        const long long m = -(long long)(i == k);
        bits = (bits & ~m) | (__double_as_longlong(v[k]) & m);
    }
    return __longlong_as_double(bits);
}
template <int N>
__device__ __forceinline__ void la_set(double (&v)[N], int i, double x) {
    const long long xb = __double_as_longlong(x);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const long long m = -(long long)(i == k);
        v[k] = __longlong_as_double((__double_as_longlong(v[k]) & ~m) | (xb & m));
    }
}
template <int N>
__device__ __forceinline__ int la_geti(const int (&v)[N], int i) {
    int r = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) r |= v[k] & -(int)(i == k);
    return r;
}

// no migration events: one population
struct LookNoMig { static constexpr bool on = false; };

// the factor of row `row` for the tree t (as the extend of that row left it), Ltree its length, mig the migration events on it
template <int NM, class KA, class MG = LookNoMig>
__device__ __forceinline__ double look_factor(const KA& A, const RTree<NM>& t, int n, long long row, double Ltree, MG mig = MG()) {
    constexpr int NI = RTree<NM>::NI;
    const int Q = A.la_Q, D = A.la_D, apf = A.apf;
    const double* fsd = A.la_fsd + (size_t)row * n;
    const double* rmr = A.la_rmr + (size_t)row * n;
    const int8_t* unph = A.la_unph + (size_t)row * n;
    const double* la_q = A.la_q;
    const double* la_tbl = A.la_tbl;
    const double recomb_rate = A.rho, mut_rate = A.mu;
    double likelihood = 1.0;
    const double rho_tbl = 2 * recomb_rate * (n - 1) / n;
    // every leaf's parent rank (the lowest node it hangs from) and that node's height
    double s_lh[NM], s_mp[NM];
    int s_par[NM];
#pragma unroll
    for (int i = 0; i < NM; ++i) {
        int pr = -1;
        double hgt = 0.0;
#pragma unroll
        for (int r = 0; r < NI; ++r)
            if (r < n - 1) {
                const bool hit = pr < 0 && (t.C0[r] == i || t.C1[r] == i);
                hgt = hit ? t.S[r] : hgt;
                pr = hit ? r : pr;
            }
        s_par[i] = pr;
        s_lh[i] = hgt;
        s_mp[i] = 0.0;
    }
    if constexpr (MG::on) {
        // structured models: the first local node above a leaf may be a migration on its branch; its id is -2 - mi, which pairs it with
        // no other leaf in the doubleton test.  One pass over the events, in time order: the first hit of a leaf is its lowest
        const int nmig = mig.count();
        for (int mi = 0; mi < nmig; ++mi) {
            const int b = mig.branch(mi);
            const double tm = mig.time(mi);
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                const bool hit = i < n && b == i && s_par[i] >= 0;
                s_lh[i] = hit ? tm : s_lh[i];
                s_par[i] = hit ? -2 - mi : s_par[i];
            }
        }
    }
    for (int i = 0; i < n; i++) {
        double pp = 0;
        const double si = fsd[i];
        double li = la_get(s_lh, i);
        const bool up = unph[i] != 0;
        if (up) li += la_get(s_lh, i + 1);
        const double rel_mut_rate = rmr[i];
        const double li_mu = li * mut_rate * rel_mut_rate;
        la_set(s_mp, i, li_mu);
        if (up) la_set(s_mp, i + 1, li_mu);
        for (int r = 0; r < 2; r++) {
            const double rel = r == 0 ? 1.0 : 0.5;
            const double li_rho = li * rho_tbl * rel;
            const double fe = fastexp_approx(-(li_rho + li_mu) * fabs(si));
            for (int q = 0; q < Q; ++q) {
                double qbot = (q == 0 ? 0.0 : la_q[q - 1]);
                double qtop = (q == Q - 1 ? 1.0 : la_q[q]);
                double l_prime = la_tbl[i * Q + q];
                double lprime_mu = l_prime * mut_rate * rel_mut_rate;
                double div = (li_rho + li_mu - lprime_mu);
                if (fabs(div) < (li_rho + li_mu + lprime_mu) * 1e-5) lprime_mu = lprime_mu * 1.0001;
                if (si > 0) {
                    pp += 0.5 * (qtop - qbot) * ((li_rho * lprime_mu * fastexp_approx(-lprime_mu * si) +
                                                  (li_mu - lprime_mu) * (li_rho + li_mu) * fe)
                                                 / (li_rho + li_mu - lprime_mu));
                } else {
                    pp += 0.5 * (qtop - qbot) * ((li_rho * fastexp_approx(-lprime_mu * (-si)) +
                                                  (li_mu - lprime_mu) * fe)
                                                 / (li_rho + li_mu - lprime_mu));
                }
            }
        }
        likelihood *= pp;
        if (up) i++;
    }
    if (apf >= 2) {
        double l_mean = 0.0;
        for (int i = 0; i < n; i++) l_mean += la_tbl[i * Q + (Q - 1)] / n;
        const double rho_c = 4 * recomb_rate * (n - 2) / n;
        const double rhoprime_c = recomb_rate * (n - 1);
        const double p_equilibrium = 2.0 / (3 * (n - 1));
        const int nd = A.la_nd[row];
        for (int k = 0; k < nd; ++k) {
            const int8_t* di = A.la_didx + ((size_t)row * D + k) * 4;
            const double fed = A.la_ddist[((size_t)row * D + k) * 2], led = A.la_ddist[((size_t)row * D + k) * 2 + 1];
            int ph1, ph2;
            for (ph1 = 0; ph1 <= di[2]; ph1++) {
                for (ph2 = 0; ph2 <= di[3]; ph2++) {
                    int a = di[0] + ph1, b = di[1] + ph2;
                    if (la_geti(s_par, a) == la_geti(s_par, b)) {
                        double l = la_get(s_lh, a);
                        double pp = 0;
                        for (int r = 0; r < 2; r++) {
                            double exp_rho = fastexp_approx(-rho_c * (r == 0 ? 1.0 : 0.5) * l * led);
                            pp += 0.5 * exp_rho + p_equilibrium * (1.0 - exp_rho);
                        }
                        likelihood *= pp;
                        ph1 = ph2 = 99;
                    }
                }
            }
            if (ph1 < 99) {
                double mutprob = (la_get(s_mp, di[0]) + la_get(s_mp, di[1])) * 0.5;
                double pp = 0;
                for (int r = 0; r < 2; r++)
                    pp += 0.5 * (mutprob + (1.0 - mutprob) * p_equilibrium *
                                 (1.0 - fastexp_approx(-rhoprime_c * (r == 0 ? 1.0 : 0.5) * l_mean * fed)));
                likelihood *= pp;
            }
        }
    }
    const double split = A.la_split[row];
    if (split > -1 && apf >= 3) {
        double rate_of_change = Ltree * recomb_rate / 2;
        double p_nochange = fastexp_approx(-rate_of_change * split);
        unsigned one_mask = 0, zero_mask = 0;
        for (int i = 0; i < n; ++i) {
            int v = A.la_salleles[(size_t)row * n + i];
            if (v == 1) one_mask |= 1u << i;
            if (v == 0) zero_mask |= 1u << i;
        }
        RBranchP<NM> bprob;
        r_site_branch_probs(t, n, mut_rate, bprob);
        double p_splitdata = r_site_lik_from(t, n, bprob, one_mask, zero_mask, false);
        int k = A.la_sk[row];
        double p_correct_split = k / double(4.0 * n * n);
        if (apf == 4) {
            double nCk = 1.0;
            for (int i = 1; i <= k; i++) nCk *= (n - i + 1) / double(i);
            p_correct_split = 1.0 / nCk;
        }
        double split_branch_length = k * A.la_mean_tbl / (2 * n * (0.577 * dlog((double)n)));
        double pp = p_nochange * p_splitdata + (1.0 - p_nochange) * p_correct_split * mut_rate * split_branch_length;
        likelihood *= pp;
    }
    return likelihood;
}

}  // namespace pf
