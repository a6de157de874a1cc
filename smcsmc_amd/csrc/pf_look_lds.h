// smcsmc_amd/csrc/pf_look_lds.h -- the look-ahead factor of the auxiliary particle filter on the per-lane LDS tree, inside a row kernel.
//
// ForestState::includeLookaheadLikelihood (particle.cpp:439-617) for one particle, of one population or of a structured model: k_lookahead's
// arithmetic (pf_hip.hip), statement for statement and in the same operation order, and therefore its bits.  Only the storage differs.
// k_lookahead keeps three scratch columns a lane beside the tree -- n parent heights, n mutation probabilities, n parent ranks,
// PF_BS * (2n * 8 + n * 4) bytes -- which the extend roles of the row pipeline have no room for (100 KB of tree columns at 16 haplotypes and
// 256 lanes).  Here
//   the parent height of leaf i is not stored: it is LS(pr) for a parent rank pr >= 0 and the time of migration event -2 - pr otherwise;
//   the mutation probabilities (n doubles) and the parent ranks (n ints) lie in the lane's columns t0 and t1 (Smem, pf_lane.h: adjacent,
//   n - 1 doubles each, 2 (n - 1) columns a lane against the n + ceil(n / 2) needed, enough from n = 4 on; the ranks two to a double, so that
//   every byte a lane touches is in its own column slots).  t0 and t1 are scratch of tracked_len_lane,
//   genealogy_update and site_lik_lane: dead when the row's site likelihood is done, and taken again only by the split term's site_lik_lane,
//   which comes last, behind the last read of either array.
// With several populations the first node above a leaf may be a migration event on its branch (k_lookahead's A.P > 1 branch, which reads
// st.Mb / st.Mt from memory): the caller hands in the lane's event list as a small functor (count / branch / time, sorted by time as the
// state keeps it; LookMigL in pf_mp_pipe.h reads the LDS columns).  Without one (LookNoMigL, the default) that code is not there.
// Used by extend_lds_pipe_body<..., LOOK> (pf_lds_pipe.h, one population) and extend_mp_pipe_body<..., LOOK> (pf_mp_pipe.h), nothing else.
// A fix to k_lookahead belongs here and in look_factor (pf_look_reg.h) as well; tests/test_gpu_lookahead_rows_lds.py holds this copy to
// k_lookahead's bits.
#pragma once
#include "pf_lane.h"

// no migration events: one population
struct LookNoMigL { static constexpr bool on = false; };

// The parent ranks are ints in columns that the site likelihood reads and writes as doubles, before and after: an int that may alias
// anything, or type-based alias analysis leaves the compiler free to move the rank stores above the last loads of the row's own site likelihood
typedef int __attribute__((may_alias)) look_rank_t;

// the factor of row `row` for the lane's tree (as the extend of that row left it), Ltree its length, mig the migration events on it;
// t0 / t1: the lane's pointers into the scratch columns (m.t0 + threadIdx.x, m.t1 + threadIdx.x)
template <class KA, class MG = LookNoMigL>
__device__ __forceinline__ double look_factor_lds(const KA& A, Lane& ln, long long row, double Ltree, double* t0, double* t1, MG mig = MG()) {
    const int n = A.n, Q = A.la_Q, D = A.la_D;
    double* s_mp = t0;                                                                        // [n] stride PF_BS
    // [n] behind s_mp, two ranks to a double of the lane's own column: rank i in half i & 1 of column n + i / 2.  (Ints at stride PF_BS would
    // put the ranks of two lanes into one double of the columns -- the slot of a lane of another wavefront, which at 256 lanes a workgroup
    // may still be in its site likelihood.)
    auto s_par = [&](int i) -> look_rank_t& { return ((look_rank_t*)(t0 + (size_t)(n + (i >> 1)) * PF_BS))[i & 1]; };
    auto s_lh = [&](int i) -> double {                                                        // what k_lookahead stores beside the rank
        const int pr = s_par(i);
        if constexpr (MG::on) { if (pr < 0) return mig.time(-2 - pr); }
        return LS(ln, pr);
    };
    const double* fsd = A.la_fsd + (size_t)row * n;
    const double* rmr = A.la_rmr + (size_t)row * n;
    const int8_t* unph = A.la_unph + (size_t)row * n;
    const double recomb_rate = A.rho, mut_rate = A.mu;
    double likelihood = 1.0;
    const double rho_tbl = 2 * recomb_rate * (n - 1) / n;
    for (int i = 0; i < n; ++i) {
        int pr = -1;
        for (int r = 0; r < n - 1 && pr < 0; ++r)
            if (LC(ln, r, 0) == i || LC(ln, r, 1) == i) pr = r;
        if constexpr (MG::on) {
            // structured models: the first local node above a leaf may be a migration on its branch (the events
            // of a particle are sorted by time, so the first hit is the lowest)
            const int nmig = mig.count();
            for (int mi = 0; mi < nmig; ++mi)
                if (mig.branch(mi) == i) { pr = -2 - mi; break; }
        }
        s_par(i) = pr;
        s_mp[i * PF_BS] = 0.0;
    }
    for (int i = 0; i < n; i++) {
        double pp = 0;
        const double si = fsd[i];
        double li = s_lh(i);
        const bool up = unph[i] != 0;
        if (up) li += s_lh(i + 1);
        const double rel_mut_rate = rmr[i];
        const double li_mu = li * mut_rate * rel_mut_rate;
        s_mp[i * PF_BS] = li_mu;
        if (up) s_mp[(i + 1) * PF_BS] = li_mu;
        for (int r = 0; r < 2; r++) {
            const double rel = r == 0 ? 1.0 : 0.5;
            const double li_rho = li * rho_tbl * rel;
            const double fe = fastexp_approx(-(li_rho + li_mu) * fabs(si));
            for (int q = 0; q < Q; ++q) {
                double qbot = (q == 0 ? 0.0 : A.la_q[q - 1]);
                double qtop = (q == Q - 1 ? 1.0 : A.la_q[q]);
                double l_prime = A.la_tbl[i * Q + q];
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
    if (A.apf >= 2) {
        double l_mean = 0.0;
        for (int i = 0; i < n; i++) l_mean += A.la_tbl[i * Q + (Q - 1)] / n;
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
                    if (s_par(a) == s_par(b)) {
                        double l = s_lh(a);
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
                double mutprob = (s_mp[di[0] * PF_BS] + s_mp[di[1] * PF_BS]) * 0.5;
                double pp = 0;
                for (int r = 0; r < 2; r++)
                    pp += 0.5 * (mutprob + (1.0 - mutprob) * p_equilibrium *
                                 (1.0 - fastexp_approx(-rhoprime_c * (r == 0 ? 1.0 : 0.5) * l_mean * fed)));
                likelihood *= pp;
            }
        }
    }
    if (A.la_split[row] > -1 && A.apf >= 3) {
        double rate_of_change = Ltree * recomb_rate / 2;
        double p_nochange = fastexp_approx(-rate_of_change * A.la_split[row]);
        unsigned one_mask = 0, zero_mask = 0;
        for (int i = 0; i < n; ++i) {
            int v = A.la_salleles[(size_t)row * n + i];
            if (v == 1) one_mask |= 1u << i;
            if (v == 0) zero_mask |= 1u << i;
        }
        // (s_mp and s_par are dead from here on: site_lik_lane takes t0 and t1)
        double p_splitdata = site_lik_lane(ln, one_mask, zero_mask, false, t0, t1);
        int k = A.la_sk[row];
        double p_correct_split = k / double(4.0 * n * n);
        if (A.apf == 4) {
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
