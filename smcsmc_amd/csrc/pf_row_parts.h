// smcsmc_amd/csrc/pf_row_parts.h -- the pieces of "extend the particles over one segment row" that more than one body is made of, one
// definition each.  The bodies keep their own row loop, order and control flow and call these for the straight-line parts:
//   register tree:  extend_reg_body (pf_hip.hip), extend_pair_body (pf_pair.h), extend_mpr_body (pf_mp.hip)              -- the row_* pieces
//   per-lane LDS tree: extend_lds_body (pf_lds_body.h, 32- and 64-bit masks), extend_lds_pipe_body (pf_lds_pipe.h), k_extend_mp (pf_mp.hip),
//                      extend_mp_pipe_body (pf_mp_pipe.h)                                                                 -- the lane_* pieces
//   either:         the delayed-factor store, the guide's stretch factor, the wavefront partials and where they are left
// Depends on PF_BS and the mask type of the including translation unit (pf_mask_t, pf_lane.h), like the headers it builds on.
#pragma once
#include "pf_device.h"
#include "pf_types.h"
#include "pf_lane.h"
#include "pf_tree_reg.h"
#include "pf_pipe.h"

// ---- register tree ----
// the alleles of a row as masks over the haplotypes
struct RowMasks { unsigned one = 0, zero = 0, present = 0, two = 0; int missing = 0; };
template <int NM, class F>
__device__ __forceinline__ RowMasks row_masks(int n, F&& allele) {
    RowMasks m;
#pragma unroll
    for (int i = 0; i < NM; ++i) if (i < n) {
        int d = allele(i);
        m.missing += d == -1;
        if (d == 1) m.one |= 1u << i;
        if (d == 0) m.zero |= 1u << i;
        if (d == 2) m.two |= 1u << i;
        if (d >= 0) m.present |= 1u << i;
    }
    return m;
}
// the likelihood of a row's site under the tree, averaged over the phasings of its unphased pairs
template <int NM>
__device__ __forceinline__ double row_site_lik(const RTree<NM>& t, int n, double v_mu, unsigned one_mask, unsigned zero_mask, unsigned two_mask, bool dephase, bool anc) {
    unsigned het_pairs = 0;
    int ncfg = 1;
    for (int i = 0; i + 1 < n; i += 2) {
        bool d0_two = (two_mask >> i) & 1u;
        bool one0 = (one_mask >> i) & 1u, one1 = (one_mask >> (i + 1)) & 1u;
        bool zero0 = (zero_mask >> i) & 1u, zero1 = (zero_mask >> (i + 1)) & 1u;
        bool het = d0_two || (dephase && ((one0 && zero1) || (zero0 && one1)));
        if (het) {
            ncfg *= 2;
            het_pairs |= 1u << i;
            one_mask &= ~(3u << i); zero_mask &= ~(3u << i);
            zero_mask |= 1u << i;
            one_mask |= 1u << (i + 1);
        }
    }
    double norm = 1.0 / (double)ncfg;
    RBranchP<NM> bprob;
    r_site_branch_probs(t, n, v_mu, bprob);     // once per row: the phasing configurations share them
    double lik = 0;
    for (;;) {
        lik += r_site_lik_from(t, n, bprob, one_mask, zero_mask, anc);
        if (ncfg == 1) break;
        bool more = false;
        for (int i = 0; i + 1 < n; i += 2) {
            if (!((het_pairs >> i) & 1)) continue;
            if ((zero_mask >> i) & 1) {
                zero_mask &= ~(1u << i); one_mask |= 1u << i;
                one_mask &= ~(1u << (i + 1)); zero_mask |= 1u << (i + 1);
                more = true;
                break;
            }
            one_mask &= ~(1u << i); zero_mask |= 1u << i;
            zero_mask &= ~(1u << (i + 1)); one_mask |= 1u << (i + 1);
        }
        if (!more) break;
    }
    lik *= norm;
    return lik;
}
// the five wavefront primitives behind the final weights of a row (the whole wavefront calls this), and where the row pipeline leaves them
struct RowScans { double sc, sp, sq, scp, scm; };
__device__ __forceinline__ RowScans row_scans(double w_post, double w_pilot, int lane) {
    RowScans r;
    r.sc = wave_hs_scan(w_pilot, lane);       // first: its running maximum below is the longest chain of the five
    r.sp = wave_tree_sum(w_post);
    r.sq = wave_tree_sum(w_pilot * w_pilot);
    r.scp = wave_hs_scan(w_post, lane);
    r.scm = wave_max_scan_d(r.sc, lane);     // running max of the pilot scan (a parallel FP scan need not be monotone)
    return r;
}
template <class KA>
__device__ __forceinline__ void row_scans_store(const KA& A2, int cur, long long p, bool active, int lane, const RowScans& r) {
    const long long chunk = p >> 6;
    const size_t ro = (size_t)cur * A2.Np, co = (size_t)cur * A2.nc;
    if (active) { A2.rg_scan1[ro + p] = r.sc; A2.rg_scanp[ro + p] = r.scp; A2.rg_scan1m[ro + p] = r.scm; }
    if (p == A2.Np - 1) A2.ctrl->last1[cur] = r.sc;
    if (lane == 63 && chunk < A2.nc) {
        A2.rg_cpost[co + chunk] = r.sp;
        A2.rg_csq[co + chunk] = r.sq;
        A2.rg_cpil[co + chunk] = r.sc;
        A2.rg_cpp[co + chunk] = r.scp;
        A2.rg_cmx1[co + chunk] = r.scm;
    }
}
// ... and where the general path leaves them (k_decide reads these), with the wavefront's count of particles that carry pending factors
template <class KA>
__device__ __forceinline__ void row_scans_store_general(const KA& A, long long p, bool active, int lane, const RowScans& r, bool biased, bool has_pending) {
    const long long chunk = p >> 6;
    if (active) { A.scan1[p] = r.sc; A.scanp2[A.sp][p] = r.scp; A.scan1m[p] = r.scm; }
    if (lane == 63 && chunk < (A.Np + 63) / 64) {
        A.chunk_post[chunk] = r.sp;
        A.chunk_sq[chunk] = r.sq;
        A.chunk_pil[chunk] = r.sc;
        A.chunk_pp[chunk] = r.scp;
        A.chunk_mx1[chunk] = r.scm;
    }
    if (biased) {
        unsigned long long pend = __ballot(has_pending);
        if (lane == 0 && chunk < (A.Np + 63) / 64) A.chunk_dpend[chunk] = __popcll(pend);
    }
}
// the stores of a row's end, but for the weights: the tree, ...
template <int NM>
__device__ __forceinline__ void row_store_tree(const DState& st1, size_t Np, long long p, int n, const RTree<NM>& t) {
#pragma unroll
    for (int r = 0; r < RTree<NM>::NI; ++r)
        if (r < n - 1) {
            st1.S[(size_t)r * Np + p] = t.S[r];
            st1.C[(size_t)(2 * r) * Np + p] = (int8_t)t.C0[r];
            st1.C[(size_t)(2 * r + 1) * Np + p] = (int8_t)t.C1[r];
        }
}
// ... what the chain carries from row to row, ...
template <class KA>
__device__ __forceinline__ void row_store_chain(const KA& A1, const DState& st1, long long p, double next_base, double x_mark, int mark_limit, const RCtx& cx) {
    st1.next_base[p] = next_base;
    st1.x_mark[p] = x_mark;
    st1.mark_limit[p] = mark_limit;
    st1.Ltree[p] = cx.Ltree;
    A1.rng_ctr[p] = cx.ctr;
    A1.ebuf[p] = cx.ebuf;
}
// ... and the counters of the row pipeline
template <class KA>
__device__ __forceinline__ void row_store_counters(const KA& A1, const PipeRow& PR, int cur, long long p, unsigned long long ctr, unsigned widx, bool do_extend) {
    if (PR.draws) A1.dt_ctr[(size_t)(PR.draws - 1) * A1.Np + p] = ctr;      // where the next row's draws start
    A1.rg_widx[(size_t)cur * A1.Np + p] = widx;
    if (!do_extend) A1.widx[p] = widx;              // the state goes back to the general kernels
    if (PR.ahead) {
        // running ahead of the counts: what they check of the ring (records appended as of the row they count) cannot see
        // this row's writes, so the writer checks them itself against the oldest generation any pending count can ask for
        const unsigned kold = A1.gstart[(size_t)(A1.ctrl->g_safe % A1.Gcap) * A1.Np + p];
        if (widx - kold > A1.cap && !A1.ctrl->err) A1.ctrl->err = ERR_LOG_OVERFLOW;
    }
}

// ---- either tree form: focused sampling and the guide ----
// importance_weight_over_segment (particle.cpp:1138-1181): true over guide rate for a stretch of length dist without recombination
__device__ __forceinline__ double row_guide_stretch(double dist, double rho, double guide_rho, double Ltree) {
    const double target_rate = dist * rho * Ltree;
    const double sampled_rate = dist * guide_rho * Ltree;
    return fastexp(sampled_rate - target_rate);
}
// particle.cpp:866-891: immediate vs delayed application of the importance weight of an update.  delay_height: the height that decides
// (the caller's: the structured bodies know a third choice); delay: the application delay of that height's epoch, looked up on the caller's tree form
__device__ __forceinline__ void row_delayed_factor(DStore& ds, const double* sBH, const double* sBS, int nbands, int delay_type, double delay_height, double iw, double rbiw,
                                                   double delay, double updated_to, double& w_post, double& w_pilot) {
    int idx = 0;
    while (idx + 1 < nbands + 1 && sBH[idx + 1] < delay_height) ++idx;
    if (idx >= nbands) idx = nbands - 1;
    if (sBS[idx] == 1.0 && !(delay_type & 4)) { w_post *= rbiw; w_pilot *= rbiw; iw /= rbiw; }   // bit 2: every factor delayed (pf_model.delay_type)
    d_adjust_with_delay(ds, w_post, w_pilot, iw, delay, updated_to);
}
// apply the factors that fell due during this extension (particle.cpp:910-916; none on a completion-only step) and leave the store's
// count and total, and the guide's segment index, with the state.  Returns whether factors are still pending.
__device__ __forceinline__ bool row_apply_due(DStore& ds, const DState& st, long long p, double extend_to, bool do_extend, bool guided, int ridx, double& w_pilot) {
    for (;;) {
        if (ds.count == 0 || !do_extend) break;
        double pm = ds.pos[0];
        for (int i = 1; i < ds.count; ++i) { double pi = ds.pos[(size_t)i * ds.Np]; if (pi < pm) pm = pi; }
        if (!(pm < extend_to)) break;
        d_apply_earliest(ds, w_pilot);
    }
    st.dcount[p] = ds.count;
    st.total_delayed[p] = ds.total;
    if (guided) st.ridx[p] = ridx;
    return ds.count > 0;
}
// the copy constructor copies the pending factors (particle.cpp:122-123): those of src[a] into dst[p]
__device__ __forceinline__ void row_copy_pending(const DState& dst, const DState& src, size_t Np, long long p, long long a, int count) {
    for (int k = 0; k < count; ++k) {
        dst.dpos[(size_t)k * Np + p] = src.dpos[(size_t)k * Np + a];
        dst.dfac[(size_t)k * Np + p] = src.dfac[(size_t)k * Np + a];
        dst.ddelta[(size_t)k * Np + p] = src.ddelta[(size_t)k * Np + a];
        dst.dk[(size_t)k * Np + p] = src.dk[(size_t)k * Np + a];
    }
}

// ---- per-lane LDS tree ----
// the tree of from[a] into this lane's columns, ...
__device__ __forceinline__ void lane_load_tree(Lane& ln, const DState& from, size_t Np, long long a, int n) {
    for (int r = 0; r < n - 1; ++r) {
        LS(ln, r) = from.S[(size_t)r * Np + a];
        LC(ln, r, 0) = from.C[(size_t)(2 * r) * Np + a];
        LC(ln, r, 1) = from.C[(size_t)(2 * r + 1) * Np + a];
    }
}
// ... and the columns into st[p]
__device__ __forceinline__ void lane_store_tree(const Lane& ln, const DState& st, size_t Np, long long p, int n) {
    for (int r = 0; r < n - 1; ++r) {
        st.S[(size_t)r * Np + p] = LS(ln, r);
        st.C[(size_t)(2 * r) * Np + p] = LC(ln, r, 0);
        st.C[(size_t)(2 * r + 1) * Np + p] = LC(ln, r, 1);
    }
}
// what the chain carries from row to row (row_store_chain for a Lane)
template <class KA>
__device__ __forceinline__ void lane_store_chain(const KA& A, const DState& st, long long p, double next_base, double x_mark, int mark_limit, const Lane& ln) {
    st.next_base[p] = next_base;
    st.x_mark[p] = x_mark;
    st.mark_limit[p] = mark_limit;
    st.Ltree[p] = ln.Ltree;
    A.rng_ctr[p] = ln.ctr;
    A.ebuf[p] = ln.ebuf;
}
// the row's alleles: 1 = no haplotype missing (the tracked length is the tree's), -1 = all missing, 0 = some (a completion-only step has no row: 1)
__device__ __forceinline__ int lane_leaf_status(const int8_t* data, int n, bool do_extend) {
    int missing = 0;
    for (int i = 0; i < n && do_extend; ++i) missing += data[i] == -1;
    int leaf_status = 0;
    if (missing == 0) leaf_status = 1;
    if (missing == n) leaf_status = -1;
    return leaf_status;
}
// update_weight_at_site: the likelihood of a row's site under the lane's tree, averaged over the phasings of its unphased pairs (pc.cpp:138-224)
__device__ __forceinline__ double lane_site_weight(const Lane& ln, const int8_t* data, int n, bool dephase, bool anc, double* tmp0, double* tmp1) {
    pf_mask_t one_mask = 0, zero_mask = 0, het_pairs = 0;
    int ncfg = 1;
    for (int i = 0; i < n; ++i) {
        if (data[i] == 1) one_mask |= (pf_mask_t)1 << i;
        if (data[i] == 0) zero_mask |= (pf_mask_t)1 << i;
    }
    for (int i = 0; i + 1 < n; i += 2) {
        bool het = (data[i] == 2) || (dephase && data[i] + data[i + 1] == 1);
        if (het) {
            ncfg *= 2;
            het_pairs |= (pf_mask_t)1 << i;
            one_mask &= ~((pf_mask_t)3 << i); zero_mask &= ~((pf_mask_t)3 << i);
            zero_mask |= (pf_mask_t)1 << i;          // hap[i] = 0
            one_mask |= (pf_mask_t)1 << (i + 1);     // hap[i+1] = 1
        }
    }
    double norm = 1.0 / (double)ncfg;
    double lik = 0;
    for (;;) {
        lik += site_lik_lane(ln, one_mask, zero_mask, anc, tmp0, tmp1);
        if (ncfg == 1) break;
        bool more = false;                  // next_haplotype (pc.cpp:163-181)
        for (int i = 0; i + 1 < n; i += 2) {
            if (!((het_pairs >> i) & 1)) continue;
            if ((zero_mask >> i) & 1) {     // phase 0 -> phase 1
                zero_mask &= ~((pf_mask_t)1 << i); one_mask |= (pf_mask_t)1 << i;
                one_mask &= ~((pf_mask_t)1 << (i + 1)); zero_mask |= (pf_mask_t)1 << (i + 1);
                more = true;
                break;
            }
            one_mask &= ~((pf_mask_t)1 << i); zero_mask |= (pf_mask_t)1 << i;
            zero_mask &= ~((pf_mask_t)1 << (i + 1)); one_mask |= (pf_mask_t)1 << (i + 1);
        }
        if (!more) break;
    }
    lik *= norm;
    return lik;
}
