// smcsmc_amd/csrc/pf_lds_body.h -- bodies of the one-population LDS-tree kernels: the prior (k_init), the extension over a
// segment (k_extend), lag calibration (k_calibrate) and the device simulator (k_simulate).  Compiled twice: by pf_hip.hip with
// 256-lane workgroups and 32-bit masks (nsam <= PF_NMAX), and by pf_wide.hip with one wavefront per workgroup and 64-bit masks
// (nsam <= PF_NMAX_WIDE, PF_WIDE).  Each translation unit wraps the bodies in kernels of its own names; `smem` is the
// kernel's dynamic LDS.
#pragma once
#include "pf_device.h"
#include "pf_types.h"
#include "pf_lane.h"
#include "pf_tree_reg.h"
#include "pf_row_parts.h"

// ------------------------------------------------------------------ k_init  (particleContainer.cpp:33-65)
__device__ __forceinline__ void init_lds_body(const KArgs& A, double initial_position, double* smem) {
    Smem m = carve(smem, A.n, A.E);
    load_model(A, m);
    __syncthreads();
    long long p = (long long)blockIdx.x * PF_BS + threadIdx.x;
    if (p == 0) {
        Ctrl* c = A.ctrl;
        c->cur_pos = initial_position;
        c->logl = 0; c->inv_T = 1; c->T = 1; c->flag = 0; c->cur = 0; c->gen = 0; c->n_resample = 0; c->lver = 0;
        c->first_epoch = A.E; c->err = 0; c->delayed_opp = 0; c->delayed_count = 0; c->count_active = 0; c->end_seq = 0;
        c->g_retain = 0; c->g_safe = 0; c->delay_peak = 0; c->n_delay_evict = 0; c->pending_fin = 0;
        for (int k = 0; k < PF_RING; ++k) c->ri[k].g_retain = 0;      // (what Ctrl::g_safe is read from in the first rows of a sweep)
        c->nbx_used = A.nbx; c->gen_prev = 0; c->nres_prev = 0;      // k_decide of the first row reads these (a re-initialised handle too)
        for (int e = 0; e < A.E; ++e) { c->counted_to[e] = 0; c->update_to[e] = 0; c->g_lo[e] = 0; c->g_hi[e] = 0; }
        A.gen_x0[0] = 0.0;
    }
    if (p >= A.Np) return;
    const int n = A.n;
    Lane ln = make_lane(A, m, p);
    ln.ebuf = -dlog(uni(ln));
    unsigned widx = 0;
    int root = 0;
    double w0 = 1.0 / (double)A.Np;
    // Forest::buildInitialTree(true): add the samples one by one; every coalescence is logged
    // as a type-2 record at position 0 (record_all_event, particle.cpp:251-300)
    for (int i = 1; i < n; ++i) {
        int ni = i - 1;
        double* rec = rec_ptr(A, p, widx);
        rec[0] = 0.0; rec[1] = 0.0; rec[2] = 0.0;
        for (int r = 0; r < n - 1; ++r) rec[5 + r] = r < ni ? LS(ln, r) : 0.0;
        double tc = coalesce_up(ln, [&](int k) { return LS(ln, k); }, ni, i, 0.0);
        if (ln.vbc) { w0 *= ln.upd_fac; ln.upd_fac = 1.0; }
        rec[3] = tc;
        ++widx;
        int pr = -1, ps = 0;
        int k = lineages_at(ln, ni, tc, -1, &pr, &ps);
        bool above_root = (ni == 0) || (tc >= LS(ln, ni - 1));
        int kk = above_root ? 1 : k;
        double u = uni(ln);
        int idx = min((int)(u * (double)kk), kk - 1);
        pf_mask_t dn = ((pf_mask_t)2 << i) - 1u;      // above the root: all samples added so far
        if (above_root) {
            insert_node(ln, ni, tc, i, -1, 0, root);
        } else {
            lineages_at(ln, ni, tc, idx, &pr, &ps);
            if (A.rec_trees) dn = ((pf_mask_t)1 << i) | lane_desc_mask(ln, LC(ln, pr, ps), m.t0 + threadIdx.x);
            insert_node(ln, ni, tc, i, pr, ps, root);
        }
        rec[4] = __longlong_as_double((long long)make_meta(2, A.E - 1, A.E - 1, i, 0, A.rec_trees ? (unsigned)dn : 0u));
        root = n + ni;
    }
    ln.Ltree = tree_length(ln, n);
    if (A.g_K > 0) {
        // with a guide the first draw uses the rate of the first segment and stops at its end
        ln.rho = A.g_rho[0];
        if (A.g_K > 1 && A.g_pos[1] < A.L) ln.L = A.g_pos[1];
    }
    double nb = sample_next_base(ln, 0.0);
    const DState st = A.st0;
    for (int r = 0; r < n - 1; ++r) {
        st.S[(size_t)r * A.Np + p] = LS(ln, r);
        st.C[(size_t)(2 * r) * A.Np + p] = LC(ln, r, 0);
        st.C[(size_t)(2 * r + 1) * A.Np + p] = LC(ln, r, 1);
    }
    st.w_post[p] = w0;
    st.w_pilot[p] = w0;
    st.next_base[p] = nb;
    st.x_mark[p] = 0.0;
    st.Ltree[p] = ln.Ltree;
    st.mark_limit[p] = A.E - 1;
    if (A.n_bias > 0 || A.g_K > 0) { st.total_delayed[p] = 1.0; st.dcount[p] = 0; }
    if (A.g_K > 0) st.ridx[p] = 0;
    if (st.lookahead) st.lookahead[p] = 1.0;
    A.rng_ctr[p] = ln.ctr;
    A.ebuf[p] = ln.ebuf;
    A.widx[p] = widx;
    A.gstart[p] = 0;   // generation 0 starts with an empty log (the init records belong to it)
}

// ------------------------------------------------------------------ k_extend
// ParticleContainer::extend_ARGs + update_weight_at_site (particleContainer.cpp:98-135, 187-224)
// with ForestState::extend_ARG (particle.cpp:743-918) per lane.
// (extend_lds_pipe_body, pf_lds_pipe.h, repeats the skeleton of this body's row loop for the row pipeline -- k_sweep_xl: a change to the
// loop here is a change there as well, and tests/test_gpu_sweep_lds.py compares the two bit for bit.  What the loop is made of -- the
// guide's factor, the delayed-factor store, the site likelihood, the stores and the partials -- has one definition, pf_row_parts.h)
__device__ __forceinline__ void extend_lds_body(const KArgs& A, long long s, double* smem) {
    Smem m = carve(smem, A.n, A.E);
    load_model(A, m);
    __shared__ double sBH[PF_BIAS_MAX + 2], sBS[PF_BIAS_MAX + 1];      // focused sampling: band boundaries / strengths
    if (threadIdx.x < PF_BIAS_MAX + 2) {
        sBH[threadIdx.x] = A.bias_H[threadIdx.x];
        if (threadIdx.x < PF_BIAS_MAX + 1) sBS[threadIdx.x] = A.bias_S[threadIdx.x];
    }
    __syncthreads();
    const bool guided = A.g_K > 0;
    const bool biased = A.n_bias > 0 || guided;          // a guide alone runs with one band of strength 1
    bool has_pending = false;
    const Ctrl* c = A.ctrl;
    const int n = A.n;
    const int cur = __builtin_amdgcn_readfirstlane(c->cur);
    const long long p = (long long)blockIdx.x * PF_BS + threadIdx.x;
    const bool active = p < A.Np;
    const int lane = threadIdx.x & 63;
    double w_post = 0.0, w_pilot = 0.0;
    if (active) {
        const DState st = state_slot(A, cur);
        Lane ln = make_lane(A, m, p);
        lane_load_tree(ln, st, (size_t)A.Np, p, n);
        w_post = st.w_post[p];
        w_pilot = st.w_pilot[p];
        double next_base = st.next_base[p];
        double x_mark = st.x_mark[p];
        int mark_limit = st.mark_limit[p];
        ln.Ltree = st.Ltree[p];
        ln.ctr = A.rng_ctr[p];
        ln.ebuf = A.ebuf[p];
        unsigned widx = A.widx[p];
        DStore ds;
        d_bind(ds, A, st, p);
        ds.count = 0; ds.total = 1.0;
        if (biased) { ds.count = st.dcount[p]; ds.total = st.total_delayed[p]; }
        int ridx = guided ? st.ridx[p] : 0;
        double* tmp0 = m.t0 + threadIdx.x;
        double* tmp1 = m.t1 + threadIdx.x;

        const int8_t* data = A.seg_alleles + (size_t)s * n;
        const double seg_end = A.seg_start[s] + A.seg_len[s];
        const double extend_to = seg_end < A.L ? seg_end : A.L;
        const int limit = A.seg_limit[s];
        const int leaf_status = lane_leaf_status(data, n, true);

        double updated_to = c->cur_pos;
        double B;
        if (leaf_status == -1) B = 0;
        else if (leaf_status == 1) B = ln.Ltree;
        else B = tracked_len_lane(ln, data, tmp0);

        while (updated_to < extend_to) {
            double new_to = extend_to < next_base ? extend_to : next_base;
            double f = fastexp(-A.mu * B * (new_to - updated_to));
            w_post *= f;
            w_pilot *= f;
            if (guided) {
                const double iws = row_guide_stretch(new_to - updated_to, A.rho, A.g_rho[ridx], ln.Ltree);
                w_post *= iws;
                w_pilot *= iws;
            }
            updated_to = new_to;
            if (guided && updated_to < extend_to && ridx + 1 < A.g_K && updated_to == A.g_pos[ridx + 1]) {
                // reached a change of the guide rate: no genealogy change, new draw under the new rate
                ridx += 1;
                next_base = sample_next_base_guided(ln, updated_to, A.g_K, A.g_pos, A.g_rho, ridx);
                continue;
            }
            if (updated_to < extend_to) {
                // a recombination: log the stretch that ends here together with the event
                double* rec = rec_ptr(A, p, widx);
                rec[0] = x_mark;
                rec[1] = updated_to;
                for (int r = 0; r < n - 1; ++r) rec[5 + r] = LS(ln, r);
                double h, tc, sp_removed;
                bool changed;
                pf_mask_t desc = 0, desc_new = 0;
                double iw = 1.0, rbiw = 1.0;
                genealogy_update(ln, &h, &tc, &sp_removed, &changed, (A.lmap_opp || A.rec_trees) ? &desc : nullptr, tmp0,
                                 biased ? sBH : nullptr, sBS, A.n_bias + 1, &iw,
                                 guided ? A.g_leaf + (size_t)ridx * n : nullptr, guided ? A.rho / A.g_rho[ridx] : 1.0, &rbiw,
                                 A.rec_trees ? &desc_new : nullptr);
                if (ln.vbc) { w_post *= ln.upd_fac; w_pilot *= ln.upd_fac; ln.upd_fac = 1.0; }
                rec[2] = h;
                rec[3] = tc;
#if PF_WIDE
                // more than 16 samples: the cut branch's samples in a word of their own behind the heights (KArgs::RS = n + 5)
                rec[4] = __longlong_as_double((long long)make_meta(0, mark_limit, limit, n));
                rec[4 + n] = __longlong_as_double((long long)desc);
#else
                rec[4] = __longlong_as_double((long long)make_meta(0, mark_limit, limit, n, desc, desc_new));
#endif
                ++widx;
                if (leaf_status == 0) B = tracked_len_lane(ln, data, tmp0);
                if (leaf_status == 1) B = ln.Ltree;
                if (biased) {
                    const double delay_height = (A.delay_type & 3) == 0 ? h : tc;
                    row_delayed_factor(ds, sBH, sBS, A.n_bias + 1, A.delay_type, delay_height, iw, rbiw, A.app_delays[epoch_of(ln, delay_height)], updated_to, w_post, w_pilot);
                }
                next_base = sample_next_base_guided(ln, updated_to, A.g_K, A.g_pos, A.g_rho, ridx);
                ln.uqn = 0;                    // the update's unused uniforms are dropped
                x_mark = updated_to;
                mark_limit = limit;
            }
        }

        if (biased) has_pending = row_apply_due(ds, st, p, extend_to, true, guided, ridx, w_pilot);
        if (A.seg_state[s] == 0) {
            const double lik = lane_site_weight(ln, data, n, A.flags & 2, A.flags & 1, tmp0, tmp1);
            w_post *= lik;
            w_pilot *= lik;
        }

        lane_store_tree(ln, st, (size_t)A.Np, p, n);
        st.w_post[p] = w_post;
        st.w_pilot[p] = w_pilot;
        lane_store_chain(A, st, p, next_base, x_mark, mark_limit, ln);
        A.widx[p] = widx;
        if (A.rec_trees && widx >= A.cap) A.ctrl->err = ERR_LOG_OVERFLOW;
        for (int r = 0; r < n - 1; ++r) A.snap_S[A.sp][(size_t)r * A.Np + p] = LS(ln, r);
        A.snap_w[A.sp][p] = w_post; A.snap_xm[A.sp][p] = x_mark; A.snap_ml[A.sp][p] = mark_limit; A.snap_widx[A.sp][p] = widx;
    }
    // per-wavefront canonical partials (level 1 of the radix-64 reduction / scan)
    row_scans_store_general(A, p, active, lane, row_scans(w_post, w_pilot, lane), biased, has_pending);
}

// ------------------------------------------------------------------ k_calibrate
// calculate_median_survival_distances (smcsmc.cpp:169-263): one prior ARG per lane; evolve it along
// the sequence without data until every internal node of the initial tree has been removed (or
// 0.6 L is reached) and report, per original node, its epoch and the position where it disappeared.
// NM = 0: the recombination loop runs on the LDS tree (any nsam); NM = 4 / 8: on the register tree of the extend
// kernels (nsam <= NM), same arithmetic operation for operation, about half the instructions.  The epoch tables of
// the register path sit behind the LDS-tree block.
template <int NM>
__device__ __forceinline__ void calibrate_lds_body(const KArgs& A, unsigned long long seed, long long rep0, long long nrep,
                                                   int* out_epoch, double* out_dist, double* smem) {
    Smem m = carve(smem, A.n, A.E);
    load_model(A, m);
    double* sT = (double*)((char*)smem + smem_bytes(A.n, A.E));
    double* sH = sT + PF_EPAD;
    double* sI = sH + PF_EPAD;
    if (NM > 0)
        for (int e = threadIdx.x; e < PF_EPAD; e += blockDim.x) {
            sT[e] = e < A.E ? A.T[e] : PF_INF;
            sH[e] = e < A.E ? A.Hc[e] : PF_INF;
            if (e < A.E) sI[e] = A.inv2N[e];
        }
    __syncthreads();
    long long r = (long long)blockIdx.x * PF_BS + threadIdx.x;
    if (r >= nrep) return;
    const int n = A.n;
    Lane ln = make_lane(A, m, rep0 + r);
    ln.seed = seed;
    ln.stream = 2;
    ln.ebuf = -dlog(uni(ln));
    int root = 0;
    for (int i = 1; i < n; ++i) {
        int ni = i - 1;
        double tc = coalesce_up(ln, [&](int k) { return LS(ln, k); }, ni, i, 0.0);
        int pr = -1, ps = 0;
        int k = lineages_at(ln, ni, tc, -1, &pr, &ps);
        bool above_root = (ni == 0) || (tc >= LS(ln, ni - 1));
        int kk = above_root ? 1 : k;
        double u = uni(ln);
        int idx = min((int)(u * (double)kk), kk - 1);
        if (above_root) insert_node(ln, ni, tc, i, -1, 0, root);
        else { lineages_at(ln, ni, tc, idx, &pr, &ps); insert_node(ln, ni, tc, i, pr, ps, root); }
        root = n + ni;
    }
    ln.Ltree = tree_length(ln, n);
    // original internal-node heights live in the t0 scratch column of this lane
    double* orig = m.t0 + threadIdx.x;
    int alive = n - 1;
    for (int j = 0; j < n - 1; ++j) {
        orig[j * PF_BS] = LS(ln, j);
        out_epoch[r * (n - 1) + j] = epoch_of(ln, LS(ln, j));
        out_dist[r * (n - 1) + j] = -1.0;
    }
    pf_mask_t alive_mask = ((pf_mask_t)1 << (n - 1)) - 1u;
    double next = sample_next_base(ln, 0.0);
    const double stop = A.L * 0.6;
    if constexpr (NM > 0) {
        RTree<NM> t;
#pragma unroll
        for (int rr = 0; rr < RTree<NM>::NI; ++rr) {
            t.S[rr] = 0.0; t.C0[rr] = 0; t.C1[rr] = 0;
            if (rr < n - 1) { t.S[rr] = LS(ln, rr); t.C0[rr] = LC(ln, rr, 0); t.C1[rr] = LC(ln, rr, 1); }
        }
        RCtx cx;
        cx.T = sT; cx.I = sI; cx.H = sH; cx.E = A.E; cx.n = n; cx.L = A.L; cx.mu = A.mu; cx.rho = A.rho;
        cx.seed = seed; cx.slot = ln.slot; cx.stream = 2; cx.ctr = ln.ctr; cx.ebuf = ln.ebuf; cx.Ltree = ln.Ltree;
        cx.nb = 1; cx.bH = nullptr; cx.bS = nullptr; cx.last_iw = 1.0; cx.want_desc = false; cx.want_desc_new = false; cx.last_desc = 0; cx.last_desc_new = 0;
        cx.vbc = nullptr; cx.upd_fac = 1.0;
        cx.gK = 0; cx.gpos = nullptr; cx.grho = nullptr; cx.gleaf = nullptr; cx.last_rbiw = 1.0; cx.ridx = 0; cx.g_rp = 0; cx.g_sb = 0;
        while (alive > 0 && next < stop) {
            const double x = next;
            double h, tc, sp;
            bool changed;
            r_genealogy_update<NM, false>(cx, t, &h, &tc, &sp, &changed);
            if (changed) {
                for (int j = 0; j < n - 1; ++j)
                    if (((alive_mask >> j) & 1u) && orig[j * PF_BS] == sp) {
                        out_dist[r * (n - 1) + j] = x;
                        alive_mask &= ~((pf_mask_t)1 << j);
                        --alive;
                        break;
                    }
            }
            next = r_sample_next_base<true>(cx, x);
        }
        return;
    }
    while (alive > 0 && next < stop) {
        double x = next;
        double h, tc, sp;
        bool changed;
        genealogy_update(ln, &h, &tc, &sp, &changed);
        if (changed) {
            for (int j = 0; j < n - 1; ++j)
                if (((alive_mask >> j) & 1u) && orig[j * PF_BS] == sp) {
                    out_dist[r * (n - 1) + j] = x;
                    alive_mask &= ~((pf_mask_t)1 << j);
                    --alive;
                    break;
                }
        }
        next = sample_next_base(ln, x);
        ln.uqn = 0;
    }
}

// ------------------------------------------------------------------ k_simulate: synthetic data on the device
// The `.seg` producer next to the path (the reference shells out to scrm and converts its
// output, populationmodels.py:440-577).  One lane = one independent chromosome chunk: a prior tree, then along the
// sequence the same SMC' transition the filter simulates (genealogy_update), and between recombinations mutations
// dropped as a Poisson process of rate mu * tree length, each on a branch drawn in proportion to its length
// (sample_point) -- the carriers are the samples below it.  Output per chunk: site positions (continuous, ascending)
// and carrier masks; the host rounds them to bases and writes rows.  Its own Philox stream (3).
__device__ __forceinline__ void simulate_lds_body(const KArgs& A, unsigned long long seed, int nchunks, long long max_sites,
                                                  double* pos_out, pf_mask_t* mask_out, long long* n_out, double* smem) {
    Smem m = carve(smem, A.n, A.E);
    load_model(A, m);
    __syncthreads();
    const long long r = (long long)blockIdx.x * PF_BS + threadIdx.x;
    if (r >= nchunks) return;
    const int n = A.n;
    Lane ln = make_lane(A, m, r);
    ln.seed = seed;
    ln.stream = 3;
    ln.ebuf = -dlog(uni(ln));
    int root = 0;
    for (int i = 1; i < n; ++i) {            // Forest::buildInitialTree: the leaves join one at a time (as k_calibrate)
        int ni = i - 1;
        double tc = coalesce_up(ln, [&](int k) { return LS(ln, k); }, ni, i, 0.0);
        int pr = -1, ps = 0;
        int k = lineages_at(ln, ni, tc, -1, &pr, &ps);
        bool above_root = (ni == 0) || (tc >= LS(ln, ni - 1));
        int kk = above_root ? 1 : k;
        double u = uni(ln);
        int idx = min((int)(u * (double)kk), kk - 1);
        if (above_root) insert_node(ln, ni, tc, i, -1, 0, root);
        else { lineages_at(ln, ni, tc, idx, &pr, &ps); insert_node(ln, ni, tc, i, pr, ps, root); }
        root = n + ni;
    }
    ln.Ltree = tree_length(ln, n);
    double* tmp = m.t0 + threadIdx.x;        // per-lane LDS column for the descendant masks
    double* pos = pos_out + (size_t)r * max_sites;
    pf_mask_t* msk = mask_out + (size_t)r * max_sites;
    long long ns = 0;
    double x = 0.0;
    double next_rec = sample_next_base(ln, 0.0);
    double next_mut = x + (-dlog(uni(ln))) / (A.mu * ln.Ltree);
    bool overflow = false;
    while (x < A.L) {
        if (next_mut < next_rec && next_mut < A.L) {
            // a mutation on the current tree: a uniform point of the tree picks the branch
            int rp = 0, sb = 0;
            double h;
            ln.uqn = 0;
            sample_point(ln, &rp, &sb, &h);
            const pf_mask_t carriers = lane_desc_mask(ln, LC(ln, rp, sb), tmp);
            if (ns < max_sites) { pos[ns] = next_mut; msk[ns] = carriers; }
            else overflow = true;
            ++ns;
            x = next_mut;
            next_mut = x + (-dlog(uni(ln))) / (A.mu * ln.Ltree);
            continue;
        }
        x = next_rec;
        if (!(x < A.L)) break;
        double h, tc, sp;
        bool changed;
        genealogy_update(ln, &h, &tc, &sp, &changed);
        ln.uqn = 0;                           // what is left of the update's uniforms is not reused
        next_rec = sample_next_base(ln, x);
        next_mut = x + (-dlog(uni(ln))) / (A.mu * ln.Ltree);     // memoryless: redrawn under the new tree length
    }
    n_out[r] = overflow ? -ns : ns;
}
