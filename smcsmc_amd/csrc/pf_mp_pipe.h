// smcsmc_amd/csrc/pf_mp_pipe.h -- the extend role of the row pipeline for structured models on the per-lane LDS tree (k_sweep_xlmp, pf_mp.hip):
// two to four populations, 9 to PF_NMAX haplotypes, only on handles created with PF_FLAG_MP_LDS_ROWS.  It is to k_extend_mp what k_sweep_xl
// (pf_lds_pipe.h) is to k_extend and what k_sweep_xmp is to k_extend_mpr: the decision on the previous row, the parent search and k_resample's
// part are in the prologue, the state is read from one slot of the sixteen-slot ring and written to the next, nothing of k_decide is read.
// Included by pf_mp.hip behind k_extend_mp (SmemMP, carve_mp, load_model_mp, make_mlane, mp_report, store_mp_state, piece_ref are that file's).
//   prologue, k_resample's part, log-ring check, partials: the functions of pf_lds_pipe.h, shared with k_sweep_xl (64 lanes a workgroup here)
//   the gather: tree, node populations and the migration list of the parent into this lane's LDS columns
//   the row: the skeleton of k_extend_mp's row loop (the order of its steps, sample_point*, mp_genealogy_rest and the walk of pf_mp.h, the record
//            of an update), from "the row" on; a change to that order belongs in both, tests/test_gpu_sweep_structured_lds.py holds them together
//            through the oracle, bit for bit.  What the steps are made of (guide's factor, delayed-factor store, site likelihood, tree and chain
//            stores) has one definition, in pf_row_parts.h
// No -arg on this path (create_plan, run_path).  A look-ahead: the LOOK instance (k_sweep_xlmp<false, true>), on handles whose look-ahead was
// loaded with PF_LA_ROW_PIPELINE_LDS (run_path: look_on_rows_lds); without the bit such a handle goes to the general kernels.
#pragma once
#include "pf_lds_pipe.h"

// the lane's migration events (LDS columns, sorted by time) as look_factor_lds reads them
struct LookMigL {
    static constexpr bool on = true;
    const MLane& ml;
    __device__ __forceinline__ int count() const { return ml.nm; }
    __device__ __forceinline__ int branch(int mi) const { return LMb(ml, mi); }
    __device__ __forceinline__ double time(int mi) const { return LMt(ml, mi); }
};

// Where the decision's tables go: into the lanes' migration-time column (mcap * 64 doubles, loaded once the previous row is decided) when they
// fit there, behind everything else otherwise (a small mig_cap).  Dynamic LDS of the launch; 0: more than the 160 KB of a workgroup.
__host__ __device__ inline bool mp_pipe_tables_inside(int mcap, int nc) { return pipe_lds_doubles(nc) <= (size_t)mcap * PF_BS; }
static size_t smem_bytes_mp_pipe(int n, int E, int P, int mcap, int nc) {
    const size_t total = smem_bytes_mp(n, E, P, mcap) + (mp_pipe_tables_inside(mcap, nc) ? 0 : pipe_lds_doubles(nc) * 8);
    return total <= 160 * 1024 ? total : 0;
}

// BIASED: focused sampling or a guide (the delayed-factor store, the guide's segment index)
// LOOK (without BIASED; k_sweep_xlmp<false, true>, pf_lookahead.flags bit 2): the look-ahead factor in the pilot weight, as in
// extend_lds_pipe_body<..., LOOK>, with the lane's migration events for the height of a leaf's branch (LookMigL).  Its scratch lies in the
// lane's columns t0 and t1, never in the decision's tables (dead by then, inside the event list or behind the state).
template <bool BIASED, bool LOOK = false, class KA>
__device__ __forceinline__ void extend_mp_pipe_body(const KA& A, long long s, const PipeRow PR, double* smem) {
    static_assert(!LOOK || !BIASED, "the look-ahead rides on the plain rows of k_sweep_xlmp");
    Smem m = carve(smem, A.n, A.E);
    SmemMP mm = carve_mp(smem, A.n, A.E, A.P, A.mcap);
    __shared__ double sBH[PF_BIAS_MAX + 2], sBS[PF_BIAS_MAX + 1];      // focused sampling: band boundaries / strengths
    const Ctrl* c = A.ctrl;
    const int n = A.n;
    const long long p = (long long)pf_bx() * PF_BS + threadIdx.x;
    const bool active = p < A.Np;
    const bool guided = BIASED && A.g_K > 0;
    const bool biased = BIASED && (A.n_bias > 0 || guided);          // a guide alone runs with one band of strength 1
    const LdsPipeReq R = lds_pipe_request(A, s, PR, p, active);
    load_model(A, m);
    load_model_mp(A, mm);
    if (threadIdx.x < PF_BIAS_MAX + 2) {
        sBH[threadIdx.x] = A.bias_H[threadIdx.x];
        if (threadIdx.x < PF_BIAS_MAX + 1) sBS[threadIdx.x] = A.bias_S[threadIdx.x];
    }
    const bool completing = PR.complete != 0;
    const double pos_prev = PR.pos_prev;
    double* tables = mp_pipe_tables_inside(A.mcap, A.nc) ? mm.Mt : (double*)((char*)smem + smem_bytes(A.n, A.E) + smem_mp_extra(A.n, A.E, A.P, A.mcap));
    const LdsPipeDec D = lds_pipe_decide(A, PR, R, tables, p, active);
    const long long a = D.a;
    __syncthreads();          // the tables are dead from here on: the lanes' event lists take their place (and the model tables are in)
    const int cur = __builtin_amdgcn_readfirstlane(PR.slot_out);
    bool has_pending = false;
    double w_post = 0.0, w_pilot = 0.0;
    if (active) {
        const DState st = state_slot(A, cur);
        const DState from = state_slot(A, R.fs);
        Lane ln = make_lane(A, m, p);
        MLane ml = make_mlane(A, mm);
        // the parent's tree, node populations and migration list into this lane's columns (its own when the row did not resample)
        lane_load_tree(ln, from, (size_t)A.Np, a, n);
        for (int r = 0; r < n - 1; ++r) LPn(ml, r) = from.Pn[(size_t)r * A.Np + a];
        ml.nm = from.nm[a];
        for (int q = 0; q < ml.nm; ++q) {
            LMt(ml, q) = from.Mt[(size_t)q * A.Np + a];
            LMb(ml, q) = from.Mb[(size_t)q * A.Np + a];
            LMq(ml, q) = from.Mq[(size_t)q * A.Np + a];
        }
        w_post = from.w_post[a];
        w_pilot = from.w_pilot[a];
        double next_base = from.next_base[a];
        double x_mark = from.x_mark[a];
        int mark_limit = from.mark_limit[a];
        ln.Ltree = from.Ltree[a];
        [[maybe_unused]] double la_prev = 1.0;
        if constexpr (LOOK) la_prev = from.lookahead[a];       // the parent's on a resampling row, the slot's own otherwise
        ln.ctr = R.o_ctr;
        ln.ebuf = R.o_ebuf;
        unsigned widx = R.o_widx;
        DStore ds;
        d_bind(ds, A, st, p);
        ds.count = 0; ds.total = 1.0;
        if (biased) {
            ds.count = from.dcount[a]; ds.total = from.total_delayed[a];
            // the copy constructor copies the pending factors (particle.cpp:122-123); the ring moves them every row
            row_copy_pending(st, from, (size_t)A.Np, p, a, ds.count);
        }
        int ridx = guided ? from.ridx[a] : 0;
        PLog pl;
        pl.base = A.plog + (size_t)p * A.pcap * 3; pl.cap = A.pcap; pl.idx = A.pidx[p]; pl.pos = pl.idx % pl.cap; pl.on = true;
        pl.fopen = false; pl.ropen = false;
        double* tmp0 = m.t0 + threadIdx.x;
        double* tmp1 = m.t1 + threadIdx.x;
        if (completing) lds_pipe_complete(A, from, ln, p, R, D, pos_prev, ridx, w_post, w_pilot, x_mark, next_base, widx);

        // ---- the row itself: k_extend_mp ----
        const bool do_extend = PR.extend != 0;             // the flush step of a call only completes the last row
        const int8_t* data = A.seg_alleles + (size_t)s * n;
        const double seg_end = do_extend ? R.sg_start + R.sg_len : 0.0;
        const double extend_to = seg_end < A.L ? seg_end : A.L;
        const int limit = R.sg_limit;
        const int leaf_status = lane_leaf_status(data, n, do_extend);

        double updated_to = completing ? pos_prev : c->cur_pos;
        if (!do_extend) updated_to = extend_to;             // completion only: the loop below does not run
        double B = 0;
        if (do_extend) {
            if (leaf_status == -1) B = 0;
            else if (leaf_status == 1) B = ln.Ltree;
            else B = tracked_len_lane(ln, data, tmp0);
        }

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
                double* rec = rec_ptr(A, p, widx);
                rec[0] = x_mark;
                rec[1] = updated_to;
                for (int r = 0; r < n - 1; ++r) rec[5 + r] = LS(ln, r);
                int rp = 0, sb = 0;
                double h, tc, sp_removed;
                bool changed;
                double iw = 1.0, rbiw = 1.0;
                if (guided)
                    sample_point_guided(ln, sBH, sBS, A.n_bias + 1, A.g_leaf + (size_t)ridx * n, A.rho / A.g_rho[ridx], &rp, &sb, &h,
                                        &iw, &rbiw, tmp0);
                else if (biased) { sample_point_biased(ln, sBH, sBS, A.n_bias + 1, &rp, &sb, &h, &iw); rbiw = iw; }
                else sample_point(ln, &rp, &sb, &h);
                const unsigned desc = A.lmap_opp ? lane_desc_mask(ln, LC(ln, rp, sb), tmp0) : 0u;
                unsigned p0 = pl.idx;
                double tfirst = 0.0;
                unsigned span = 0;
                mp_genealogy_rest<true, false>(ln, ml, pl, limit, rp, sb, h, &tc, &sp_removed, &changed, &tfirst, &span, desc, tmp0);
                if (ln.vbc) { w_post *= ln.upd_fac; w_pilot *= ln.upd_fac; ln.upd_fac = 1.0; }
                rec[2] = h;
                rec[3] = piece_ref(p0, pl.idx - p0);
                rec[4] = __longlong_as_double((long long)make_meta(0, mark_limit, limit, n, desc, span));
                ++widx;
                if (ml.err) break;
                if (leaf_status == 0) B = tracked_len_lane(ln, data, tmp0);
                if (leaf_status == 1) B = ln.Ltree;
                if (biased) {
                    const double delay_height = (A.delay_type & 3) == 0 ? h : ((A.delay_type & 3) == 2 ? tfirst : tc);
                    row_delayed_factor(ds, sBH, sBS, A.n_bias + 1, A.delay_type, delay_height, iw, rbiw, A.app_delays[epoch_of(ln, delay_height)], updated_to, w_post, w_pilot);
                }
                next_base = sample_next_base_guided(ln, updated_to, A.g_K, A.g_pos, A.g_rho, ridx);
                x_mark = updated_to;
                mark_limit = limit;
            }
        }
        mp_report(A, ml);
        if (biased) has_pending = row_apply_due(ds, st, p, extend_to, do_extend, guided, ridx, w_pilot);

        if (do_extend && R.sg_state == 0) {
            const double lik = lane_site_weight(ln, data, n, A.flags & 2, A.flags & 1, tmp0, tmp1);
            w_post *= lik;
            w_pilot *= lik;
        }
        if constexpr (LOOK) {
            // removeLookaheadLikelihood + includeLookaheadLikelihood (particle.hpp:182, particle.cpp:614-616), as k_lookahead ends
            double la_w = la_prev;
            // (!ml.err: the one difference from k_lookahead, which takes every particle.  A lane whose event list overflowed left the loop above
            // in the middle of an update, its tree half edited; the run ends with mp_report's error whatever its weight is)
            if (do_extend && !ml.err) {
                const double likelihood = look_factor_lds(A, ln, s, ln.Ltree, tmp0, tmp1, LookMigL{ml});
                w_pilot /= la_prev;
                la_w = 1.0;
                la_w *= likelihood;
                w_pilot *= likelihood;
            }
            st.lookahead[p] = la_w;          // (the slot the general kernels and the step API read when the call ends here)
        }

        lane_store_tree(ln, st, (size_t)A.Np, p, n);
        store_mp_state(A, st, ln, ml, p);
        st.w_post[p] = w_post;
        st.w_pilot[p] = w_pilot;
        lane_store_chain(A, st, p, next_base, x_mark, mark_limit, ln);
        A.rg_widx[(size_t)cur * A.Np + p] = widx;
        if (!do_extend) A.widx[p] = widx;              // the state goes back to the general kernels
        A.pidx[p] = pl.idx;
        pipe_log_ring_check(A, p, widx);
    }
    lds_pipe_partials(A, PR, cur, p, active, w_post, w_pilot, biased, has_pending);
}
