// smcsmc_amd/csrc/pf_lds_pipe.h -- the extend role of the row pipeline on the per-lane LDS tree (k_sweep_xl, pf_hip.hip): one
// population, 9 to PF_NMAX haplotypes.  What extend_lds_body (pf_lds_body.h) does for a row between k_resample and k_decide,
// with the decision on the previous row, the parent search and k_resample's part taken into the prologue, as
// extend_reg_body<..., PIPE> does for the register tree.  A function of its own: k_extend, k_extend_wide and the calibration
// and simulation kernels keep the body they had, instruction for instruction.
// The price is a second copy of the skeleton: from "the row" on, extend_lds_pipe_body repeats extend_lds_body's row loop (the order of
// its steps, the record of an update, the guide's change of rate), and the prologue follows extend_reg_body<..., PIPE> (pf_hip.hip).  A
// change to that order belongs in both; tests/test_gpu_sweep_lds.py holds the copies together bit for bit.  What the steps are made of --
// the guide's factor, the delayed-factor store, the site likelihood, the tree and chain stores, the wavefront partials -- has one
// definition, in pf_row_parts.h.
// The prologue (what is requested first, the decision and the parent search), k_resample's part, the log-ring check and the partials are
// functions of their own (lds_pipe_request, lds_pipe_decide, lds_pipe_complete, pipe_log_ring_check, lds_pipe_partials): the extend role of
// the structured models from 9 to 16 haplotypes (k_sweep_xlmp, pf_mp_pipe.h, 64 lanes a workgroup) calls the same ones.
#pragma once
#include "pf_device.h"
#include "pf_types.h"
#include "pf_lane.h"
#include "pf_pipe.h"
#include "pf_look_lds.h"
#include "pf_row_parts.h"

// the decision tables of the prologue lie where the lanes' tree columns (S, t0, t1) go afterwards
__host__ __device__ inline bool lds_pipe_tables_fit(int n, int nc) { return pipe_lds_doubles(nc) <= (size_t)3 * (n - 1) * PF_BS; }

// ---- The pieces of the prologue and of the end of a row that the LDS-tree extend roles share: k_sweep_xl (below: one population, 256 lanes a
// workgroup) and k_sweep_xlmp (pf_mp_pipe.h: structured models, 64 lanes a workgroup, PF_BS of its translation unit).  One particle a lane in both. ----

// Everything the prologue and the lane need first, requested in one round trip: the row's own segment, the partials of the decision, the pilot
// scans around this workgroup (the parent search of a resampling row), what the slot owns.
struct LdsPipeReq {
    double sg_start = 0.0, sg_len = 0.0;
    int sg_limit = 0, sg_state = 1;
    int fs = 0;                               // the ring slot the row continues from
    RowPre pre;
    long long o_nres = 0; int o_bflag = 0, o_bgen = 0;
    double spec_sm[PF_PIPE_STAGE * 64 / PF_BS];
    int spec_lo = 0;
    double o_sm = 0.0, o_xmark = 0.0, o_ebuf = 0.0;
    int o_ml = 0;
    unsigned o_widx = 0;
    unsigned long long o_ctr = 0;
};
template <class KA>
__device__ __forceinline__ LdsPipeReq lds_pipe_request(const KA& A, long long s, const PipeRow& PR, long long p, bool active) {
    const Ctrl* c = A.ctrl;
    LdsPipeReq R;
    if (PR.extend) {
        R.sg_start = A.seg_start[s]; R.sg_len = A.seg_len[s];
        R.sg_limit = A.seg_limit[s]; R.sg_state = A.seg_state[s];
    }
    const int fs = __builtin_amdgcn_readfirstlane(PR.slot_prev >= 0 ? PR.slot_prev : c->cur);
    R.fs = fs;
    if (PR.complete) {
        R.pre = row_preload<PF_BS>(A, fs);
        // the row before it: what the extend role of the previous launch noted (the bookkeeping role runs on another stream and
        // is not waited for)
        const int bs = (fs + PF_RING - 1) & (PF_RING - 1);
        R.o_nres = c->xr[bs].n_res; R.o_bflag = c->xr[bs].flag; R.o_bgen = c->xr[bs].gen;
        R.spec_lo = pf_bx() * (PF_BS / 64) - (PF_PIPE_STAGE - PF_BS / 64) / 2;
        if (R.spec_lo > A.nc - PF_PIPE_STAGE) R.spec_lo = A.nc - PF_PIPE_STAGE;
        if (R.spec_lo < 0) R.spec_lo = 0;
        const double* sm0 = A.rg_scan1m + (size_t)fs * A.Np;
#pragma unroll
        for (int k = 0; k < PF_PIPE_STAGE * 64 / PF_BS; ++k) {
            const long long src = (long long)R.spec_lo * 64 + k * PF_BS + threadIdx.x;
            R.spec_sm[k] = src < A.Np ? sm0[src] : PF_INF;
        }
    }
    if (active) {
        const DState own = state_slot(A, fs);
        R.o_xmark = own.x_mark[p]; R.o_ml = own.mark_limit[p];
        R.o_widx = PR.complete ? A.rg_widx[(size_t)fs * A.Np + p] : A.widx[p];
        R.o_ctr = A.rng_ctr[p]; R.o_ebuf = A.ebuf[p];
        if (PR.complete) R.o_sm = A.rg_scan1m[(size_t)fs * A.Np + p];
    }
    return R;
}

// The decision on the previous row and, when it resampled, the parent of every slot of this workgroup (extend_reg_body's prologue:
// decide_row, the offspring offsets in closed form, the two-level search over the pilot prefix sums).  `tables`: the LDS the decision's
// tables take (pipe_lds_doubles(A.nc) doubles, dead again when the caller has passed its next barrier).  Every thread of the workgroup
// calls this (barriers).  rg_blkcnt gets one entry a workgroup: KArgs::blk_gran says how many that is per 256 particles, 1 at 256 lanes, 4 at 64.
struct LdsPipeDec {
    bool gather = false;
    double inv = 1.0, S1v = 0.0;
    int lo_p = 0, lo_p1 = 0;
    bool first_copy = true;
    long long a = 0;               // the parent (the slot itself when the row did not resample)
    int G_end = 0, ev = 0;
};
template <class KA>
__device__ __forceinline__ LdsPipeDec lds_pipe_decide(const KA& A, const PipeRow& PR, const LdsPipeReq& R, double* tables, long long p, bool active) {
    const int lane = threadIdx.x & 63;
    const int fs = R.fs;
    LdsPipeDec D;
    D.a = p;
    if (PR.complete != 0) {
        PipeLds q = pipe_carve(tables, A.nc);
        const int row_slot = fs;
        const long long n_res = R.o_nres + R.o_bflag;
        D.G_end = R.o_bgen + R.o_bflag;
        D.ev = (int)n_res;
#pragma unroll
        for (int k = 0; k < PF_PIPE_STAGE * 64 / PF_BS; ++k) q.stage[k * PF_BS + threadIdx.x] = R.spec_sm[k];    // visible after decide_row's barriers
        RowDecision d = decide_row<true, PF_BS>(A, q, row_slot, n_res, R.pre);
        D.inv = d.inv; D.S1v = d.S1;
        D.gather = d.flag != 0;
        if (pf_bx() == 0 && threadIdx.x == 0) {
            Ctrl* cw = A.ctrl;
            cw->xr[row_slot].n_res = n_res; cw->xr[row_slot].gen = D.G_end; cw->xr[row_slot].flag = d.flag;
        }
        if (D.gather) {
            const double dn = (double)A.Np;
            const double invS1 = 1.0 / d.S1;
            const double* sm = A.rg_scan1m + (size_t)row_slot * A.Np;
            const int wave = threadIdx.x >> 6;
            const int ch_own = (int)(p >> 6);
            int lo_next = 0;
            if (active) {
                const double w = pipe_chunk_offset(q, ch_own) + R.o_sm;
                const double v_own = q.pmx[ch_own] > w ? q.pmx[ch_own] : w;          // largest pilot prefix sum up to particle p
                lo_next = p + 1 < A.Np ? pipe_lo_from(v_own, dn, A.Np, d.S1, invS1, d.u) : (int)A.Np;
                q.slo[threadIdx.x] = lo_next;
            }
            // parent of slot p: the first particle a with (p+u) * S1 < N * (largest prefix sum up to a)
            const double lhs = ((double)p + d.u) * d.S1;
            int pch = 0;
            if (active) {
                int lo_c = 0, hi_c = A.nc - 1;
                while (lo_c < hi_c) {
                    int mid = (lo_c + hi_c) >> 1;
                    if (lhs < dn * q.pmx[mid + 1]) hi_c = mid; else lo_c = mid + 1;
                }
                pch = lo_c;
            }
            int cmin = active ? pch : 0x7fffffff, cmax = active ? pch : -1;
            wave_minmax(cmin, cmax);
            if (lane == 0) { q.wint[wave] = cmin; q.wint[PF_BS / 64 + wave] = cmax; }
            __syncthreads();
            if (active) {
                D.lo_p1 = lo_next;
                if (threadIdx.x > 0) D.lo_p = q.slo[threadIdx.x - 1];
                else D.lo_p = p > 0 ? pipe_lo_from(q.pmx[ch_own], dn, A.Np, d.S1, invS1, d.u) : 0;
            }
            cmin = q.wint[0]; cmax = q.wint[PF_BS / 64];
            for (int w = 1; w < PF_BS / 64; ++w) {
                cmin = q.wint[w] < cmin ? q.wint[w] : cmin;
                cmax = q.wint[PF_BS / 64 + w] > cmax ? q.wint[PF_BS / 64 + w] : cmax;
            }
            // survivors of this workgroup (the ledger positions the run list of the ending generation with them)
            {
                unsigned long long bal = __ballot(active && D.lo_p1 > D.lo_p);
                if (lane == 0) q.wint[2 * (PF_BS / 64) + wave] = __popcll(bal);
            }
            int nst = cmax - cmin + 1;
            if (nst > PF_PIPE_STAGE) nst = PF_PIPE_STAGE;
            if (nst < 0) nst = 0;
            int stage_lo = cmin;
            if (cmin >= R.spec_lo && cmax < R.spec_lo + PF_PIPE_STAGE) {
                stage_lo = R.spec_lo; nst = PF_PIPE_STAGE;       // the scans requested with the prologue cover the range
            } else {
                __syncthreads();                               // everybody has read the range before the buffer is refilled
                for (int idx = threadIdx.x; idx < nst * 64; idx += PF_BS) {
                    long long src = (long long)cmin * 64 + idx;
                    q.stage[idx] = src < A.Np ? sm[src] : PF_INF;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int tot = 0;
                for (int w = 0; w < PF_BS / 64; ++w) tot += q.wint[2 * (PF_BS / 64) + w];
                A.rg_blkcnt[(size_t)row_slot * (size_t)((A.Np + 255) / 256) * A.blk_gran + pf_bx()] = tot;
            }
            if (active) {
                const double coff_p = pipe_chunk_offset(q, pch);
                const double pm_p = q.pmx[pch];
                const bool staged = pch >= stage_lo && pch - stage_lo < nst;
                auto val_at = [&](int l) -> double {           // largest prefix sum up to particle pch*64 + l
                    long long idx = (long long)pch * 64 + l;
                    double smv = staged ? q.stage[(pch - stage_lo) * 64 + l] : (idx < A.Np ? sm[idx] : PF_INF);
                    double w = coff_p + smv;
                    return pm_p > w ? pm_p : w;
                };
                int lo_l = 0, hi_l = 63;
                while (lo_l < hi_l) {
                    int mid = (lo_l + hi_l) >> 1;
                    if (lhs < dn * val_at(mid)) hi_l = mid; else lo_l = mid + 1;
                }
                long long a = (long long)pch * 64 + lo_l;
                if (a > A.Np - 1) a = A.Np - 1;
                // slot p is the first copy of a (it keeps a's next recombination position) iff it equals a's offset
                const int la = (int)(a & 63);
                if (p == 0 || a == 0) D.first_copy = (p == 0);
                else {
                    double vprev = la > 0 ? val_at(la - 1) : pm_p;      // largest prefix sum up to a - 1
                    if (a != (long long)pch * 64 + lo_l) {             // clamped: recompute on the true chunk of a - 1
                        long long am = a - 1;
                        int chm = (int)(am >> 6);
                        double w = pipe_chunk_offset(q, chm) + sm[am];
                        vprev = q.pmx[chm] > w ? q.pmx[chm] : w;
                    }
                    D.first_copy = ((((double)(p - 1)) + d.u) * d.S1 < dn * vprev);
                }
                D.a = a;
                // the offspring table of the generation that ends here, for the ledger
                int* lo_tab = A.lo + (size_t)(D.G_end % A.Gcap) * (A.Np + 1);
                lo_tab[p] = D.lo_p;
                if (p == A.Np - 1) lo_tab[A.Np] = (int)A.Np;
            }
        }
    }
    return D;
}

// k_resample's part (pc.cpp:321-392, 435-437), operation for operation, on the values the lane has loaded from its parent `from[a]`:
// normalisation, or the closing record of the old slot p, the generation mark, the weights of a copy and a fresh position for all but the first
template <class KA>
__device__ __forceinline__ void lds_pipe_complete(const KA& A, const DState& from, Lane& ln, long long p, const LdsPipeReq& R, const LdsPipeDec& D,
                                                  double pos_prev, int ridx, double& w_post, double& w_pilot, double& x_mark, double& next_base,
                                                  unsigned& widx) {
    const int n = A.n;
    if (!D.gather) {
        w_post *= D.inv;                             // normalize_probability, pc.cpp:435-437
        w_pilot *= D.inv;
    } else {
        // role of the old slot p: close its stretch if it has offspring
        if (D.lo_p1 > D.lo_p) {
            double* rec = rec_ptr(A, p, widx);
            rec[0] = R.o_xmark;
            rec[1] = pos_prev;
            rec[2] = 0.0; rec[3] = 0.0;
            rec[4] = __longlong_as_double((long long)make_meta(1, R.o_ml, -1, n));
            for (int r = 0; r < n - 1; ++r) rec[5 + r] = from.S[(size_t)r * A.Np + p];
            ++widx;
        }
        A.gstart[(size_t)((D.G_end + 1) % A.Gcap) * A.Np + p] = widx;
        // role of the new slot p: weights of the copy (pc.cpp:350-351), fresh position for all but the first
        if (D.ev < A.max_trace_events) A.ev_parents[(size_t)D.ev * A.Np + p] = (int)D.a;
        const double wp = w_post * D.inv;
        const double wq = w_pilot * D.inv;
        const double sumn = D.S1v * D.inv;
        const double adj = sumn / ((double)A.Np * wq);
        w_post = wp * adj;
        w_pilot = wq * adj;
        x_mark = pos_prev;
        if (!D.first_copy && pos_prev < A.L) next_base = sample_next_base_guided(ln, pos_prev, A.g_K, A.g_pos, A.g_rho, ridx);     // pc.cpp:357-368
    }
}

// The extend launch runs up to PF_RING - 2 rows ahead of the counts: the writer itself checks that it has not overwritten a record that a
// pending count can still ask for (Ctrl::g_safe: the oldest generation those counts reach)
template <class KA>
__device__ __forceinline__ void pipe_log_ring_check(const KA& A, long long p, unsigned widx) {
    const unsigned kold = A.gstart[(size_t)(A.ctrl->g_safe % A.Gcap) * A.Np + p];
    if (widx - kold > A.cap && !A.ctrl->err) A.ctrl->err = ERR_LOG_OVERFLOW;
}

// per-wavefront canonical partials (level 1 of the radix-64 reduction / scan) into ring slot `cur` of the row
template <class KA>
__device__ __forceinline__ void lds_pipe_partials(const KA& A, const PipeRow& PR, int cur, long long p, bool active, double w_post, double w_pilot,
                                                  bool biased, bool has_pending) {
    const int lane = threadIdx.x & 63;
    row_scans_store(A, cur, p, active, lane, row_scans(w_post, w_pilot, lane));
    const long long chunk = p >> 6;
    const size_t co = (size_t)cur * A.nc;
    if (biased) {
        unsigned long long pend = __ballot(has_pending);
        if (lane == 0 && chunk < A.nc) {
            A.rg_dpend[co + chunk] = __popcll(pend);
            if (!PR.extend) A.chunk_dpend[chunk] = __popcll(pend);     // the state goes back to the general kernels
        }
    }
}

// BIASED: focused sampling or a guide (the delayed-factor store, the guide's segment index)
// LOOK (without BIASED; k_sweep_xl<false, true>, pf_lookahead.flags bit 2): the auxiliary particle filter's look-ahead factor (look_factor_lds,
// pf_look_lds.h = k_lookahead) enters the pilot weight behind the site likelihood and in front of the state stores and the wavefront
// partials, so that the partials lds_pipe_decide reads in the next launch are those k_lookahead leaves.  The previous factor travels with
// the state: the slot's own, the parent's on a resampling row.  A completion-only launch applies none, reads no look-ahead row (its row may
// lie past the table) and hands on the factor it carried.  No LDS beyond the plain instance's.
template <bool BIASED, bool LOOK = false, class KA>
__device__ __forceinline__ void extend_lds_pipe_body(const KA& A, long long s, const PipeRow PR, double* smem) {
    static_assert(!LOOK || !BIASED, "the look-ahead rides on the plain rows of k_sweep_xl");
    Smem m = carve(smem, A.n, A.E);
    __shared__ double sBH[PF_BIAS_MAX + 2], sBS[PF_BIAS_MAX + 1];      // focused sampling: band boundaries / strengths
    const Ctrl* c = A.ctrl;
    const int n = A.n;
    const long long p = (long long)pf_bx() * PF_BS + threadIdx.x;
    const bool active = p < A.Np;
    const bool guided = BIASED && A.g_K > 0;
    const bool biased = BIASED;                          // a guide alone runs with one band of strength 1
    const LdsPipeReq R = lds_pipe_request(A, s, PR, p, active);
    const double sg_start = R.sg_start, sg_len = R.sg_len;
    const int sg_limit = R.sg_limit, sg_state = R.sg_state;
    const int fs = R.fs;
    load_model(A, m);
    if (threadIdx.x < PF_BIAS_MAX + 2) {
        sBH[threadIdx.x] = A.bias_H[threadIdx.x];
        if (threadIdx.x < PF_BIAS_MAX + 1) sBS[threadIdx.x] = A.bias_S[threadIdx.x];
    }
    // the decision's tables lie where the lanes' tree columns go afterwards (lds_pipe_tables_fit)
    const bool completing = PR.complete != 0;
    const double pos_prev = PR.pos_prev;
    const LdsPipeDec D = lds_pipe_decide(A, PR, R, smem, p, active);
    const long long a = D.a;
    __syncthreads();          // the tables are dead from here on: the lanes' tree columns take their place (and the model tables are in)
    const int cur = __builtin_amdgcn_readfirstlane(PR.slot_out);
    const int from_slot = fs;
    bool has_pending = false;
    double w_post = 0.0, w_pilot = 0.0;
    if (active) {
        const DState st = state_slot(A, cur);
        const DState from = state_slot(A, from_slot);
        Lane ln = make_lane(A, m, p);
        // the parent's tree into this lane's columns (its own when the row did not resample)
        lane_load_tree(ln, from, (size_t)A.Np, a, n);
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
        double* tmp0 = m.t0 + threadIdx.x;
        double* tmp1 = m.t1 + threadIdx.x;
        if (completing) lds_pipe_complete(A, from, ln, p, R, D, pos_prev, ridx, w_post, w_pilot, x_mark, next_base, widx);

        // ---- the row itself: extend_lds_body ----
        const bool do_extend = PR.extend != 0;             // the flush step of a call only completes the last row
        const int8_t* data = A.seg_alleles + (size_t)s * n;
        const double seg_end = do_extend ? sg_start + sg_len : 0.0;
        const double extend_to = seg_end < A.L ? seg_end : A.L;
        const int limit = sg_limit;
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
                // a recombination: log the stretch that ends here together with the event
                double* rec = rec_ptr(A, p, widx);
                rec[0] = x_mark;
                rec[1] = updated_to;
                for (int r = 0; r < n - 1; ++r) rec[5 + r] = LS(ln, r);
                double h, tc, sp_removed;
                bool changed;
                pf_mask_t desc = 0;
                double iw = 1.0, rbiw = 1.0;
                genealogy_update(ln, &h, &tc, &sp_removed, &changed, A.lmap_opp ? &desc : nullptr, tmp0,
                                 biased ? sBH : nullptr, sBS, A.n_bias + 1, &iw,
                                 guided ? A.g_leaf + (size_t)ridx * n : nullptr, guided ? A.rho / A.g_rho[ridx] : 1.0, &rbiw, nullptr);
                if (ln.vbc) { w_post *= ln.upd_fac; w_pilot *= ln.upd_fac; ln.upd_fac = 1.0; }
                rec[2] = h;
                rec[3] = tc;
                rec[4] = __longlong_as_double((long long)make_meta(0, mark_limit, limit, n, desc, 0u));
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

        if (biased) has_pending = row_apply_due(ds, st, p, extend_to, do_extend, guided, ridx, w_pilot);
        if (do_extend && sg_state == 0) {
            const double lik = lane_site_weight(ln, data, n, A.flags & 2, A.flags & 1, tmp0, tmp1);
            w_post *= lik;
            w_pilot *= lik;
        }
        if constexpr (LOOK) {
            // removeLookaheadLikelihood + includeLookaheadLikelihood (particle.hpp:182, particle.cpp:614-616), as k_lookahead ends
            double la_w = la_prev;
            if (do_extend) {
                const double likelihood = look_factor_lds(A, ln, s, ln.Ltree, tmp0, tmp1);
                w_pilot /= la_prev;
                la_w = 1.0;
                la_w *= likelihood;
                w_pilot *= likelihood;
            }
            st.lookahead[p] = la_w;          // (the slot the general kernels and the step API read when the call ends here)
        }

        lane_store_tree(ln, st, (size_t)A.Np, p, n);
        st.w_post[p] = w_post;
        st.w_pilot[p] = w_pilot;
        lane_store_chain(A, st, p, next_base, x_mark, mark_limit, ln);
        A.rg_widx[(size_t)cur * A.Np + p] = widx;
        if (!do_extend) A.widx[p] = widx;              // the state goes back to the general kernels
        pipe_log_ring_check(A, p, widx);
    }
    lds_pipe_partials(A, PR, cur, p, active, w_post, w_pilot, biased, has_pending);
}
