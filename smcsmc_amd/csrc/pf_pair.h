// smcsmc_amd/csrc/pf_pair.h -- the paired form of the extend role of the headline row kernel (k_sweep4p; included by pf_hip.hip behind
// extend_reg_body, whose parts it shares by function: row_head_*, row_parent_*, row_stage_parents, row_ctx, row_update_trip, row_site_lik, row_copy_weights, row_store_*, row_scans*).
//
// A row of the one-wavefront form is one instruction stream per 64 particles, bound by instruction issue, and much of that stream does not lie
// on the genealogy's dependency chain (draws -> cut point -> selection -> re-coalescence -> edit -> tree length -> next recombination position):
// everything that only touches the weights hangs off it, and so does what belongs to the old slot of a resampling row.  Here an extend
// workgroup keeps its 256 threads and owns 128 particles.  Wavefronts 0 and 1 are TREE wavefronts, one particle a lane (particle
// bx * 128 + (tid & 127)); wavefronts 2 and 3 are WEIGHT wavefronts, lane l of wavefront w + 2 serving the particle of lane l of wavefront w.
// A workgroup of 256 threads has one wavefront on each SIMD of its compute unit, so the two streams of a particle issue side by side.  The form
// runs when every extend workgroup can have a compute unit of its own (run_sweep_split).
//
// Every arithmetic operation keeps its operands and its place in the particle's own order; only the wavefront that executes it changes:
//   head         all four wavefronts take the decision on the row before (decide_row over 256 threads, as in the other form)
//   resampling   tree: search of the chunk table, staging, search inside the wavefront, first copy, the parent's tree, gstart
//                weight: the slots' own offspring offsets (q.slo), then survivors, offspring table, closing record, ev_parents, and the
//                parent's weights by the parent index the tree wavefront leaves in LDS
//   update loop  tree: the loop without the no-mutation factor; at the head of a pass (B, new_to - updated_to) goes to the lane's slot of a ring
//                in LDS.  weight: f = fastexp(-mu * B * dt), w_post *= f, w_pilot *= f, in the order of the passes
//   tail         tree: site likelihood (through LDS), the tree's stores.  weight: the last product, the weights' stores, the five wavefront
//                primitives, scans and partials
// The hand-off words (ring, lik, pub, con, fin, lkf, stall) are read and written through pair_get / pair_put alone: volatile accesses through
// pointers whose type says LDS (address space 3), so each is one ds_read / ds_write and none a flat instruction.  (Through a generic
// `volatile PairLds*` every one was a flat access at system scope behind a wait for every request of the wavefront, the draw table's
// prefetch among them.)  What orders them: the compiler keeps volatile accesses in program order, and the DS instructions of one wavefront
// execute in order in the one LDS of the compute unit -- an entry is in place when its count is, pub is final once fin is set, lik is in place
// when lkf says so -- so no fence and no wait stands between an entry's stores and its count's; a reader waits (lgkmcnt) for a count only
// because it branches on it.  What they do NOT order: global memory.  A hand-off implies nothing about the stores and loads either wavefront
// has in flight, and nothing needs it to: within a row no role reads global memory the other writes (the closing record, the offspring table,
// ev_parents, the survivor counts, the weights and the scans are written by the weight wavefront and read by later launches; the tree's
// records, gstart -- which the check of the record ring reads back, hence on the tree wavefront -- state and counters likewise), and the
// parent index goes through LDS in front of a barrier.  A dependence through memory added later needs an order of its own.
// Every spin sleeps and is bounded by the 100 MHz clock (PF_PAIR_TICKS, 0.1 s where a row takes tens of microseconds): on expiry the
// wavefront notes ERR_PAIR_STALL and leaves, and so does every wavefront that sees the note.  No barrier stands inside or behind the update loop.
#pragma once

#define PF_PAIR_N 128                   // particles of an extend workgroup
#define PF_PAIR_DEPTH 8                 // entries a tree lane may be ahead of its weight lane
#define PF_PAIR_TICKS 10000000ull       // bound of a spin in ticks of the 100 MHz clock

struct PairLds {
    double ring[2][PF_PAIR_DEPTH][2][64];   // [pair][entry][B, dt][lane]
    double lik[2][64];
    unsigned pub[2][64];                // entries the tree lane has written this row
    unsigned con[2][64];                // entries the weight lane has applied
    unsigned fin[2][64];                // 1 + entries of the row, once the tree lane's loop has ended (0: still running)
    unsigned lkf[2][64];                // 1: the row has no site likelihood, 2: it is in lik (0: not yet known)
    int parent[PF_PAIR_N];              // resampling row: the parent of the slot
    int stall;                          // a wavefront of the workgroup gave up
};

#ifdef PF_STAMPS
// the stamps of a pair share the words of their particles' wavefront: the tree wavefront's under today's numbers, the weight wavefront's in
// words 29 to 31 (offsets done, last factor applied, scans done); word 15: the hardware ids of the two (tree low, weight high)
#define PF_PSTAMP(k) do { if (A.stamps && lane == 0 && s < A.stamp_rows && (p >> 6) < A.nc)                              \
        A.stamps[((size_t)s * A.nc + (size_t)(p >> 6)) * PF_STAMP_W + (k)] = wall_clock64(); } while (0)
#define PF_PHWID() do { if (A.stamps && lane == 0 && s < A.stamp_rows && (p >> 6) < A.nc)                                \
        ((unsigned*)&A.stamps[((size_t)s * A.nc + (size_t)(p >> 6)) * PF_STAMP_W + 15])[tree ? 0 : 1] = __builtin_amdgcn_s_getreg((31 << 11) | 4); } while (0)
#define PF_PACC_STORE do { if (A.stamps && lane == 0 && s < A.stamp_rows && (p >> 6) < A.nc) {                           \
        for (int k_ = 0; k_ < 6; ++k_) A.stamps[((size_t)s * A.nc + (size_t)(p >> 6)) * PF_STAMP_W + 9 + k_] = pf_acc[k_];   \
        for (int k_ = 0; k_ < 8; ++k_) A.stamps[((size_t)s * A.nc + (size_t)(p >> 6)) * PF_STAMP_W + 21 + k_] = pf_acc2[k_]; } } while (0)
#else
#define PF_PSTAMP(k) do {} while (0)
#define PF_PHWID() do {} while (0)
#define PF_PACC_STORE do {} while (0)
#endif

// the hand-off words: the address space stands in the pointer's type, here and nowhere else (w: the address of a member of the __shared__ PairLds)
template <class T>
__device__ __forceinline__ volatile __attribute__((address_space(3))) T* pair_word(T* w) { return (volatile __attribute__((address_space(3))) T*)w; }
template <class T>
__device__ __forceinline__ T pair_get(T* w) { return *pair_word(w); }
template <class T, class V>
__device__ __forceinline__ void pair_put(T* w, V v) { *pair_word(w) = (T)v; }

// a turn of a spin that found nothing: sleep; true when the wavefront has to leave (the partner gave up, or the row has taken PF_PAIR_TICKS)
__device__ __forceinline__ bool pair_spin_fail(PairLds& pl, unsigned long long t_row, Ctrl* c) {
    __builtin_amdgcn_s_sleep(1);
    if (pair_get(&pl.stall)) return true;
    if (wall_clock64() - t_row > PF_PAIR_TICKS) {
        pair_put(&pl.stall, 1);
        if (!c->err) c->err = ERR_PAIR_STALL;
        return true;
    }
    return false;
}

template <bool EXACT, class KA>
__device__ __forceinline__ void extend_pair_body(const KA& A, long long s, int nb, PipeRow PR, const SweepHeadR& H) {
    constexpr int NM = 4;
    static_assert(PF_BS == 2 * PF_PAIR_N && PF_EPAD <= PF_BS && 2 * PF_LUT_N / 4 <= PF_BS, "two tree and two weight wavefronts; one table entry a thread");
    extern __shared__ double smem[];
    __shared__ PairLds pl;
    __shared__ unsigned s_lut[2 * PF_LUT_N / 4];
    const int E_head = PF_HI(H, E), n_head = PF_HI(H, n), nc = PF_HI(H, nc);
    const long long Np_head = PF_HL(H, Np);
    double* sT = smem;
    double* sH = smem + PF_EPAD;
    double* sI = sH + PF_EPAD;
    double* sBH = sI + E_head;
    double* sBS = sBH + (PF_BIAS_MAX + 2);
    const int n = EXACT ? NM : n_head;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), pw = wave & 1;      // pw: the pair within the workgroup
    const bool tree = wave < 2;                                                     // wave-uniform: the roles are scalar branches
    const int idx = tid & (PF_PAIR_N - 1);
    const long long p = (long long)pf_bx() * PF_PAIR_N + idx;
    const bool active = p < Np_head;
    Ctrl* const cw = A.ctrl;
    if (tree) PF_PSTAMP(0);

    // ---- head: every request of the row's start, back to back.  The particle's doubles come from addresses chosen by role (a scalar
    // select, no branch to join behind): next_base / Ltree / ebuf for the tree, w_post / w_pilot / the slot's scan for the weights.  Heights, x_mark,
    // mark_limit and the record counter serve both (the closing record of the old slot is the weight wavefront's).
    RowPre pre;
    RTree<NM> t0;
    double o_a, o_b, o_c, o_xmark;
    int o_ml;
    unsigned o_widx, o_tab_end = 0;
    unsigned long long o_ctr;
    long long o_nres = 0; int o_bflag = 0, o_bgen = 0;
    double spec_sm[PF_PIPE_STAGE * 64 / PF_BS];
    double sg_start = 0.0, sg_len = 0.0, sgp_start = 0.0, sgp_len = 0.0;
    int sg_limit = 0, sg_state = 1;
    int sg_allele[NM];
#pragma unroll
    for (int i = 0; i < NM; ++i) sg_allele[i] = 0;
    double h_T = PF_INF, h_Hc = PF_INF, h_I = 0.0;
    unsigned h_lut = 0;
    bool use_lut = false;
    const int spec_lo = row_spec_lo(pf_bx() * (PF_PAIR_N / 64), PF_PAIR_N / 64, nc, PF_HI(H, flags));
    {
        const RowHeadPtrs hp = row_head_ptrs(H, PR.complete != 0, Np_head, n_head);
        if (PR.complete) row_head_decision(H, nc, Np_head, spec_lo, pre, o_nres, o_bflag, o_bgen, spec_sm);
        const long long q = active ? p : Np_head - 1;
        const auto pa = tree ? hp.next_base : hp.w_post;
        const auto pb = tree ? hp.Ltree : hp.w_pilot;
        const auto pc = tree ? PF_HP(H, ebuf) : PF_HP(H, scan1m);
#pragma unroll
        for (int r = 0; r < RTree<NM>::NI; ++r) {
            t0.S[r] = 0.0; t0.C0[r] = 0; t0.C1[r] = 0;
            if (r < n - 1) {
                t0.S[r] = hp.S[(size_t)r * Np_head + q];
                t0.C0[r] = hp.C[(size_t)(2 * r) * Np_head + q];
                t0.C1[r] = hp.C[(size_t)(2 * r + 1) * Np_head + q];
            }
        }
        o_a = pa[q]; o_b = pb[q]; o_c = pc[q]; o_xmark = hp.x_mark[q];
        o_ml = hp.mark_limit[q];
        o_widx = hp.widx[q];
        o_ctr = PF_HP(H, rng_ctr)[q];
        if (PR.draws) o_tab_end = (unsigned)PF_HP(H, dt_filled)[q];
        asm volatile("" ::: "memory");
        row_head_tables(H, E_head, h_T, h_Hc, h_I, use_lut, h_lut);
        asm volatile("" ::: "memory");
        row_head_segment<NM, EXACT>(H, s, n, sgp_start, sgp_len, sg_start, sg_len, sg_limit, sg_state, sg_allele);
        asm volatile("" ::: "memory");
    }
    // the hand-off words start the row at zero, behind the issue of the row's requests and in front of the row's first barrier: the first poll of
    // a weight wavefront (pub, fin, lkf, stall) and the first read of con by a tree wavefront lie behind at least one __syncthreads() on every
    // path, rows that complete nothing included, since either role runs tables_to_lds(); __syncthreads(); in front of them.  (The spin bound counts
    // from here.)
    const unsigned long long t_row = wall_clock64();
    PF_PHWID();
    if (tree) { pair_put(&pl.pub[pw][lane], 0); pair_put(&pl.fin[pw][lane], 0); pair_put(&pl.lkf[pw][lane], 0); }
    else pair_put(&pl.con[pw][lane], 0);
    if (tid == 0) pair_put(&pl.stall, 0);

    // ---- the decision on the row before, by all 256 threads as in the other form
    const PipeLds q = pipe_carve(sBS + (PF_BIAS_MAX + 1), A.nc);
    const int cur = __builtin_amdgcn_readfirstlane(PR.slot_out);
    const bool completing = PR.complete != 0;
    const int row_slot = PR.slot_prev;          // ring slot of the row being completed
    bool gather = false;
    double inv = 1.0, S1v = 0.0;
    RowDecision d = {};
    int G_end = 0, ev = 0;
    if (completing) {
        if (tree) PF_PSTAMP(1);
        pre.last1 = pf_arrive(pre.last1); o_nres = pf_arrive(o_nres); o_bflag = pf_arrive(o_bflag); o_bgen = pf_arrive(o_bgen);
        const long long n_res = o_nres + o_bflag;
        G_end = o_bgen + o_bflag;
        ev = (int)n_res;
#pragma unroll
        for (int k = 0; k < PF_PIPE_STAGE * 64 / PF_BS; ++k) q.stage[k * PF_BS + tid] = spec_sm[k];    // visible after decide_row's barriers
        d = decide_row<true>(A, q, row_slot, n_res, pre);
        if (tree) PF_PSTAMP(2);
        inv = d.inv; S1v = d.S1;
        gather = d.flag != 0;
        if (pf_bx() == 0 && tid == PF_PAIR_N) { cw->xr[row_slot].n_res = n_res; cw->xr[row_slot].gen = G_end; cw->xr[row_slot].flag = d.flag; }
    }
    // ---- resampling row: the two searches side by side, between the barriers the search has
    const double dn = (double)A.Np;
    const double* sm = A.rg_scan1m + (size_t)(row_slot < 0 ? 0 : row_slot) * A.Np;
    const double lhs = ((double)p + d.u) * d.S1;
    int pch = 0, stage_lo = 0, nst = 0;
    if (gather) {
        if (tree) {
            if (active) pch = row_parent_chunk(q, A.nc, lhs, dn);
            int cmin = active ? pch : 0x7fffffff, cmax = active ? pch : -1;
            wave_minmax(cmin, cmax);
            if (lane == 0) { q.wint[pw] = cmin; q.wint[PF_BS / 64 + pw] = cmax; }
        } else {
            // the offspring offsets of the workgroup's particles: q.slo[i + 1] ends the offspring of its particle i, q.slo[0] starts those of the first
            const double invS1 = 1.0 / d.S1;
            if (active) {
                const int ch_own = (int)(p >> 6);
                const double w = pipe_chunk_offset(q, ch_own) + o_c;
                const double v_own = q.pmx[ch_own] > w ? q.pmx[ch_own] : w;          // largest pilot prefix sum up to particle p
                q.slo[idx + 1] = p + 1 < A.Np ? pipe_lo_from(v_own, dn, A.Np, d.S1, invS1, d.u) : (int)A.Np;
                if (idx == 0) q.slo[0] = p > 0 ? pipe_lo_from(q.pmx[ch_own], dn, A.Np, d.S1, invS1, d.u) : 0;
            }
        }
        __syncthreads();
        row_stage_parents<PF_PAIR_N / 64>(A, q, sm, spec_lo, stage_lo, nst);
    }
    // what either role does right in front of the last barrier of the row: the tables of the update loop go to LDS, the end of the row before
    double pos_prev = 0.0;
    auto tables_to_lds = [&]() {
        if (tid < PF_EPAD) {
            sT[tid] = h_T; sH[tid] = h_Hc;
            if (tid < E_head) sI[tid] = h_I;
        }
        if (use_lut && tid < 2 * PF_LUT_N / 4) s_lut[tid] = h_lut;
        if (completing && s > PF_HL(H, s_begin)) {
            const double e = pf_arrive(sgp_start) + pf_arrive(sgp_len), Lq = A.L;       // sweep_seg_pos of row s - 1
            pos_prev = e < Lq ? e : Lq;
        }
    };
    const double v_mu = in_vgpr(A.mu);
    const bool do_extend = PR.extend != 0;

    if (tree) {
        // ================================================================= tree wavefront
        long long a = p;
        bool first_copy = true, closes = false;
        if (gather && active) {
            row_parent_in_chunk(A, q, sm, pch, stage_lo, nst, lhs, dn, p, d, a, first_copy, []() {});
            pl.parent[idx] = (int)a;
            closes = q.slo[idx + 1] > q.slo[idx];
        }
        RTree<NM> t = t0;
        double next_base = o_a, x_mark = o_xmark, Ltree = o_b;
        int mark_limit = o_ml;
        if (gather && active) {            // the parent's tree, requested at once
            const DState from = state_slot(A, row_slot);
#pragma unroll
            for (int r = 0; r < RTree<NM>::NI; ++r)
                if (r < n - 1) {
                    t.S[r] = from.S[(size_t)r * A.Np + a];
                    t.C0[r] = from.C[(size_t)(2 * r) * A.Np + a];
                    t.C1[r] = from.C[(size_t)(2 * r + 1) * A.Np + a];
                }
            next_base = from.next_base[a];
            mark_limit = from.mark_limit[a];
            Ltree = from.Ltree[a];
        }
        tables_to_lds();
        __syncthreads();
        PF_PSTAMP(3);
        RCtx cx;
        DStore ds;
        const double v_L = in_vgpr(A.L), v_rho = in_vgpr(A.rho);
        unsigned widx = o_widx, npub = 0;
        int limit = 0;
        double extend_to = 0.0;
        RowMasks rm;
        bool failed = false;
        row_segment_arrive<NM, EXACT>(do_extend, n, sg_start, sg_len, sg_limit, sg_state, sg_allele);
        if (active) {
            row_ctx<false, false, true>(cx, A, sT, sI, sH, sBH, sBS, n, p, v_L, v_mu, v_rho, use_lut, s_lut, PR.draws, o_tab_end);
            cx.vbc = nullptr;              // (run_sweep_split keeps vb_coal handles on the other form)
            cx.Ltree = Ltree;
            cx.ctr = o_ctr; cx.ebuf = o_c;
            r_draws_prefetch(cx);
            if (gather) {
                if (closes) ++widx;        // the closing record of the old slot (the weight wavefront writes it) comes first
                // (here and not beside that record: the check of the record ring at the row's end may read this very entry back, which one
                // wavefront orders and two do not)
                A.gstart[(size_t)((G_end + 1) % A.Gcap) * A.Np + p] = widx;
                x_mark = pos_prev;
                if (!first_copy && pos_prev < v_L) {
                    next_base = r_sample_next_base<false>(cx, pos_prev);     // pc.cpp:357-368
                    r_draws_prefetch(cx);           // the counter moved: the request above is stale
                }
            }
            PF_PSTAMP(4);
            double seg_end = 0.0;
            if (do_extend) { seg_end = sg_start + sg_len; limit = sg_limit; }
            extend_to = seg_end < v_L ? seg_end : v_L;
            if (do_extend) rm = row_masks<NM>(n, [&](int i) { return sg_allele[i]; });
            int leaf_status = 0;
            if (rm.missing == 0) leaf_status = 1;
            if (rm.missing == n) leaf_status = -1;
            double updated_to = completing ? pos_prev : A.ctrl->cur_pos;
            if (!do_extend) updated_to = extend_to;             // completion only: the loop below does not run
            double B;
            if (leaf_status == -1) B = 0;
            else if (leaf_status == 1) B = cx.Ltree;
            else B = r_tracked_len(t, n, rm.present);
            double w_none_a = 1.0, w_none_b = 1.0;              // (the weights are the partner's)
            unsigned con_seen = 0;
            PF_ACC_DECL;
            while (updated_to < extend_to) {
                PF_TICK(tk0);
                const double new_to = extend_to < next_base ? extend_to : next_base;
                // the pass's entry for the weight lane; a lane a whole ring ahead waits for its partner
                while (npub - con_seen >= PF_PAIR_DEPTH) {
                    con_seen = pair_get(&pl.con[pw][lane]);
                    if (npub - con_seen >= PF_PAIR_DEPTH && pair_spin_fail(pl, t_row, cw)) { failed = true; break; }
                }
                if (failed) break;
                pair_put(&pl.ring[pw][npub & (PF_PAIR_DEPTH - 1)][0][lane], B);              // entry, then count
                pair_put(&pl.ring[pw][npub & (PF_PAIR_DEPTH - 1)][1][lane], new_to - updated_to);
                ++npub;
                pair_put(&pl.pub[pw][lane], npub);
                updated_to = new_to;
                PF_TICK(tk1);
                PF_ACC(0, tk0, tk1);
                if (updated_to < extend_to)
                    row_update_trip<NM, false, EXACT, false, true>(A, cx, t, ds, p, n, limit, leaf_status, rm.present, updated_to, widx, x_mark, mark_limit, next_base, B,
                                                                   w_none_a, w_none_b, sBH, sBS PF_ACC_ARGS);
            }
            PF_PACC_STORE;
        }
        if (__any(failed)) return;
        pair_put(&pl.fin[pw][lane], npub + 1);
        PF_PSTAMP(5);
        // the site likelihood needs the tree: it goes to the weight lane through LDS
        unsigned lflag = 1;
        if (do_extend && sg_state == 0) {
            if (active) pair_put(&pl.lik[pw][lane], row_site_lik<NM>(t, n, v_mu, rm.one, rm.zero, rm.two, A.flags & 2, A.flags & 1));
            lflag = 2;
        }
        pair_put(&pl.lkf[pw][lane], lflag);
        PF_PSTAMP(6);
        if (active) {
            const KA& A1 = pf_reopen(A);
            const DState st1 = state_slot(A1, cur);
            row_store_tree<NM>(st1, (size_t)A1.Np, p, n, t);
            row_store_chain(A1, st1, p, next_base, x_mark, mark_limit, cx);
            row_store_counters(A1, PR, cur, p, cx.ctr, widx, do_extend);
        }
        PF_PSTAMP(7);
        PF_PSTAMP(8);
    } else {
        // ================================================================= weight wavefront
        tables_to_lds();
        __syncthreads();
        double w_post = 0.0, w_pilot = 0.0;
        bool closes = false;
        if (active) {
            if (gather) {
                const int a = pl.parent[idx];
                const DState from = state_slot(A, row_slot);
                w_post = from.w_post[a];           // the parent's weights, requested first
                w_pilot = from.w_pilot[a];
                // the old slot p: offspring table, closing record, the trace of parents
                const int lo_p = q.slo[idx], lo_p1 = q.slo[idx + 1];
                int* lo_tab = A.lo + (size_t)(G_end % A.Gcap) * (A.Np + 1);
                lo_tab[p] = lo_p;
                if (p == A.Np - 1) lo_tab[A.Np] = (int)A.Np;
                closes = lo_p1 > lo_p;
                if (closes) {
                    double* rec = rec_ptr(A, p, o_widx);
                    row_close_record(rec, o_xmark, pos_prev, o_ml, n);
#pragma unroll
                    for (int r = 0; r < RTree<NM>::NI; ++r) if (r < n - 1) rec[5 + r] = t0.S[r];
                }
                if (ev < A.max_trace_events) A.ev_parents[(size_t)ev * A.Np + p] = a;
                row_copy_weights(w_post, w_pilot, inv, S1v, (double)A.Np);
            } else {
                w_post = o_a; w_pilot = o_b;
                if (completing) { w_post *= inv; w_pilot *= inv; }      // normalize_probability, pc.cpp:435-437
            }
        }
        if (gather) {
            // survivors per wavefront (A.blk_gran = 4; the ledger positions the run list of the ending generation with them); the last
            // workgroup also clears the entries of the block's wavefronts that no workgroup owns
            const unsigned long long bal = __ballot(active && closes);
            if (lane == 0) {
                int* bc = A.rg_blkcnt + (size_t)row_slot * gridDim_particles(A) * (PF_BS / 64);
                const int e = pf_bx() * (PF_PAIR_N / 64) + pw;
                bc[e] = __popcll(bal);
                if (pf_bx() == nb - 1 && e + 2 < gridDim_particles(A) * (PF_BS / 64)) bc[e + 2] = 0;
            }
        }
        PF_PSTAMP(29);
        // the factors of the update loop as the tree lane produces them
        unsigned consumed = 0;
        for (;;) {
            const unsigned finv = pair_get(&pl.fin[pw][lane]);           // (before pub: once the loop has ended, pub is final)
            const unsigned pubv = pair_get(&pl.pub[pw][lane]);
            const bool have = pubv != consumed;
            if (have) {
                const double eB = pair_get(&pl.ring[pw][consumed & (PF_PAIR_DEPTH - 1)][0][lane]);      // count, then entry; the entry's reads, then con
                const double edt = pair_get(&pl.ring[pw][consumed & (PF_PAIR_DEPTH - 1)][1][lane]);
                const double f = fastexp(-v_mu * eB * edt);
                w_post *= f;
                w_pilot *= f;
                ++consumed;
                pair_put(&pl.con[pw][lane], consumed);
            }
            if (__all(finv != 0 && consumed == finv - 1)) break;
            if (!__any(have) && pair_spin_fail(pl, t_row, cw)) return;
        }
        for (;;) {
            const unsigned lf = pair_get(&pl.lkf[pw][lane]);
            if (__all(lf != 0)) {
                if (lf == 2 && active) { const double lik = pair_get(&pl.lik[pw][lane]); w_post *= lik; w_pilot *= lik; }
                break;
            }
            if (pair_spin_fail(pl, t_row, cw)) return;
        }
        PF_PSTAMP(30);
        const KA& A2 = pf_reopen(A);
        if (active) {
            const DState st1 = state_slot(A2, cur);
            st1.w_post[p] = w_post;
            st1.w_pilot[p] = w_pilot;
        }
        const RowScans rs = row_scans(w_post, w_pilot, lane);
        row_scans_store(A2, cur, p, active, lane, rs);
        PF_PSTAMP(31);
    }
}
