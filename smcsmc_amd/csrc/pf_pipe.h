// smcsmc_amd/csrc/pf_pipe.h -- what the row pipeline's kernels share across translation units (pf_hip.hip: k_pipe, k_sweep and
// the bookkeeping / ledger / count roles, k_sweep_xl through pf_lds_pipe.h; pf_mp.hip: the extend role of the structured models): the decision on a finished
// row taken redundantly by every workgroup, the offspring offsets in closed form, the plan of a step, the per-chunk table
// of k_sweep.  Workgroup size is a template parameter here (PF_BS differs between the two units).
#pragma once
#include <cstddef>
#include <cstring>
#include <type_traits>

#include "pf_device.h"
#include "pf_types.h"

#define PF_PIPE_BS 256          // largest workgroup that runs the pipeline's prologue (sizes the LDS carve-out)

// A fresh, opaque handle on the same argument block in the constant address space: loads through it cannot be merged with
// earlier ones nor hoisted above this point, so what a phase of a long kernel needs from the block is loaded in that phase
// instead of being held in (and spilled from) scalar registers across the phases before it.  The by-value form of the
// block (kernels that take KArgs as an argument) is returned as it is.
__device__ __forceinline__ KArgsC& pf_reopen(KArgsC& A) { KArgsC* q = &A; asm volatile("" : "+s"(q)); return *q; }
__device__ __forceinline__ const KArgs& pf_reopen(const KArgs& A) { return A; }

// ---- decision on a finished row, made redundantly by every workgroup that needs it (single-launch pipeline) --------
// normalize_probability (pc.cpp:420-438) and the ESS test of resample (pc.cpp:247-283) from the per-wavefront partials
// the row's extend workgroups left in ring slot `slot`: the level-2 / level-3 part of the canonical radix-64 reduction,
// operation for operation what k_decide does, so T, S1, ESS, the flag and the uniform are bit-identical everywhere.
#define PF_PIPE_STAGE 16        // wavefronts of pilot scans staged per workgroup for the parent search
struct RowDecision { double T, S1, S2, ess, inv, u; int flag; };
struct PipeLds {                // carved from the dynamic LDS of k_pipe behind the epoch tables
    double* l2s;                // [ncpad] level-2 inclusive scan of the per-wavefront pilot totals
    double* pmx;                // [ncpad + 1] pmx[ch] = largest pilot prefix sum before wavefront ch (pmx[ch + 1]: up to its end)
    double* l2_post; double* l2_sq; double* l2_tot;   // [64] each
    double* wredd;              // [PF_PIPE_BS / 64]
    double* stage;              // [PF_PIPE_STAGE * 64]
    int* slo;                   // [PF_PIPE_BS]
    int* wint;                  // [3 * PF_PIPE_BS / 64]
};
__host__ __device__ inline size_t pipe_lds_doubles(int nc) {
    const size_t ncpad = ((size_t)nc + 63) / 64 * 64;
    return ncpad + (ncpad + 1) + 3 * 64 + PF_PIPE_BS / 64 + (size_t)PF_PIPE_STAGE * 64 + (PF_PIPE_BS + 3 * (PF_PIPE_BS / 64) + 1) / 2 + 2;
}
__device__ __forceinline__ PipeLds pipe_carve(double* base, int nc) {
    const size_t ncpad = ((size_t)nc + 63) / 64 * 64;
    PipeLds q;
    q.l2s = base; base += ncpad;
    q.pmx = base; base += ncpad + 1;
    q.l2_post = base; base += 64; q.l2_sq = base; base += 64; q.l2_tot = base; base += 64;
    q.wredd = base; base += PF_PIPE_BS / 64;
    q.stage = base; base += (size_t)PF_PIPE_STAGE * 64;
    q.slo = (int*)base; q.wint = q.slo + PF_PIPE_BS;
    return q;
}
__device__ __forceinline__ double pipe_chunk_offset(const PipeLds& q, int ch) {
    double run = 0.0;
    const int gq = ch / 64;
    for (int g = 0; g < gq; ++g) run = run + q.l2_tot[g];
    double off = (ch % 64 == 0) ? 0.0 : q.l2s[ch - 1];
    return run + off;
}
// every thread of the workgroup calls this (it contains barriers); WANT_TABLE: also the prefix maxima the offspring
// table / parent search need (only computed when the row resamples)
// the partials a thread needs first, requested before anything else so that their memory round trip overlaps the
// particle's own loads (what the previous launch wrote comes from another XCD's L2: about a microsecond)
// (the second set: a workgroup of BS threads reduces up to 2 BS wavefront partials -- the structured models' 64-particle
// workgroups at Np = 20 000 have 313 for 256 threads -- and the second pass of a thread would otherwise start with a
// round trip of its own; vm / vm2 are the two consecutive entries a thread of the prefix-maxima pass owns then)
struct RowPre { double vp = 0.0, vs = 0.0, vl = 0.0, vm = 0.0, last1 = 0.0, vp2 = 0.0, vs2 = 0.0, vl2 = 0.0, vm2 = 0.0; bool have = false; };
template <int BS = PF_PIPE_BS, class KA>
__device__ __forceinline__ RowPre row_preload(const KA& A, int slot) {
    const int nc = A.nc, ch = threadIdx.x;
    const int perc = (nc + BS - 1) / BS;
    RowPre r;
    r.have = true;
    if (ch < nc) {
        r.vp = A.rg_cpost[(size_t)slot * nc + ch];
        r.vs = A.rg_csq[(size_t)slot * nc + ch];
        r.vl = A.rg_cpil[(size_t)slot * nc + ch];
    }
    if (ch + BS < nc) {
        r.vp2 = A.rg_cpost[(size_t)slot * nc + ch + BS];
        r.vs2 = A.rg_csq[(size_t)slot * nc + ch + BS];
        r.vl2 = A.rg_cpil[(size_t)slot * nc + ch + BS];
    }
    // only a resampling row uses them (the prefix maxima), but then a round trip earlier
    if (perc == 1) { if (ch < nc) r.vm = A.rg_cmx1[(size_t)slot * nc + ch]; }
    else if (perc == 2) {
        if (2 * ch < nc) r.vm = A.rg_cmx1[(size_t)slot * nc + 2 * ch];
        if (2 * ch + 1 < nc) r.vm2 = A.rg_cmx1[(size_t)slot * nc + 2 * ch + 1];
    }
    r.last1 = A.ctrl->last1[slot];
    return r;
}
template <bool WANT_TABLE, int BS = PF_PIPE_BS, class KA>
__device__ __forceinline__ RowDecision decide_row(const KA& A, const PipeLds& q, int slot, long long n_res, RowPre pre = RowPre()) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = BS / 64;
    const int nc = A.nc;
    const int ng = (nc + 63) / 64;
    const double* cpost = A.rg_cpost + (size_t)slot * nc;
    const double* csq = A.rg_csq + (size_t)slot * nc;
    const double* cpil = A.rg_cpil + (size_t)slot * nc;
    const double* cmx1 = A.rg_cmx1 + (size_t)slot * nc;
    const double last_scan1 = pre.have ? pre.last1 : A.ctrl->last1[slot];
    for (int g = wave; g < ng; g += nwaves) {
        int ch = g * 64 + lane;
        const bool first = pre.have && g == wave, second = pre.have && g == wave + nwaves;
        double vp = first ? pre.vp : (second ? pre.vp2 : (ch < nc ? cpost[ch] : 0.0));
        double vs = first ? pre.vs : (second ? pre.vs2 : (ch < nc ? csq[ch] : 0.0));
        double vl = first ? pre.vl : (second ? pre.vl2 : (ch < nc ? cpil[ch] : 0.0));
        double rp = wave_tree_sum(vp);
        double rs = wave_tree_sum(vs);
        double sc = wave_hs_scan(vl, lane);
        if (ch < nc) q.l2s[ch] = sc;
        if (lane == 63) { q.l2_post[g] = rp; q.l2_sq[g] = rs; q.l2_tot[g] = sc; }
    }
    __syncthreads();
    RowDecision d;
    {
        double vp = lane < ng ? q.l2_post[lane] : 0.0;
        double vs = lane < ng ? q.l2_sq[lane] : 0.0;
        d.T = wave_tree_sum(vp);
        d.S2 = wave_tree_sum(vs);
    }
    d.S1 = pipe_chunk_offset(q, nc - 1) + last_scan1;   // inclusive scan at the last particle (= oracle incl[N-1])
    d.ess = (d.S1 * d.S1) / d.S2;
    d.flag = (d.ess < A.ess_threshold - 1e-6) ? 1 : 0;
    d.inv = 1.0 / d.T;
    d.u = d.flag ? philox_uniform(A.seed, 0xFFFFFFFFu, 1, (unsigned long long)n_res) : 0.0;
    if (WANT_TABLE && d.flag) {
        // pmx[ch] = max over wavefronts c' < ch of (chunk_off[c'] + mx1[c']): the running maximum that makes the offspring
        // table monotone is taken on the prefix sums (lo_raw is monotone in its argument), as in k_decide
        const int perc = (nc + BS - 1) / BS;
        const int c0 = tid * perc, c1 = c0 + perc < nc ? c0 + perc : nc;
        double run = 0.0;
        // one wavefront per thread (nc <= BS): thread tid's entry is the one row_preload asked for
        const bool pre_mx = pre.have && perc <= 2;
        const double pre_vm = pre.vm, pre_vm2 = pre.vm2;
        for (int ch = c0; ch < c1; ++ch) { double vch = pipe_chunk_offset(q, ch) + (pre_mx ? (ch == c0 ? pre_vm : pre_vm2) : cmx1[ch]); run = vch > run ? vch : run; }
        double scd = wave_max_scan_d(run, lane);
        if (lane == 63) q.wredd[wave] = scd;
        __syncthreads();
        double pre = 0.0;
        for (int w = 0; w < wave; ++w) pre = q.wredd[w] > pre ? q.wredd[w] : pre;
        double before = wave_prev_lane(scd, scd);
        if (lane > 0) pre = before > pre ? before : pre;
        run = pre;
        for (int ch = c0; ch < c1; ++ch) {
            q.pmx[ch] = run;
            double vch = pipe_chunk_offset(q, ch) + (pre_mx ? (ch == c0 ? pre_vm : pre_vm2) : cmx1[ch]);
            run = vch > run ? vch : run;
        }
        if (c1 == nc && c0 < c1) q.pmx[nc] = run;
        __syncthreads();
    }
    return d;
}
// final offspring offset from the (running-maximum) pilot prefix sum v: #{ j in [0,N) : (j+u) * S1 < N * v }  (pc.cpp:491
// scaled by N*S1: no division), guess plus exact predicate correction -- the arithmetic of k_decide's lo_at
__device__ __forceinline__ int pipe_lo_from(double v, double dn, long long Np, double S1, double invS1, double u) {
    double rhs = dn * v;
    double guess = floor(rhs * invS1 - u);
    long long g = guess < 0 ? 0 : (guess > dn ? Np : (long long)guess);
    while (g > 0 && !((((double)(g - 1)) + u) * S1 < rhs)) --g;
    while (g < Np && ((((double)g) + u) * S1 < rhs)) ++g;
    return (int)g;
}

// what the single-launch pipeline tells the extend workgroups about their row
struct PipeRow {
    int complete;          // the previous row has to be completed on load (0 for the first row of a pf_run call)
    int extend;            // 0: completion only (flush at the end of a pf_run call)
    int slot_prev;         // state ring slot to read (the general double-buffer index when !complete)
    int slot_out;          // slot to write
    double pos_prev;       // end of the previous row
    int draws;             // the draw table is kept up by this launch sequence (k_sweep): 1 + parity of the row, 0: no table
    int ahead;             // the extend role is a launch of its own and runs up to PF_RING - 2 rows ahead of the other roles
};


struct PipeLaunch {
    PipeRow row;
    int nb;                // extend workgroups of this launch (0: a launch of the bookkeeping / ledger / count roles only)
    int nblk;              // particle blocks of 256 (what the ledger's new run list is built by)
    int b_slot;            // ring slot of the row whose bookkeeping is due (-1: none)
    long long b_row;       // its row index (traces)
    double b_pos;          // its end position
    int b_set_cur;         // >= 0: the general kernels take over after this launch, with this state slot
    int lc_slot;           // ring slot of the row whose ledger upkeep and counts are due (-1: none)
    int live_slot;         // newest complete slot of the per-slot record counters (ring-overwrite check)
    int nL;                // ledger workgroups
    int ncw;               // count workgroups per epoch
    int nT;                // workgroups that keep up the draw table (k_sweep only)
    int ahead;             // as PipeRow::ahead: the rings need PF_RING entries of headroom
    int workers;           // > 0: the ledger and count work of the step is dealt out among this many workgroups (Ctrl::wq)
};


struct SweepChunk {
    KArgs A;
    long long s_begin;             // first row of this call
    long long s_last;              // last row extended by this call; steps s_last + 1 and s_last + 2 flush
    double counted_to[PF_EMAX];    // window state (CountModel::counted_to) at the start of the call
    int no_count;
    int nL_full;                   // ledger workgroups per step
    int ncw;                       // count workgroups per epoch
    int nblk;                      // particle blocks of 256
    int nT;                        // draw-table workgroups per step (0: no table)
    int split;                     // 2: the ledger and count roles are a launch of their own beside the extend, bookkeeping and draw roles
                                   // (run_sweep_split); 1: the extend role alone is a launch of its own and runs ahead of the other roles (run_sweep_x
                                   // for one population on the LDS tree); 0: one launch per step (run_sweep), or the structured models' two (run_sweep_x)
    unsigned long long* trace;     // pf_set_wg_trace: four words per workgroup of steps [trace_t0, trace_t0 + trace_n) (k_sweep4t only)
    int trace_t0, trace_n, trace_stride;
    int workers;                   // pf_params.count_workers (PipeLaunch::workers)
};
typedef const __attribute__((address_space(4))) SweepChunk SweepChunkC;

// The row header of the headline row kernels (k_sweep4, k_sweep4p, k_sweep4q, k_sweep4t): what the head of an extend workgroup reads, resolved on the
// host once per call and uploaded in front of the chunk table (sweep_head_of).  Every address the head loads from is a function of the chunk's device pointers (fixed for the life of the handle)
// and of the ring slots of the step, and those are (s_begin + t) mod PF_RING: one entry per chunk and ring phase, PF_RING entries a chunk,
// entry t & (PF_RING - 1) for step t.  slot_prev = (s_begin + t - 1) & (PF_RING - 1) is the row the step completes and continues from,
// and every pointer into a ring below already points at that slot.  An extend wavefront loads its entry in one batch behind the
// kernel arguments (five lines of 64 bytes, what is used first in the first), waits once, derives the plan of the step from t and
// the entry without another memory access and requests everything the head needs back to back.  (The first step of a call continues
// from the slot Ctrl::cur names, which only the device knows: the kernel moves the eight state pointers by the difference of the
// slots, sweep_head_first.)  No arrays of pointers: a run-time index into one would put the entry on the stack.
struct SweepHead {
    // line 0: the plan of the step and the bounds of the requests
    long long s_begin, s_last, Np;
    int nc, n, E, flags, nT, split, nblk, no_count, P, slot_prev;
    // line 1: the decision on the row in slot_prev (per-wavefront partials [nc], the scan at the last particle, the note of the extend role
    // of the step before: Ctrl::xr of slot_prev - 1), the pilot scans [Np] the parent search stages, the slots' record counters
    const double* cpost; const double* csq; const double* cpil; const double* cmx1;
    const double* last1; const Ctrl::ExtendNote* xr_before; const double* scan1m; const unsigned* rg_widx;
    // line 2: the particle's own state in slot_prev
    const double* S; const int8_t* C; const double* w_post; const double* w_pilot;
    const double* next_base; const double* x_mark; const int* mark_limit; const double* Ltree;
    // line 3: what a slot owns whatever the row (dt_filled: of the parity of the row before), the row's segment
    const unsigned* widx; const unsigned long long* rng_ctr; const double* ebuf; const unsigned long long* dt_filled;
    const double* seg_start; const double* seg_len; const int* seg_limit; const int8_t* seg_state;
    // line 4: the alleles, the epoch tables and the bucket table that go to LDS
    const int8_t* seg_alleles; const double* T; const double* Hc; const double* inv2N;
    const unsigned char* lut; const Ctrl* ctrl; const void* pad_[2];
};
static_assert(sizeof(SweepHead) == 5 * 64, "SweepHead: five lines of sixteen words");
typedef const __attribute__((address_space(4))) SweepHead SweepHeadC;
// Where the entries are: in front of the chunk table, in the same allocation, chunk 0's PF_RING entries last -- `table` is the address of
// the chunk table (what the kernels are given), so an entry's address takes nothing from memory.
template <class H>
__host__ __device__ inline H* sweep_head_of(H* table, int chunk, long long t) {
    return table - ((size_t)chunk + 1) * PF_RING + (size_t)(t & (PF_RING - 1));
}

// An entry in scalar registers: its five lines requested together (five s_load_dwordx16 behind one address) and waited for once --
// left to itself the compiler fetches every field where it is first used, a round trip each.  Fields are read with PF_HP (pointers),
// PF_HL (64-bit integers) and PF_HI (32-bit integers) by their names in SweepHead; the words are compile-time positions in the lines.
typedef int pf_line16 __attribute__((ext_vector_type(16)));
struct SweepHeadR {
    pf_line16 l0, l1, l2, l3, l4;
    __device__ __forceinline__ SweepHeadR() : l0(0), l1(0), l2(0), l3(0), l4(0) {}
    __device__ __forceinline__ explicit SweepHeadR(SweepHeadC* e) {
        typedef const __attribute__((address_space(4))) pf_line16 LineC;
        LineC* q = (LineC*)e;
        l0 = q[0]; l1 = q[1]; l2 = q[2]; l3 = q[3]; l4 = q[4];
        asm volatile("" : "+s"(l0), "+s"(l1), "+s"(l2), "+s"(l3), "+s"(l4));
    }
    template <int OFF> __device__ __forceinline__ unsigned word() const {
        static_assert(OFF % 4 == 0 && OFF >= 0 && OFF < (int)sizeof(SweepHead), "a word of the entry");
        constexpr int L = OFF / 64, K = (OFF % 64) / 4;
        if constexpr (L == 0) return (unsigned)l0[K];
        else if constexpr (L == 1) return (unsigned)l1[K];
        else if constexpr (L == 2) return (unsigned)l2[K];
        else if constexpr (L == 3) return (unsigned)l3[K];
        else return (unsigned)l4[K];
    }
    template <int OFF> __device__ __forceinline__ unsigned long long dword() const {
        return ((unsigned long long)word<OFF + 4>() << 32) | (unsigned long long)word<OFF>();
    }
};
// (pointers come out in the global address space: one put together from two words would otherwise be a flat pointer, whose loads count
// against both wait counters)
#define PF_HP(R, f) ((__attribute__((address_space(1))) std::remove_pointer_t<decltype(SweepHead::f)>*)(R).template dword<(int)offsetof(SweepHead, f)>())
#define PF_HL(R, f) ((long long)(R).template dword<(int)offsetof(SweepHead, f)>())
#define PF_HI(R, f) ((int)(R).template word<(int)offsetof(SweepHead, f)>())

// entry `phase` of chunk A for a call that starts at row s_begin (host; SweepFrame::table)
inline SweepHead sweep_head_entry(const KArgs& A, const SweepChunk& ch, int phase) {
    SweepHead H;
    memset(&H, 0, sizeof(H));
    const size_t sp = (size_t)((ch.s_begin + phase + PF_RING - 1) & (PF_RING - 1)), Np = (size_t)A.Np, nc = (size_t)A.nc;
    H.s_begin = ch.s_begin; H.s_last = ch.s_last; H.Np = A.Np;
    H.nc = A.nc; H.n = A.n; H.E = A.E; H.flags = A.flags; H.nT = ch.nT; H.split = ch.split; H.nblk = ch.nblk; H.no_count = ch.no_count; H.P = A.P;
    H.slot_prev = (int)sp;
    H.cpost = A.rg_cpost + sp * nc; H.csq = A.rg_csq + sp * nc; H.cpil = A.rg_cpil + sp * nc; H.cmx1 = A.rg_cmx1 + sp * nc;
    H.last1 = &A.ctrl->last1[sp]; H.xr_before = &A.ctrl->xr[(sp + PF_RING - 1) & (PF_RING - 1)];
    H.scan1m = A.rg_scan1m + sp * Np; H.rg_widx = A.rg_widx + sp * Np;
    const DState st = state_slot(A, (int)sp);
    H.S = st.S; H.C = st.C; H.w_post = st.w_post; H.w_pilot = st.w_pilot; H.next_base = st.next_base; H.x_mark = st.x_mark;
    H.mark_limit = st.mark_limit; H.Ltree = st.Ltree;
    H.widx = A.widx; H.rng_ctr = A.rng_ctr; H.ebuf = A.ebuf;
    H.dt_filled = A.dt_filled ? A.dt_filled + (size_t)((ch.s_begin + phase + 1) & 1) * Np : nullptr;
    H.seg_start = A.seg_start; H.seg_len = A.seg_len; H.seg_limit = A.seg_limit; H.seg_state = A.seg_state; H.seg_alleles = A.seg_alleles;
    H.T = A.T; H.Hc = A.Hc; H.inv2N = A.inv2N; H.lut = A.lut; H.ctrl = A.ctrl;
    return H;
}

// The pacing of the two streams of a sweep through the ring (host; SweepFrame, pf_run.h).  The extend launch of step t overwrites the slot of
// row t - PF_RING, which the counts read in step t - PF_RING + 2: one wait every eight steps, for the second launch of seven steps ago, covers the
// eight steps that follow (t + 7 - 14 <= t - 7).  sweep_ring_awaited: the step whose second launch the extend launch of step t waits for (-1: none).
// sweep_blc_awaited: whether anything in a call of `steps` steps waits for the second launch of step u -- the ring wait of step u + 7, or the end
// of the call.  The second says what the first says, by calling it: a launch that signals only where the second holds records every entry the
// first makes a wait read (tests/test_count_chain_cpu.py plays the schedule through).
inline long long sweep_ring_awaited(long long t) {
    static_assert(PF_RING == 16, "the wait schedule is written for sixteen ring slots");
    return (t >= 8 && (t & 7) == 0) ? t - 7 : -1;
}
inline bool sweep_blc_awaited(long long u, long long steps) {
    return (u + 7 < steps && sweep_ring_awaited(u + 7) == u) || u == steps - 1;
}

template <class KA>
__device__ __forceinline__ double sweep_seg_pos(const KA& A, long long s) {       // seg_pos() of the host
    const double e = A.seg_start[s] + A.seg_len[s];
    return e < A.L ? e : A.L;
}

// what run_pipeline's `launch` lambda computes on the host, from the step's row alone
// (ROW_END = false: a launch without the extend and bookkeeping roles -- k_sweep_blc4 -- does not ask for the end of row s - 1, two dependent
// scalar round trips through the segment table in front of every workgroup's first request)
template <bool ROW_END = true>
__device__ __forceinline__ bool sweep_plan(SweepChunkC& ch, long long s, int nb, PipeLaunch& PL) {
    const long long s_begin = ch.s_begin, s_last = ch.s_last;
    if (s_last < s_begin || s > s_last + 2) return false;
    const bool extend = s <= s_last, flush1 = s == s_last + 1;
    const bool have_b = extend ? (s > s_begin) : flush1;
    const bool have_lc = extend ? (s > s_begin + 1) : (flush1 ? (s_last - 1 >= s_begin) : true);
    PL.nb = nb; PL.nblk = ch.nblk;
    PL.row.extend = extend ? 1 : 0;
    PL.row.complete = ((extend && s > s_begin) || flush1) ? 1 : 0;
    PL.row.slot_prev = PL.row.complete ? (int)((s - 1) & (PF_RING - 1)) : -1;
    PL.row.slot_out = (int)(s & (PF_RING - 1));
    // only a step that completes a row needs its end; on the second flush step row s - 1 = s_last + 1 may lie past the table
    PL.row.pos_prev = (ROW_END && PL.row.complete && s > s_begin) ? sweep_seg_pos(ch.A, s - 1) : 0.0;
    PL.row.draws = ch.nT > 0 ? 1 + (int)(s & 1) : 0;
    PL.ahead = PL.row.ahead = (ch.split || ch.A.P > 1) ? 1 : 0;
    PL.nT = extend ? ch.nT : 0;
    PL.b_slot = have_b ? (int)((s - 1) & (PF_RING - 1)) : -1;
    PL.b_row = s - 1;
    PL.b_pos = (ROW_END && have_b) ? sweep_seg_pos(ch.A, s - 1) : 0.0;
    PL.b_set_cur = flush1 ? (int)((s_last + 1) & (PF_RING - 1)) : -1;
    PL.lc_slot = (have_lc && !ch.no_count) ? (int)((s - 2) & (PF_RING - 1)) : -1;
    PL.live_slot = (int)((s - 1) & (PF_RING - 1));
    PL.nL = PL.lc_slot >= 0 ? ch.nL_full : 0;
    PL.ncw = ch.ncw;
    PL.workers = ch.workers;
    return true;
}

