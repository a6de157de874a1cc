// smcsmc_amd/csrc/pf_hip.hip -- gfx950 kernels + C-ABI (include/smcsmc_pf.h) of the smcsmc particle filter.
//
// One particle per lane.  Per genome segment the stream carries:
//   k_extend   [grid]   ForestState::extend_ARG + site likelihood, per-wavefront partial sums/scans
//   k_decide   [1 WG]   normalisation constant, ESS, resampling decision, offspring table,
//                       backward push of posterior weight through the ancestor ledger
//   k_count    [grid]   CountModel::extract_and_update_count over the per-slot event logs
//   k_count_fin[1 WG]   ordered reduction of k_count partials
//   k_resample [grid]   normalisation or systematic-resampling gather (ParticleContainer::resample)
// The host never reads device memory inside pf_run: the decision to resample is taken on the
// device and every kernel is launched unconditionally (k_count only on segments where the
// reference's lag rule, which is particle-independent, schedules an update).
//
// No CUDA compatibility layer, no CPU fallback: this file is HIP for gfx950 only.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/smcsmc_pf.h"
#include "pf_device.h"
#include "pf_types.h"
#include "pf_lane.h"
#include "pf_tree_reg.h"
#include "pf_look_reg.h"
#include "pf_row_parts.h"
#include "pf_lds_body.h"
#include "pf_mp_host.h"
#include "pf_wide_host.h"
#include "pf_pipe.h"
#include "pf_lds_pipe.h"

using namespace pf;

// ------------------------------------------------------------------ k_init, k_extend (bodies in pf_lds_body.h)
__global__ __launch_bounds__(PF_BS) void k_init(KArgs A, double initial_position) {
    extern __shared__ double smem[];
    init_lds_body(A, initial_position, smem);
}

__global__ __launch_bounds__(PF_BS) void k_extend(KArgs A, long long s) {
    extern __shared__ double smem[];
    extend_lds_body(A, s, smem);
}

// A wave-uniform value moved into vector registers on purpose.  The extend kernels are short of scalar registers (the
// argument block alone is ~240 of them; spilled ones come back through v_readlane inside the update loop, with the
// s_nop padding that follows), while only a third of the vector file is in use: the handful of scalars the update loop
// reads on every trip live in VGPRs instead.
__device__ __forceinline__ double in_vgpr(double x) { double y; asm("v_mov_b64 %0, %1" : "=v"(y) : "s"(x)); return y; }
__device__ __forceinline__ unsigned long long in_vgpr(unsigned long long x) { unsigned long long y; asm("v_mov_b64 %0, %1" : "=v"(y) : "s"(x)); return y; }

#ifdef PF_STAMPS
__device__ __forceinline__ void pf_acc_trip(unsigned long long* a) { a[5] += 1; }
#else
#define pf_acc_trip(a) do {} while (0)
#endif
#ifdef PF_STAMPS
#define PF_STAMP(k) do { if (A.stamps && (threadIdx.x & 63) == 0 && s < A.stamp_rows)                                   \
        A.stamps[((size_t)s * A.nc + (size_t)(((long long)pf_bx() * PF_BS + threadIdx.x) >> 6)) * PF_STAMP_W + (k)] = wall_clock64(); } while (0)
#define PF_TICK(var) unsigned long long var = wall_clock64()
#define PF_ACC(slot, t0, t1) pf_acc[slot] += (t1) - (t0)
#define PF_ACC_DECL unsigned long long pf_acc[6] = {0, 0, 0, 0, 0, 0}, pf_acc2[8] = {0, 0, 0, 0, 0, 0, 0, 0}
// (what row_update_trip takes of them)
#define PF_ACC_PARAMS , unsigned long long* pf_acc, unsigned long long* pf_acc2, unsigned long long tk1
#define PF_ACC_ARGS , pf_acc, pf_acc2, tk1
// the finer split of a trip (words 21-28): [0] no-mutation weight up to the factor, [1] its two products, [2..7] the genealogy update
// between the marks of PF_GTICK (pf_tree_reg.h): draws, cut point, descendant mask, node searches, walk and inverse, tree edit
#define PF_ACC2(slot, t0, t1) pf_acc2[slot] += (t1) - (t0)
#define PF_ACC_STORE do { if (A.stamps && (threadIdx.x & 63) == 0 && s < A.stamp_rows) {                                \
        for (int k_ = 0; k_ < 6; ++k_)                                                                                  \
            A.stamps[((size_t)s * A.nc + (size_t)(((long long)pf_bx() * PF_BS + threadIdx.x) >> 6)) * PF_STAMP_W + 9 + k_] = pf_acc[k_]; \
        for (int k_ = 0; k_ < 8; ++k_)                                                                                  \
            A.stamps[((size_t)s * A.nc + (size_t)(((long long)pf_bx() * PF_BS + threadIdx.x) >> 6)) * PF_STAMP_W + 21 + k_] = pf_acc2[k_]; } } while (0)
#else
#define PF_STAMP(k) do {} while (0)
#define PF_TICK(var) do {} while (0)
#define PF_ACC(slot, t0, t1) do {} while (0)
#define PF_ACC2(slot, t0, t1) do {} while (0)
#define PF_ACC_DECL do {} while (0)
#define PF_ACC_PARAMS
#define PF_ACC_ARGS
#define PF_ACC_STORE do {} while (0)
#endif

template <class KA>
__device__ __forceinline__ int gridDim_particles(const KA& A) { return (int)((A.Np + PF_BS - 1) / PF_BS); }

// ------------------------------------------------------------------ k_extend_reg
// Same computation as k_extend with the local tree held in registers (pf_tree_reg.h); used for
// n <= 8.  LDS only carries the two epoch tables.
// With fuse != 0 the launch also completes the previous row: the in-place normalisation or the resampling gather of
// k_resample (pc.cpp:321-392, 435-437) happens while the particle is loaded, which removes one kernel and its
// launch gap from the per-row critical path.  The arithmetic is k_resample's, operation for operation.
// EXACT: the number of haplotypes equals NM, so every `r < n - 1` guard of the unrolled tree loops is decided at
// compile time (the guards are compare + exec-mask instructions, and instructions are what the time is made of)
// TREES: -arg, the records also carry the descendants of the node each update creates
// PIPE: single-launch pipeline (k_pipe).  The workgroup takes the decision on the previous row itself (decide_row),
// derives the offspring offsets of its own particles and finds the parent of each of its slots by a two-level search
// over the pilot prefix sums -- no offspring / parent table from an earlier kernel is read --, reads the previous row
// from one slot of the state ring and writes this row into the next, and leaves the offspring table for the ledger.
// HEAD (with PIPE; k_sweep4, k_sweep4q, k_sweep4t): the addresses of the head come from the row header H (SweepHead in registers, pf_pipe.h), which
// the caller has loaded in one batch.  Every request of the head then goes out back to back in the order the prologue consumes them --
// the partials of the decision and last1, the note on the row before, the scans the parent search stages, the particle's own state and
// counters, the epoch tables, the row's segment last -- and nothing is waited for before the last one is out.  What every lane loads
// from one address (the note, last1, the segment) would be moved to scalar registers, behind a wait, right where it is loaded: those
// values stay in vector registers until pf_arrive() where they are first used.  PR.pos_prev is not used: the end of row s - 1 is
// requested with the rest.
// LOOK (with PIPE, without HEAD, BIASED and TREES; k_sweep<..., LOOK>): the auxiliary particle filter's look-ahead factor (look_factor,
// pf_look_reg.h = k_lookahead) enters the pilot weight here, behind the site likelihood and in front of the state stores and the wavefront
// partials, so that the partials decide_row reads are those k_lookahead leaves.  The previous factor travels with the state: the slot's own
// with the preload, the parent's on a resampling row.  A completion-only launch applies none and hands on the one it carried.
__device__ __forceinline__ int pf_arrive(int v) { asm volatile("" : "+v"(v)); return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long pf_arrive(long long v) {
    asm volatile("" : "+v"(v));
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v & 0xffffffffu));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double pf_arrive(double v) { return __longlong_as_double(pf_arrive(__double_as_longlong(v))); }

// ---- parts of a row that extend_reg_body and the paired form of the row kernel (extend_pair_body, pf_pair.h) share ----
// the window of pilot scans a workgroup requests ahead of the parent search: PF_PIPE_STAGE wavefronts centred on its own `own`, which
// start at wavefront `first`
__device__ __forceinline__ int row_spec_lo(int first, int own, int nc, int flags) {
    int spec_lo = first - (PF_PIPE_STAGE - own) / 2;
    if (spec_lo > nc - PF_PIPE_STAGE) spec_lo = nc - PF_PIPE_STAGE;
    if (spec_lo < 0) spec_lo = 0;
    if (flags & 256) spec_lo = -0x40000000;              // PF_DEBUG_NO_SPEC_STAGE (A/B): never covers the range
    return spec_lo;
}
// parent search, first level: the wavefront the parent of a slot sits in (lhs = (p + u) * S1)
__device__ __forceinline__ int row_parent_chunk(const PipeLds& q, int nc, double lhs, double dn) {
    int lo_c = 0, hi_c = nc - 1;
    while (lo_c < hi_c) {
        int mid = (lo_c + hi_c) >> 1;
        if (lhs < dn * q.pmx[mid + 1]) hi_c = mid; else lo_c = mid + 1;
    }
    return lo_c;
}
// parent search, second level: the parent a of slot p inside wavefront pch, from the staged scans where they cover it, and whether p
// is a's first copy
// (found(): called between the two, where the profiling build has a stamp)
template <class KA, class MARK>
__device__ __forceinline__ void row_parent_in_chunk(const KA& A, const PipeLds& q, const double* sm, int pch, int stage_lo, int nst, double lhs, double dn,
                                                    long long p, const RowDecision& d, long long& a, bool& first_copy, MARK&& found) {
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
    a = (long long)pch * 64 + lo_l;
    found();
    if (a > A.Np - 1) a = A.Np - 1;
    // slot p is the first copy of a (it keeps a's next recombination position) iff it equals a's offset
    const int la = (int)(a & 63);
    if (p == 0 || a == 0) first_copy = (p == 0);
    else {
        double vprev = la > 0 ? val_at(la - 1) : pm_p;      // largest prefix sum up to a - 1
        if (a != (long long)pch * 64 + lo_l) {             // clamped: recompute on the true chunk of a - 1
            long long am = a - 1;
            int chm = (int)(am >> 6);
            double w = pipe_chunk_offset(q, chm) + sm[am];
            vprev = q.pmx[chm] > w ? q.pmx[chm] : w;
        }
        first_copy = ((((double)(p - 1)) + d.u) * d.S1 < dn * vprev);
    }
}
// the record that closes the stretch of an old slot with offspring: everything but the heights
__device__ __forceinline__ void row_close_record(double* rec, double x_mark, double pos, int mark_limit, int n) {
    rec[0] = x_mark;
    rec[1] = pos;
    rec[2] = 0.0; rec[3] = 0.0;
    rec[4] = __longlong_as_double((long long)make_meta(1, mark_limit, -1, n));
}
// (RowMasks, row_masks, row_site_lik, RowScans, row_scans, row_scans_store: pf_row_parts.h)

// the head of a row of the headline row kernels, requests only: what the decision on the row before needs and the window of pilot scans
// that starts at wavefront spec_lo
template <class HR>
__device__ __forceinline__ void row_head_decision(const HR& H, int nc, long long Np_head, int spec_lo, RowPre& pre, long long& o_nres, int& o_bflag, int& o_bgen,
                                                  double (&spec_sm)[PF_PIPE_STAGE * 64 / PF_BS]) {
    const int ch = threadIdx.x, perc = (nc + PF_BS - 1) / PF_BS;
    pre.have = true;
    if (ch < nc) { pre.vp = PF_HP(H, cpost)[ch]; pre.vs = PF_HP(H, csq)[ch]; pre.vl = PF_HP(H, cpil)[ch]; }
    if (ch + PF_BS < nc) { pre.vp2 = PF_HP(H, cpost)[ch + PF_BS]; pre.vs2 = PF_HP(H, csq)[ch + PF_BS]; pre.vl2 = PF_HP(H, cpil)[ch + PF_BS]; }
    // (the entry or the two entries of the prefix-maxima pass, row_preload; two plain guarded requests: behind an if / else chain
    // the second one waited for everything before it)
    const int cm = perc == 2 ? 2 * ch : ch;
    if (perc <= 2 && cm < nc) pre.vm = PF_HP(H, cmx1)[cm];
    if (perc == 2 && cm + 1 < nc) pre.vm2 = PF_HP(H, cmx1)[cm + 1];
    pre.last1 = *PF_HP(H, last1);
    asm volatile("" ::: "memory");
    o_nres = PF_HP(H, xr_before)->n_res; o_bflag = PF_HP(H, xr_before)->flag; o_bgen = PF_HP(H, xr_before)->gen;
    asm volatile("" ::: "memory");
    // (the window of scans requested ahead of the parent search: as in the other form of the head)
#pragma unroll
    for (int k = 0; k < PF_PIPE_STAGE * 64 / PF_BS; ++k) {
        const long long src = (long long)spec_lo * 64 + k * PF_BS + threadIdx.x;
        spec_sm[k] = (src >= 0 && src < Np_head) ? PF_HP(H, scan1m)[src] : PF_INF;
    }
    asm volatile("" ::: "memory");
}
// ... the epoch tables and the bucket table, one entry a thread
template <class HR>
__device__ __forceinline__ void row_head_tables(const HR& H, int E_head, double& h_T, double& h_Hc, double& h_I, bool& use_lut, unsigned& h_lut) {
    if ((int)threadIdx.x < E_head) { h_T = PF_HP(H, T)[threadIdx.x]; h_Hc = PF_HP(H, Hc)[threadIdx.x]; h_I = PF_HP(H, inv2N)[threadIdx.x]; }
    use_lut = PF_HP(H, lut) != nullptr;
    if (use_lut && threadIdx.x < 2 * PF_LUT_N / 4) h_lut = ((const __attribute__((address_space(1))) unsigned*)PF_HP(H, lut))[threadIdx.x];
}
// ... the end of the row before and the row's own segment
template <int NM, bool EXACT, class HR>
__device__ __forceinline__ void row_head_segment(const HR& H, long long s, int n, double& sgp_start, double& sgp_len, double& sg_start, double& sg_len, int& sg_limit, int& sg_state,
                                                 int (&sg_allele)[NM]) {
    // (requested whatever the step, from rows the call has: a flush step and the first step of a call use none of them, and a
    // request under a condition is one more join at which the value would have to be in its final register)
    {
        const long long s_first = PF_HL(H, s_begin), s_last = PF_HL(H, s_last);
        const long long sq = s <= s_last ? s : s_last, sb = s > s_first ? s - 1 : s_first;
        sgp_start = PF_HP(H, seg_start)[sb]; sgp_len = PF_HP(H, seg_len)[sb];
        sg_start = PF_HP(H, seg_start)[sq]; sg_len = PF_HP(H, seg_len)[sq];
        sg_limit = PF_HP(H, seg_limit)[sq]; sg_state = ((const __attribute__((address_space(1))) unsigned char*)PF_HP(H, seg_state))[sq];
        // (as loaded, all four in one word where there are four: sign-extended where they arrive)
        if constexpr (EXACT && NM == 4) sg_allele[0] = (int)*(const __attribute__((address_space(1))) unsigned*)(PF_HP(H, seg_alleles) + (size_t)sq * 4);
        else {
#pragma unroll
            for (int i = 0; i < NM; ++i) if (i < n) sg_allele[i] = ((const __attribute__((address_space(1))) unsigned char*)PF_HP(H, seg_alleles))[(size_t)sq * n + i];
        }
    }
}
// the row's segment where it is first used: in scalar registers, the bytes sign-extended (a flush step has none)
template <int NM, bool EXACT>
__device__ __forceinline__ void row_segment_arrive(bool do_extend, int n, double& sg_start, double& sg_len, int& sg_limit, int& sg_state, int (&sg_allele)[NM]) {
    if (!do_extend) {
        sg_start = 0.0; sg_len = 0.0; sg_limit = 0; sg_state = 1;
#pragma unroll
        for (int i = 0; i < NM; ++i) sg_allele[i] = 0;
    } else {
        sg_start = pf_arrive(sg_start); sg_len = pf_arrive(sg_len); sg_limit = pf_arrive(sg_limit); sg_state = (int)(int8_t)pf_arrive(sg_state);
        if constexpr (EXACT && NM == 4) {
            const unsigned w = (unsigned)pf_arrive(sg_allele[0]);
#pragma unroll
            for (int i = 0; i < NM; ++i) sg_allele[i] = (int)(int8_t)(w >> (8 * i));
        } else {
#pragma unroll
            for (int i = 0; i < NM; ++i) if (i < n) sg_allele[i] = (int)(int8_t)pf_arrive(sg_allele[i]);
        }
    }
}
// The wavefronts the parents of a workgroup's slots sit in, from what its NW searching wavefronts left in q.wint, and their pilot scans in q.stage:
// the window requested with the head where it covers them, staged now otherwise.  Every thread of the workgroup calls this (barriers).
template <int NW, class KA>
__device__ __forceinline__ void row_stage_parents(const KA& A, const PipeLds& q, const double* sm, int spec_lo, int& stage_lo, int& nst) {
    int cmin = q.wint[0], cmax = q.wint[PF_BS / 64];
    for (int w = 1; w < NW; ++w) {
        cmin = q.wint[w] < cmin ? q.wint[w] : cmin;
        cmax = q.wint[PF_BS / 64 + w] > cmax ? q.wint[PF_BS / 64 + w] : cmax;
    }
    nst = cmax - cmin + 1;
    if (nst > PF_PIPE_STAGE) nst = PF_PIPE_STAGE;
    if (nst < 0) nst = 0;
    stage_lo = cmin;
    if (cmin >= spec_lo && cmax < spec_lo + PF_PIPE_STAGE) {
        stage_lo = spec_lo; nst = PF_PIPE_STAGE;       // the scans requested with the prologue cover the range
    } else {
        __syncthreads();                               // everybody has read the range before the buffer is refilled
        for (int idx = threadIdx.x; idx < nst * 64; idx += PF_BS) {
            long long src = (long long)cmin * 64 + idx;
            q.stage[idx] = src < A.Np ? sm[src] : PF_INF;
        }
    }
    __syncthreads();
}

// the state a row of the headline row kernels continues from: ring slot slot_prev (the pointers of the row header), or on the first step of a
// call the slot Ctrl::cur names, and then the handle's own record counters
struct RowHeadPtrs {
    const __attribute__((address_space(1))) double* S; const __attribute__((address_space(1))) int8_t* C;
    const __attribute__((address_space(1))) double* w_post; const __attribute__((address_space(1))) double* w_pilot;
    const __attribute__((address_space(1))) double* next_base; const __attribute__((address_space(1))) double* x_mark;
    const __attribute__((address_space(1))) int* mark_limit; const __attribute__((address_space(1))) double* Ltree;
    const __attribute__((address_space(1))) unsigned* widx;
};
template <class HR>
__device__ __forceinline__ RowHeadPtrs row_head_ptrs(const HR& H, bool complete, long long Np_head, int n_head) {
    RowHeadPtrs r;
    r.S = PF_HP(H, S); r.C = PF_HP(H, C); r.w_post = PF_HP(H, w_post); r.w_pilot = PF_HP(H, w_pilot);
    r.next_base = PF_HP(H, next_base); r.x_mark = PF_HP(H, x_mark); r.mark_limit = PF_HP(H, mark_limit); r.Ltree = PF_HP(H, Ltree);
    r.widx = PF_HP(H, rg_widx);
    if (!complete) {
        const long long dk = (long long)__builtin_amdgcn_readfirstlane(PF_HP(H, ctrl)->cur) - PF_HI(H, slot_prev), dN = dk * Np_head, n1 = n_head - 1;
        r.S += dN * n1; r.C += dN * 2 * n1; r.w_post += dN; r.w_pilot += dN; r.next_base += dN; r.x_mark += dN; r.mark_limit += dN; r.Ltree += dN;
        r.widx = PF_HP(H, widx);
    }
    return r;
}
// weights of a copy (pc.cpp:350-351)
__device__ __forceinline__ void row_copy_weights(double& w_post, double& w_pilot, double inv, double S1v, double dn) {
    double wp = w_post * inv;
    double wq = w_pilot * inv;
    double sumn = S1v * inv;
    double adj = sumn / (dn * wq);
    w_post = wp * adj;
    w_pilot = wq * adj;
}
// (the stores of a row's end -- row_store_tree, row_store_chain, row_store_counters: pf_row_parts.h)
// the per-lane context of the update loop, but for the position in the recombination guide
template <bool BIASED, bool TREES, bool PIPE, class KA>
__device__ __forceinline__ void row_ctx(RCtx& cx, const KA& A, const double* sT, const double* sI, const double* sH, const double* sBH, const double* sBS, int n, long long p,
                                        double v_L, double v_mu, double v_rho, bool use_lut, const unsigned* s_lut, int draws, unsigned o_tab_end) {
    cx.T = sT; cx.I = sI; cx.H = sH; cx.E = A.E; cx.n = n; cx.L = v_L; cx.mu = v_mu; cx.rho = v_rho;
    cx.seed = in_vgpr(A.seed); cx.slot = (unsigned)p; cx.stream = 0;
    cx.nb = A.n_bias + 1; cx.bH = sBH; cx.bS = sBS; cx.last_iw = 1.0;
    cx.want_desc = A.lmap_opp != nullptr || TREES; cx.want_desc_new = TREES; cx.last_desc = 0; cx.last_desc_new = 0;
    cx.vbc = A.vb_coal; cx.upd_fac = 1.0;
    cx.gK = BIASED ? A.g_K : 0; cx.gpos = A.g_pos; cx.grho = A.g_rho; cx.gleaf = A.g_leaf; cx.last_rbiw = 1.0;
    cx.ridx = 0; cx.g_rp = 0; cx.g_sb = 0;
    if constexpr (PIPE) {
        cx.lutT = use_lut ? (const unsigned char*)s_lut : nullptr;
        cx.lutH = use_lut ? (const unsigned char*)s_lut + PF_LUT_N : nullptr;
        cx.kbT = A.lut_kbT; cx.kbH = A.lut_kbH;
        cx.tab = nullptr; cx.tab_end = 0; cx.pf_ok = false; cx.pf_ctr = 0; cx.draws_log = false;
        if (draws) {
            cx.tab = (const double2*)A.dt_tab + (size_t)p * PF_DRAW_RING;
            cx.tab_end = o_tab_end;
        }
    }
}

// one trip of the update loop behind the move to updated_to < extend_to: the record of the stretch that ends there, the genealogy update, the
// tracked length and the next recombination position (w_post, w_pilot: only vb_coal and focused sampling touch them)
template <int NM, bool BIASED, bool EXACT, bool TREES, bool PIPE, class KA>
__device__ __forceinline__ void row_update_trip(const KA& A, RCtx& cx, RTree<NM>& t, DStore& ds, long long p, int n, int limit, int leaf_status, unsigned present_mask,
                                                double updated_to, unsigned& widx, double& x_mark, int& mark_limit, double& next_base, double& B,
                                                double& w_post, double& w_pilot, const double* sBH, const double* sBS PF_ACC_PARAMS) {
    double* rec = rec_ptr(A, p, widx);
    rec[0] = x_mark;
    rec[1] = updated_to;
#pragma unroll
    for (int r = 0; r < RTree<NM>::NI; ++r) if (r < n - 1) rec[5 + r] = t.S[r];
    double h, tc;
    PF_TICK(tk2);
    PF_ACC(1, tk1, tk2);
    r_genealogy_update<NM, BIASED, PIPE, PIPE && EXACT && NM == 4 && !BIASED && !TREES>(cx, t, &h, &tc);
    PF_TICK(tk3);
    PF_ACC(2, tk2, tk3);
#ifdef PF_STAMPS
    PF_ACC2(2, tk2, cx.gt[0]);
    for (int k_ = 0; k_ < 5; ++k_) PF_ACC2(3 + k_, cx.gt[k_], cx.gt[k_ + 1]);
#endif
    if (cx.vbc) { w_post *= cx.upd_fac; w_pilot *= cx.upd_fac; cx.upd_fac = 1.0; }
    rec[2] = h;
    rec[3] = tc;
    rec[4] = __longlong_as_double((long long)make_meta(0, mark_limit, limit, n, cx.last_desc, TREES ? cx.last_desc_new : 0u));
    ++widx;
    if (leaf_status == 0) B = r_tracked_len(t, n, present_mask);
    if (leaf_status == 1) B = cx.Ltree;
    PF_TICK(tk4);
    PF_ACC(3, tk3, tk4);
    pf_acc_trip(pf_acc);
    if (BIASED) {
        // particle.cpp:866-891: immediate vs delayed application of the importance weight
        double iw = cx.last_iw, rbiw = cx.last_rbiw;
        double delay_height = (A.delay_type & 3) == 0 ? h : tc;
        int idx = 0;
        while (idx + 1 < cx.nb + 1 && sBH[idx + 1] < delay_height) ++idx;
        if (idx >= cx.nb) idx = cx.nb - 1;
        if (sBS[idx] == 1.0 && !(A.delay_type & 4)) { w_post *= rbiw; w_pilot *= rbiw; iw /= rbiw; }   // bit 2: every factor delayed (pf_model.delay_type)
        double delay = A.app_delays[r_epoch_of(cx, delay_height)];
        d_adjust_with_delay(ds, w_post, w_pilot, iw, delay, updated_to);
    }
    PF_TICK(tk5);
    next_base = r_sample_next_base<true, PIPE>(cx, updated_to);      // fourth uniform of the update
    x_mark = updated_to;
    mark_limit = limit;
    PF_TICK(tk6);
    PF_ACC(4, tk5, tk6);
}

template <int NM, bool BIASED, bool EXACT = false, bool TREES = false, bool PIPE = false, bool HEAD = false, bool LOOK = false, class KA>
__device__ __forceinline__ void extend_reg_body(const KA& A, long long s, int fuse, PipeRow PR = PipeRow(), const SweepHeadR& H = SweepHeadR()) {
    static_assert(!HEAD || PIPE, "the row header belongs to the row pipeline");
    static_assert(!LOOK || (PIPE && !HEAD && !BIASED && !TREES), "the look-ahead rides on the plain rows of k_sweep");
    extern __shared__ double smem[];
    int E_head; long long Np_head; int n_head;
    if constexpr (HEAD) { E_head = PF_HI(H, E); Np_head = PF_HL(H, Np); n_head = PF_HI(H, n); } else { E_head = A.E; Np_head = A.Np; n_head = A.n; }
    double* sT = smem;                            // epoch starts and ...
    double* sH = smem + PF_EPAD;                  // ... cumulative coalescence intensity there, both padded with +inf (r_search4)
    double* sI = sH + PF_EPAD;
    double* sBH = sI + E_head;                    // bias band boundaries / strengths (focused sampling)
    double* sBS = sBH + (PF_BIAS_MAX + 2);
    const Ctrl* c = A.ctrl;
    const int n = EXACT ? NM : n_head;
    const long long p = (long long)pf_bx() * PF_BS + threadIdx.x;
    const bool active = p < Np_head;
    const int lane = threadIdx.x & 63;
    // PIPE: everything the prologue and the particle itself need from memory is requested first, in one round trip: the
    // partials of the decision, this slot's own state of the previous row (what most rows continue from, and what the
    // old slot's closing record needs when the row resampled) -- a copy reloads from its parent afterwards.
    PF_STAMP(0);
    RowPre pre;
    RTree<NM> t0;
    double o_wpost = 0.0, o_wpilot = 0.0, o_next = 0.0, o_xmark = 0.0, o_Ltree = 0.0, o_sm = 0.0, o_ebuf = 0.0;
    [[maybe_unused]] double o_la = 1.0;
    int o_ml = 0;
    unsigned o_widx = 0;
    unsigned long long o_ctr = 0;
    unsigned o_tab_end = 0;
    long long o_nres = 0; int o_bflag = 0, o_bgen = 0;
    double spec_sm[PF_PIPE_STAGE * 64 / PF_BS];
    int spec_lo = 0;
    // PIPE: the row's own segment (end, mutation limit, state, alleles) depends on nothing but s.  Read where it is used -- behind
    // the prologue, the end before the limit before the alleles, the state after the update loop -- it was four dependent memory
    // round trips of every wavefront of every row; here they ride along with the first loads of the launch.
    double sg_start = 0.0, sg_len = 0.0;
    int sg_limit = 0, sg_state = 1;
    int sg_allele[NM];
#pragma unroll
    for (int i = 0; i < NM; ++i) sg_allele[i] = 0;
    if constexpr (PIPE && !HEAD) {
        if (PR.extend) {
            sg_start = A.seg_start[s]; sg_len = A.seg_len[s];
            sg_limit = A.seg_limit[s]; sg_state = A.seg_state[s];
            const int8_t* al = A.seg_alleles + (size_t)s * n;
#pragma unroll
            for (int i = 0; i < NM; ++i) if (i < n) sg_allele[i] = al[i];
        }
    }
    if constexpr (PIPE && !HEAD) {
        const int fs = __builtin_amdgcn_readfirstlane(PR.slot_prev >= 0 ? PR.slot_prev : c->cur);
        if (PR.complete) {
            pre = row_preload(A, fs);
            // the row before it: what the extend role of the previous launch noted about it (the same numbers the bookkeeping
            // role publishes in Ctrl::ri, without depending on the launch that carries that role)
            o_nres = c->xr[(fs + PF_RING - 1) & (PF_RING - 1)].n_res; o_bflag = c->xr[(fs + PF_RING - 1) & (PF_RING - 1)].flag; o_bgen = c->xr[(fs + PF_RING - 1) & (PF_RING - 1)].gen;
            // The parent search of a resampling row stages the pilot scans of the wavefronts its parents sit in.  Offspring
            // stay close to their parents' slots (the offsets drift like a random walk of a few hundred slots), so the scans
            // of this workgroup's own wavefronts and six on either side are requested now, with everything else the prologue
            // reads, instead of in a round trip of their own once the search knows the range; a range outside this window
            // is staged the old way.
            spec_lo = row_spec_lo(pf_bx() * (PF_BS / 64), PF_BS / 64, A.nc, A.flags);
            const double* sm0 = A.rg_scan1m + (size_t)fs * A.Np;
#pragma unroll
            for (int k = 0; k < PF_PIPE_STAGE * 64 / PF_BS; ++k) {
                const long long src = (long long)spec_lo * 64 + k * PF_BS + threadIdx.x;
                spec_sm[k] = (src >= 0 && src < A.Np) ? sm0[src] : PF_INF;
            }
        }
        if (active) {
            const DState own = state_slot(A, fs);
#pragma unroll
            for (int r = 0; r < RTree<NM>::NI; ++r) {
                t0.S[r] = 0.0; t0.C0[r] = 0; t0.C1[r] = 0;
                if (r < n - 1) {
                    t0.S[r] = own.S[(size_t)r * A.Np + p];
                    t0.C0[r] = own.C[(size_t)(2 * r) * A.Np + p];
                    t0.C1[r] = own.C[(size_t)(2 * r + 1) * A.Np + p];
                }
            }
            o_wpost = own.w_post[p]; o_wpilot = own.w_pilot[p]; o_next = own.next_base[p]; o_xmark = own.x_mark[p];
            o_ml = own.mark_limit[p]; o_Ltree = own.Ltree[p];
            if constexpr (LOOK) o_la = own.lookahead[p];
            o_widx = PR.complete ? A.rg_widx[(size_t)fs * A.Np + p] : A.widx[p];
            o_ctr = A.rng_ctr[p]; o_ebuf = A.ebuf[p];
            if (PR.draws) o_tab_end = (unsigned)A.dt_filled[(size_t)((PR.draws - 1) ^ 1) * A.Np + p];
            if (PR.complete) o_sm = A.rg_scan1m[(size_t)fs * A.Np + p];
        }
    }
    __shared__ unsigned s_lut[PIPE ? 2 * PF_LUT_N / 4 : 1];
    bool use_lut = false;
    double h_T = PF_INF, h_Hc = PF_INF, h_I = 0.0, sgp_start = 0.0, sgp_len = 0.0;
    unsigned h_lut = 0;
    if constexpr (HEAD) {
        static_assert(PF_EPAD <= PF_BS && 2 * PF_LUT_N / 4 <= PF_BS && !BIASED, "one table entry a thread");
        const int nc = PF_HI(H, nc);
        // the state the row continues from: ring slot slot_prev, or on the first step of a call the slot Ctrl::cur names
        const RowHeadPtrs hp = row_head_ptrs(H, PR.complete != 0, Np_head, n_head);
        const auto pS = hp.S; const auto pC = hp.C; const auto pwpost = hp.w_post; const auto pwpil = hp.w_pilot;
        const auto pnext = hp.next_base; const auto pxm = hp.x_mark; const auto pml = hp.mark_limit; const auto pLt = hp.Ltree; const auto pwidx = hp.widx;
        if (PR.complete) {
            spec_lo = row_spec_lo(pf_bx() * (PF_BS / 64), PF_BS / 64, nc, PF_HI(H, flags));
            row_head_decision(H, nc, Np_head, spec_lo, pre, o_nres, o_bflag, o_bgen, spec_sm);
        }
        // (every lane asks, the lanes behind the last particle for the last particle's and use nothing of it: requests under a lane
        // condition come out with the widening of the bytes, and a wait, right behind them)
        const __attribute__((address_space(1))) unsigned char* pCu = (const __attribute__((address_space(1))) unsigned char*)pC;
        {
            const long long q = active ? p : Np_head - 1;
#pragma unroll
            for (int r = 0; r < RTree<NM>::NI; ++r) {
                t0.S[r] = 0.0; t0.C0[r] = 0; t0.C1[r] = 0;
                if (r < n - 1) {
                    t0.S[r] = pS[(size_t)r * Np_head + q];
                    t0.C0[r] = pCu[(size_t)(2 * r) * Np_head + q];         // as loaded: sign-extended behind the prologue
                    t0.C1[r] = pCu[(size_t)(2 * r + 1) * Np_head + q];
                }
            }
            o_wpost = pwpost[q]; o_wpilot = pwpil[q]; o_next = pnext[q]; o_xmark = pxm[q];
            o_ml = pml[q]; o_Ltree = pLt[q];
            o_widx = pwidx[q];
            o_ctr = PF_HP(H, rng_ctr)[q]; o_ebuf = PF_HP(H, ebuf)[q];
            if (PR.draws) o_tab_end = (unsigned)PF_HP(H, dt_filled)[q];
            o_sm = PF_HP(H, scan1m)[q];
        }
        asm volatile("" ::: "memory");
        row_head_tables(H, E_head, h_T, h_Hc, h_I, use_lut, h_lut);
        asm volatile("" ::: "memory");
        row_head_segment<NM, EXACT>(H, s, n, sgp_start, sgp_len, sg_start, sg_len, sg_limit, sg_state, sg_allele);
        asm volatile("" ::: "memory");
    } else {
        for (int e = threadIdx.x; e < PF_EPAD; e += blockDim.x) {
            sT[e] = e < A.E ? A.T[e] : PF_INF;
            sH[e] = e < A.E ? A.Hc[e] : PF_INF;
            if (e < A.E) sI[e] = A.inv2N[e];
        }
        if (BIASED && threadIdx.x < PF_BIAS_MAX + 2) {
            sBH[threadIdx.x] = A.bias_H[threadIdx.x];
            if (threadIdx.x < PF_BIAS_MAX + 1) sBS[threadIdx.x] = A.bias_S[threadIdx.x];
        }
        use_lut = PIPE && A.lut != nullptr;
        if constexpr (PIPE) {
            if (use_lut && threadIdx.x < 2 * PF_LUT_N / 4) s_lut[threadIdx.x] = ((const unsigned*)A.lut)[threadIdx.x];
        }
    }
    // ---- what completing the previous row needs ----
    int cur = 0, from_slot = 0;
    bool completing = false, gather = false;
    double inv = 1.0, S1v = 0.0, pos_prev = 0.0;
    int lo_p = 0, lo_p1 = 0;
    bool first_copy = true;
    long long a = p;
    int G_end = 0, ev = 0;
    if constexpr (PIPE) {
        PipeLds q = pipe_carve(sBS + (PF_BIAS_MAX + 1), A.nc);
        cur = PR.slot_out; from_slot = PR.slot_prev >= 0 ? PR.slot_prev : c->cur;
        completing = PR.complete != 0;
        pos_prev = PR.pos_prev;
        if (completing) {
            const int row_slot = from_slot;                        // ring slot of the row being completed
            if constexpr (HEAD) {
                PF_STAMP(1);
                pre.last1 = pf_arrive(pre.last1); o_nres = pf_arrive(o_nres); o_bflag = pf_arrive(o_bflag); o_bgen = pf_arrive(o_bgen);
            }
            const long long n_res = o_nres + o_bflag;
            G_end = o_bgen + o_bflag;
            ev = (int)n_res;
            if constexpr (!HEAD) PF_STAMP(1);
#pragma unroll
            for (int k = 0; k < PF_PIPE_STAGE * 64 / PF_BS; ++k) q.stage[k * PF_BS + threadIdx.x] = spec_sm[k];    // visible after decide_row's barriers
            RowDecision d = decide_row<true>(A, q, row_slot, n_res, pre);
            PF_STAMP(2);
            inv = d.inv; S1v = d.S1;
            gather = d.flag != 0;
            if (pf_bx() == 0 && threadIdx.x == 0) {
                Ctrl* cw = A.ctrl;
                cw->xr[row_slot].n_res = n_res; cw->xr[row_slot].gen = G_end; cw->xr[row_slot].flag = d.flag;
            }
            if (gather) {
                const double dn = (double)A.Np;
                const double invS1 = 1.0 / d.S1;
                const double* sm = A.rg_scan1m + (size_t)row_slot * A.Np;
                const int wave = threadIdx.x >> 6;
                int ch_own = (int)(p >> 6);
                double coff_own = 0.0, v_own = 0.0;
                int lo_next = 0;
                if (active) {
                    coff_own = pipe_chunk_offset(q, ch_own);
                    double w = coff_own + o_sm;
                    v_own = q.pmx[ch_own] > w ? q.pmx[ch_own] : w;          // largest pilot prefix sum up to particle p
                    lo_next = p + 1 < A.Np ? pipe_lo_from(v_own, dn, A.Np, d.S1, invS1, d.u) : (int)A.Np;
                    q.slo[threadIdx.x] = lo_next;
                }
                PF_STAMP(16);
                // ---- parent of slot p: the first particle a with (p+u) * S1 < N * (largest prefix sum up to a) ----
                const double lhs = ((double)p + d.u) * d.S1;
                int pch = 0;
                if (active) pch = row_parent_chunk(q, A.nc, lhs, dn);
                PF_STAMP(17);
                int cmin = active ? pch : 0x7fffffff, cmax = active ? pch : -1;
                wave_minmax(cmin, cmax);
                if (lane == 0) { q.wint[wave] = cmin; q.wint[PF_BS / 64 + wave] = cmax; }
                __syncthreads();
                if (active) lo_p1 = lo_next;
                if (active) {
                    if (threadIdx.x > 0) lo_p = q.slo[threadIdx.x - 1];
                    else lo_p = p > 0 ? pipe_lo_from(q.pmx[ch_own], dn, A.Np, d.S1, invS1, d.u) : 0;
                }
                // survivors of this workgroup (the ledger positions the run list of the ending generation with them)
                {
                    unsigned long long bal = __ballot(active && lo_p1 > lo_p);
                    if (lane == 0) {
                        if (A.blk_gran == PF_BS / 64) A.rg_blkcnt[((size_t)row_slot * gridDim_particles(A) + pf_bx()) * (PF_BS / 64) + wave] = __popcll(bal);
                        else q.wint[2 * (PF_BS / 64) + wave] = __popcll(bal);
                    }
                }
                PF_STAMP(18);
                int stage_lo, nst;
                row_stage_parents<PF_BS / 64>(A, q, sm, spec_lo, stage_lo, nst);
                PF_STAMP(19);
                if (threadIdx.x == 0 && A.blk_gran != PF_BS / 64) {      // (one entry a wavefront: written with the ballot above)
                    int tot = 0;
                    for (int w = 0; w < PF_BS / 64; ++w) tot += q.wint[2 * (PF_BS / 64) + w];
                    A.rg_blkcnt[(size_t)row_slot * gridDim_particles(A) * A.blk_gran + pf_bx()] = tot;
                }
                if (active) {
                    row_parent_in_chunk(A, q, sm, pch, stage_lo, nst, lhs, dn, p, d, a, first_copy, [&]() { PF_STAMP(20); });
                    // the offspring table of the generation that ends here, for the ledger (launch s + 1) and -arg
                    int* lo_tab = A.lo + (size_t)(G_end % A.Gcap) * (A.Np + 1);
                    lo_tab[p] = lo_p;
                    if (p == A.Np - 1) lo_tab[A.Np] = (int)A.Np;
                }
            }
        }
    } else {
        cur = c->cur;
        completing = fuse != 0;
        gather = fuse && c->flag;
        from_slot = gather ? (cur ^ 1) : cur;
        __syncthreads();
    }
    if constexpr (HEAD) {
        // the tables of the update loop go to LDS here, behind the decision: nothing before this point reads them
        if (threadIdx.x < PF_EPAD) {
            sT[threadIdx.x] = h_T; sH[threadIdx.x] = h_Hc;
            if ((int)threadIdx.x < E_head) sI[threadIdx.x] = h_I;
        }
        if (use_lut && threadIdx.x < 2 * PF_LUT_N / 4) s_lut[threadIdx.x] = h_lut;
#pragma unroll
        for (int r = 0; r < RTree<NM>::NI; ++r) {
            asm volatile("" : "+v"(t0.C0[r]), "+v"(t0.C1[r]));
            t0.C0[r] = (int)(int8_t)t0.C0[r]; t0.C1[r] = (int)(int8_t)t0.C1[r];
        }
        if (completing && s > PF_HL(H, s_begin)) {
            const double e = pf_arrive(sgp_start) + pf_arrive(sgp_len), Lq = A.L;       // sweep_seg_pos of row s - 1
            pos_prev = e < Lq ? e : Lq;
        } else pos_prev = 0.0;
    }
    if constexpr (PIPE) __syncthreads();
    PF_STAMP(3);
    // wave-uniform slots: indexed kernel arguments stay scalar loads (a lane-varying index would put them on the stack)
    cur = __builtin_amdgcn_readfirstlane(cur);
    from_slot = __builtin_amdgcn_readfirstlane(from_slot);
    double w_post = 0.0, w_pilot = 0.0;
    bool has_pending = false;
    if (active) {
        const DState st = state_slot(A, cur);
        const DState from = state_slot(A, from_slot);
        if constexpr (!PIPE) {
            a = gather ? (long long)A.parent[p] : p;
            // offspring offsets of this slot (as the old particle) and of its parent: requested with the parent index and
            // with the parent's state, not after them (each dependent request is a memory round trip of about 1 us)
            const int* lo_tab = A.lo + (size_t)((c->gen - 1 + A.Gcap) % A.Gcap) * (A.Np + 1);
            if (gather) { lo_p = lo_tab[p]; lo_p1 = lo_tab[p + 1]; first_copy = (p == lo_tab[a]); }
            inv = c->inv_T; S1v = c->S1; pos_prev = c->cur_pos;
            G_end = c->gen - 1; ev = (int)c->n_resample - 1;
        }
        RTree<NM> t;
        const bool reload = !PIPE || gather;           // PIPE: the slot's own state is already in registers
        if (!reload) t = t0;
        else {
#pragma unroll
            for (int r = 0; r < RTree<NM>::NI; ++r) {
                t.S[r] = 0.0; t.C0[r] = 0; t.C1[r] = 0;
                if (r < n - 1) {
                    t.S[r] = from.S[(size_t)r * A.Np + a];
                    t.C0[r] = from.C[(size_t)(2 * r) * A.Np + a];
                    t.C1[r] = from.C[(size_t)(2 * r + 1) * A.Np + a];
                }
            }
        }
        RCtx cx;
        const double v_L = in_vgpr(A.L), v_mu = in_vgpr(A.mu), v_rho = in_vgpr(A.rho);
        row_ctx<BIASED, TREES, PIPE>(cx, A, sT, sI, sH, sBH, sBS, n, p, v_L, v_mu, v_rho, use_lut, s_lut, PR.draws, o_tab_end);
        cx.ridx = cx.gK > 0 ? from.ridx[a] : 0;
        DStore ds;
        if (BIASED) {
            d_bind(ds, A, st, p);
            ds.count = from.dcount[a]; ds.total = from.total_delayed[a];
            if (gather || PIPE)   // the copy constructor copies the pending factors (particle.cpp:122-123); the ring moves them every row
                for (int k = 0; k < ds.count; ++k) {
                    st.dpos[(size_t)k * A.Np + p] = from.dpos[(size_t)k * A.Np + a];
                    st.dfac[(size_t)k * A.Np + p] = from.dfac[(size_t)k * A.Np + a];
                    st.ddelta[(size_t)k * A.Np + p] = from.ddelta[(size_t)k * A.Np + a];
                    st.dk[(size_t)k * A.Np + p] = from.dk[(size_t)k * A.Np + a];
                }
        }
        double next_base, x_mark;
        int mark_limit;
        unsigned widx;
        if (reload) {
            w_post = from.w_post[a];
            w_pilot = from.w_pilot[a];
            next_base = from.next_base[a];
            x_mark = from.x_mark[a];
            mark_limit = from.mark_limit[a];
            cx.Ltree = from.Ltree[a];
        } else {
            w_post = o_wpost; w_pilot = o_wpilot; next_base = o_next; x_mark = o_xmark; mark_limit = o_ml; cx.Ltree = o_Ltree;
        }
        [[maybe_unused]] double la_prev = 1.0;
        if constexpr (LOOK) la_prev = reload ? from.lookahead[a] : o_la;
        if constexpr (PIPE) { cx.ctr = o_ctr; cx.ebuf = o_ebuf; widx = o_widx; r_draws_prefetch(cx); }
        else { cx.ctr = A.rng_ctr[p]; cx.ebuf = A.ebuf[p]; widx = A.widx[p]; }
        if (completing) {
            if (!PIPE && p == 0) { Ctrl* cw = A.ctrl; cw->gen_prev = c->gen; cw->nres_prev = c->n_resample; }
            if (!gather) {
                w_post *= inv;                             // normalize_probability, pc.cpp:435-437
                w_pilot *= inv;
            } else {
                const int G = G_end;                       // the generation that ended with the previous row
                const double pos = pos_prev;
                const DState& src = from;
                // role of the old slot p: close its stretch if it has offspring
                if (lo_p1 > lo_p) {
                    double* rec = rec_ptr(A, p, widx);
                    row_close_record(rec, PIPE ? o_xmark : src.x_mark[p], pos, PIPE ? o_ml : src.mark_limit[p], n);
                    if constexpr (PIPE) {
#pragma unroll
                        for (int r = 0; r < RTree<NM>::NI; ++r) if (r < n - 1) rec[5 + r] = t0.S[r];
                    } else {
                        for (int r = 0; r < n - 1; ++r) rec[5 + r] = src.S[(size_t)r * A.Np + p];
                    }
                    ++widx;
                }
                A.gstart[(size_t)((G + 1) % A.Gcap) * A.Np + p] = widx;
                // role of the new slot p: weights of the copy (pc.cpp:350-351), fresh position for all but the first
                if (ev < A.max_trace_events) A.ev_parents[(size_t)ev * A.Np + p] = (int)a;
                row_copy_weights(w_post, w_pilot, inv, S1v, (double)A.Np);
                x_mark = pos;
                if (!first_copy && pos < v_L) {
                    next_base = r_sample_next_base<false>(cx, pos);     // pc.cpp:357-368
                    if constexpr (PIPE) r_draws_prefetch(cx);           // the counter moved: the request of the prologue is stale
                }
            }
        }

        PF_STAMP(4);
        const bool do_extend = !PIPE || PR.extend != 0;
        if constexpr (HEAD) {
            row_segment_arrive<NM, EXACT>(do_extend, n, sg_start, sg_len, sg_limit, sg_state, sg_allele);
        }
        const int8_t* data = A.seg_alleles + (size_t)s * n;
        double seg_end = 0.0;
        int limit = 0;
        if constexpr (PIPE) { if (do_extend) { seg_end = sg_start + sg_len; limit = sg_limit; } }
        else { if (do_extend) { seg_end = A.seg_start[s] + A.seg_len[s]; limit = A.seg_limit[s]; } }
        const double extend_to = seg_end < v_L ? seg_end : v_L;
        RowMasks rm;
        if (do_extend) rm = row_masks<NM>(n, [&](int i) { return PIPE ? sg_allele[i] : (int)data[i]; });
        const unsigned one_mask = rm.one, zero_mask = rm.zero, present_mask = rm.present, two_mask = rm.two;
        const int missing = rm.missing;
        int leaf_status = 0;
        if (missing == 0) leaf_status = 1;
        if (missing == n) leaf_status = -1;

        double updated_to = (PIPE && completing) ? pos_prev : c->cur_pos;
        if (!do_extend) updated_to = extend_to;             // completion only: the loop below does not run
        double B;
        if (leaf_status == -1) B = 0;
        else if (leaf_status == 1) B = cx.Ltree;
        else B = r_tracked_len(t, n, present_mask);

        PF_ACC_DECL;
        while (updated_to < extend_to) {
            PF_TICK(tk0);
            double new_to = extend_to < next_base ? extend_to : next_base;
            double f = fastexp(-v_mu * B * (new_to - updated_to));
            PF_TICK(tk0a);
            PF_ACC2(0, tk0, tk0a);
            w_post *= f;
            w_pilot *= f;
            if (BIASED && cx.gK > 0) {
                // importance_weight_over_segment (particle.cpp:1138-1181): true over guide rate for the stretch
                // without recombination
                double dist = new_to - updated_to;
                double target_rate = dist * v_rho * cx.Ltree;
                double sampled_rate = dist * cx.grho[cx.ridx] * cx.Ltree;
                double iws = fastexp(sampled_rate - target_rate);
                w_post *= iws;
                w_pilot *= iws;
            }
            updated_to = new_to;
            if (BIASED && cx.gK > 0 && updated_to < extend_to && cx.ridx + 1 < cx.gK && updated_to == cx.gpos[cx.ridx + 1]) {
                // reached a change of the guide rate: no genealogy change, new draw under the new rate
                // (particle.cpp:822-826); the open stretch continues
                cx.ridx += 1;
                next_base = r_sample_next_base<false>(cx, updated_to);
                if constexpr (PIPE) r_draws_prefetch(cx);
                continue;
            }
            PF_TICK(tk1);
            PF_ACC(0, tk0, tk1);
            PF_ACC2(1, tk0a, tk1);
            if (updated_to < extend_to) {
                row_update_trip<NM, BIASED, EXACT, TREES, PIPE>(A, cx, t, ds, p, n, limit, leaf_status, present_mask, updated_to, widx, x_mark, mark_limit, next_base, B,
                                                                w_post, w_pilot, sBH, sBS PF_ACC_ARGS);
            }
        }
        PF_ACC_STORE;

        PF_STAMP(5);
        // a fresh handle on the argument block (pf_reopen): what the rest of the row needs from it -- the pointers of the output
        // slot, the scan rings -- is loaded from here on and does not sit in scalar registers across the update loop
        const KA& A1 = pf_reopen(A);
        const DState st1 = state_slot(A1, cur);
        if (BIASED) {
            // apply the factors that fell due during this extension (particle.cpp:910-916)
            for (;;) {
                if (ds.count == 0 || !do_extend) break;
                double pm = ds.pos[0];
                for (int i = 1; i < ds.count; ++i) { double pi = ds.pos[(size_t)i * ds.Np]; if (pi < pm) pm = pi; }
                if (!(pm < extend_to)) break;
                d_apply_earliest(ds, w_pilot);
            }
            st1.dcount[p] = ds.count;
            st1.total_delayed[p] = ds.total;
            if (cx.gK > 0) st1.ridx[p] = cx.ridx;
            has_pending = ds.count > 0;
        }
        if (do_extend && (PIPE ? sg_state : (int)A1.seg_state[s]) == 0) {
            const double lik = row_site_lik<NM>(t, n, v_mu, one_mask, zero_mask, two_mask, A1.flags & 2, A1.flags & 1);
            w_post *= lik;
            w_pilot *= lik;
        }
        if constexpr (LOOK) {
            // removeLookaheadLikelihood + includeLookaheadLikelihood (particle.hpp:182, particle.cpp:614-616), as k_lookahead ends
            double la_w = la_prev;
            if (do_extend) {
                const double likelihood = look_factor<NM>(A1, t, n, s, cx.Ltree);
                w_pilot /= la_prev;
                la_w = 1.0;
                la_w *= likelihood;
                w_pilot *= likelihood;
            }
            st1.lookahead[p] = la_w;
        }

        PF_STAMP(6);
        row_store_tree<NM>(st1, (size_t)A1.Np, p, n, t);
        st1.w_post[p] = w_post;
        st1.w_pilot[p] = w_pilot;
        row_store_chain(A1, st1, p, next_base, x_mark, mark_limit, cx);
        if constexpr (PIPE) {
            row_store_counters(A1, PR, cur, p, cx.ctr, widx, do_extend);
        } else {
            A1.widx[p] = widx;
        }
        if (TREES && widx >= A1.cap) A1.ctrl->err = ERR_LOG_OVERFLOW;       // -arg keeps every record
        if constexpr (!PIPE) {
#pragma unroll
            for (int r = 0; r < RTree<NM>::NI; ++r) if (r < n - 1) A1.snap_S[A1.sp][(size_t)r * A1.Np + p] = t.S[r];
            A1.snap_w[A1.sp][p] = w_post; A1.snap_xm[A1.sp][p] = x_mark; A1.snap_ml[A1.sp][p] = mark_limit; A1.snap_widx[A1.sp][p] = widx;
        }
    }
    PF_STAMP(7);
    const KA& A2 = pf_reopen(A);
    const RowScans rs = row_scans(w_post, w_pilot, lane);
    const double sc = rs.sc, sp = rs.sp, sq = rs.sq, scp = rs.scp, scm = rs.scm;
    long long chunk = p >> 6;
    PF_STAMP(8);
    if constexpr (PIPE) {
        const size_t co = (size_t)cur * A2.nc;
        row_scans_store(A2, cur, p, active, lane, rs);
        if (BIASED) {
            unsigned long long pend = __ballot(has_pending);
            if (lane == 0 && chunk < A2.nc) {
                A2.rg_dpend[co + chunk] = __popcll(pend);
                if (!PR.extend) A2.chunk_dpend[chunk] = __popcll(pend);     // the state goes back to the general kernels
            }
        }
    } else {
        if (active) { A2.scan1[p] = sc; A2.scanp2[A2.sp][p] = scp; A2.scan1m[p] = scm; }
        if (lane == 63 && chunk < (A2.Np + 63) / 64) {
            A2.chunk_post[chunk] = sp;
            A2.chunk_sq[chunk] = sq;
            A2.chunk_pil[chunk] = sc;
            A2.chunk_pp[chunk] = scp;
            A2.chunk_mx1[chunk] = scm;
        }
        if (BIASED) {
            unsigned long long pend = __ballot(has_pending);
            if (lane == 0 && chunk < (A2.Np + 63) / 64) A2.chunk_dpend[chunk] = __popcll(pend);
        }
    }
}

#include "pf_pair.h"

template <int NM, bool BIASED, bool TREES = false>
__global__ __launch_bounds__(PF_BS) void k_extend_reg(KArgs A, long long s, int fuse) {
    extend_reg_body<NM, BIASED, false, TREES>(A, s, fuse);
}

// ------------------------------------------------------------------ count bookkeeping (shared)
// Ordered reduction of the k_count partials of the previous step into the totals
// (count.cpp:407-414).  Every k_count workgroup adds its step result to its own accumulator (same workgroup, same
// address, kernels in stream order: no race), so nothing has to be folded per row; k_count_fin folds the
// accumulators into the totals when the host asks for them (pf_sync).
#define PF_FIN_TILE_B 64       // k_count workgroup partials staged per pass
#define PF_FIN_PAIRS 64        // (epoch, statistic) pairs staged per pass

template <class KA>
__device__ void finalize_counts(const KA& A, Ctrl* c, int tid, int nthreads, double* stage /* PF_FIN_PAIRS*PF_FIN_TILE_B */) {
    const int E = A.E;
    const int nb = A.nbx;
    const int NC = A.ncol;
    const int npairs = E * NC;
    // All accumulators of a tile are fetched with independent loads (a serial load-add chain would pay the
    // full memory latency per term), then each pair is summed in workgroup order from LDS.
    for (int p0 = 0; p0 < npairs; p0 += PF_FIN_PAIRS) {
        const int np_ = npairs - p0 < PF_FIN_PAIRS ? npairs - p0 : PF_FIN_PAIRS;
        double run = 0.0;                                   // running sum of pair (p0 + tid), threads < np_
        for (int b0 = 0; b0 < nb; b0 += PF_FIN_TILE_B) {
            const int nbt = nb - b0 < PF_FIN_TILE_B ? nb - b0 : PF_FIN_TILE_B;
            for (int idx = tid; idx < np_ * nbt; idx += nthreads) {
                int pp = idx / nbt, b = idx % nbt;
                int pair = p0 + pp;
                int e = pair / NC, k = pair % NC;
                double* src = &A.partial[((size_t)e * A.nbx + b0 + b) * NC + k];
                stage[pp * PF_FIN_TILE_B + b] = *src;
                *src = 0.0;
            }
            __syncthreads();
            if (tid < np_)
                for (int b = 0; b < nbt; ++b) run += stage[tid * PF_FIN_TILE_B + b];
            __syncthreads();
        }
        if (tid < np_) {
            int pair = p0 + tid;
            int e = pair / NC, k = pair % NC;
            A.totals[(size_t)k * E + e] += run;
        }
    }
    __syncthreads();
    if (tid == 0) {
        c->first_epoch = E;
        c->count_active = 0;
        c->pending_fin = 0;
    }
    __syncthreads();
}

// generation bookkeeping for the windows of the coming count step: g_lo[e] / g_hi[e] = generations
// that hold the window ends (both monotone along the sweep: amortised O(1) per step)
template <class KA>
__device__ void window_generations(const KA& A, Ctrl* c, const Windows& W, int tid) {
    const int E = A.E;
    const int G = c->gen_prev;
    if (tid < E) {
        const int e = tid;
        int g = c->g_lo[e];
        while (g < G && A.gen_x0[(g + 1) % A.Gcap] <= W.a[e]) ++g;
        c->g_lo[e] = g;
        if (e >= W.first) {
            int h = c->g_hi[e];
            if (h < g) h = g;
            while (h < G && A.gen_x0[(h + 1) % A.Gcap] < W.b[e]) ++h;
            c->g_hi[e] = h;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int gr = c->g_lo[0];
        for (int e = 1; e < E; ++e) gr = c->g_lo[e] < gr ? c->g_lo[e] : gr;
        c->g_retain = gr;
        c->delayed_opp += W.b[E - 1] - W.a[E - 1];
        if (A.n_bias > 0 || A.g_K > 0) {
            // update_delayed_weight_count (count.cpp:395-397): particles that carry pending factors (a guide alone delays its
            // factors too: the extend kernels fill chunk_dpend whenever they run biased)
            long long npend = 0;
            const int ncq = (int)((A.Np + 63) / 64);
            for (int q = 0; q < ncq; ++q) npend += A.chunk_dpend[q];
            c->delayed_count += (double)npend * (W.b[E - 1] - W.a[E - 1]);
        }
        c->first_epoch = W.first;
        c->count_active = W.first < E;
        if (W.first < E) c->pending_fin = 1;
        c->nbx_used = A.nbx;
    }
}

// ------------------------------------------------------------------ k_decide
// normalize_probability (pc.cpp:420-438), the ESS test of resample (pc.cpp:247-283) and
// systematic_resampling (pc.cpp:474-504) -> offspring table, parent table, survivor run list.
//
// Grid = one workgroup per 256 particles + one bookkeeping workgroup.  A single workgroup has four
// SIMDs, far too few for anything per-particle, so:
//   * every particle workgroup redundantly redoes the tiny level-2/3 part of the canonical reduction
//     (<= 4096 per-wavefront partials): all of them obtain bit-identical T, S1, S2, ESS, flag, u without
//     any inter-workgroup wait;
//   * if resampling is due, each computes the final offspring offsets of its own particles (one per lane),
//     the parent table entries of their offspring and its survivor count: no inter-workgroup wait;
//   * the bookkeeping workgroup advances the window
//     generations (off the critical path).
template <class KA>
__device__ __forceinline__ void decide_body(const KA& A, long long s, int mode, const Windows& W, int nblocks) {
    __shared__ double l2s[4096];          // level-2 inclusive scan of the per-wavefront pilot totals / finalize staging
    __shared__ double l2_post[64], l2_sq[64], l2_tot[64], l2_totp[64];
    __shared__ int wred[PF_BS / 64];
    __shared__ double wredd[PF_BS / 64];
    __shared__ int slo[PF_BS];
    __shared__ double pm[4096];           // exclusive prefix max over chunks of the pilot prefix sums
    Ctrl* c = A.ctrl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = PF_BS / 64;
    if (pf_bx() == nblocks) {
        window_generations(A, c, W, tid);
        return;
    }
    const long long Np = A.Np;
    const int nc = (int)((Np + 63) / 64);
    const int ng = (nc + 63) / 64;
    const double last_scan1 = A.scan1[Np - 1];
    const long long i_own = (long long)pf_bx() * PF_BS + tid;
    const double own_scan1m = (i_own > 0 && i_own < Np) ? A.scan1m[i_own - 1] : 0.0;
    const double next_scan1m = (i_own + 1 < Np) ? A.scan1m[i_own] : 0.0;
    // generation / event counters as published by the previous k_resample: workgroup 0 advances the live ones
    // at the end of this kernel while other workgroups may still be starting
    const int G = c->gen_prev;
    const unsigned long long n_res = (unsigned long long)c->nres_prev;
    // level 2 of the canonical radix-64 reduction / scans
    for (int g = wave; g < ng; g += nwaves) {
        int ch = g * 64 + lane;
        double vp = ch < nc ? A.chunk_post[ch] : 0.0;
        double vs = ch < nc ? A.chunk_sq[ch] : 0.0;
        double vl = ch < nc ? A.chunk_pil[ch] : 0.0;
        double vq = ch < nc ? A.chunk_pp[ch] : 0.0;
        double rp = wave_tree_sum(vp);
        double rs = wave_tree_sum(vs);
        double sc = wave_hs_scan(vl, lane);
        double scq = wave_hs_scan(vq, lane);
        if (ch < nc) { l2s[ch] = sc; if (pf_bx() == 0) A.l2scanp[ch] = scq; }
        if (lane == 63) { l2_post[g] = rp; l2_sq[g] = rs; l2_tot[g] = sc; l2_totp[g] = scq; }
    }
    __syncthreads();
    // level 3, redundantly in every thread (at most 64 group totals): no further barrier needed
    double T, S2;
    {
        double vp = lane < ng ? l2_post[lane] : 0.0;
        double vs = lane < ng ? l2_sq[lane] : 0.0;
        T = wave_tree_sum(vp);
        S2 = wave_tree_sum(vs);
    }
    auto chunk_offset = [&](int ch) -> double {
        double run = 0.0;
        const int gq = ch / 64;
        for (int g = 0; g < gq; ++g) run = run + l2_tot[g];
        double off = (ch % 64 == 0) ? 0.0 : l2s[ch - 1];
        return run + off;
    };
    if (pf_bx() == 0) {
        for (int ch = tid; ch < nc; ch += PF_BS) {
            A.chunk_off[ch] = chunk_offset(ch);
            double runp = 0.0;
            for (int g = 0; g < ch / 64; ++g) runp = runp + l2_totp[g];
            double offp = (ch % 64 == 0) ? 0.0 : A.l2scanp[ch - 1];
            A.chunk_offp2[A.sp][ch] = runp + offp;
        }
    }
    const double S1 = chunk_offset(nc - 1) + last_scan1;   // inclusive scan at the last particle (= oracle incl[N-1])
    const double ess = (S1 * S1) / S2;
    const int flag = (mode == 0 && ess < A.ess_threshold - 1e-6) ? 1 : 0;
    double pos = A.L;
    if (mode == 0) {
        double seg_end = A.seg_start[s] + A.seg_len[s];
        pos = seg_end < A.L ? seg_end : A.L;
    }
    const double u = flag ? philox_uniform(A.seed, 0xFFFFFFFFu, 1, n_res) : 0.0;
    if (pf_bx() == 0 && tid == 0) {
        if (!(T > 0.0) && !c->err) c->err = ERR_ZERO_PROB;       // the first error is the one reported
        double logl = c->logl + dlog(T);
        c->logl = logl;
        double inv = 1.0 / T;
        if (mode == 0) {
            A.tr_T[s] = T;
            A.tr_ess[s] = ess;
            A.tr_flag[s] = flag;
            A.tr_logl[s] = logl;
            c->cur_pos = pos;
        }
        c->T = T; c->inv_T = inv; c->S1 = S1; c->S2 = S2; c->ess = ess; c->u = u; c->flag = flag;
        c->step[A.sp].inv_T = inv; c->step[A.sp].G = G; c->step[A.sp].flag = flag;
    }
    if (!flag) return;

    // ---- systematic resampling (pc.cpp:474-504) in closed form, one particle per lane, no inter-workgroup wait ----
    // lo[i] = max_{j<=i} lo_raw(incl[j-1]),  lo_raw(x) = #{ j in [0,N) : (j+u) * S1 < N * x }  (pc.cpp:491 scaled by
    // N*S1: no division).  lo_raw is monotone in x, so the running max can be taken on the prefix sums instead:
    // max_{j<=m} incl[j] = max( max_{c'<c} (chunk_off[c'] + mx1[c']),  chunk_off[c] + runmax(scan1)[m] ), which every
    // workgroup derives from the per-wavefront summaries alone.
    const double dn = (double)Np;
    const double invS1 = 1.0 / S1;
    {
        const int perc = (nc + PF_BS - 1) / PF_BS;
        const int c0 = tid * perc, c1 = c0 + perc < nc ? c0 + perc : nc;
        double run = 0.0;
        for (int ch = c0; ch < c1; ++ch) { double vch = chunk_offset(ch) + A.chunk_mx1[ch]; run = vch > run ? vch : run; }
        double scd = wave_max_scan_d(run, lane);
        if (lane == 63) wredd[wave] = scd;
        __syncthreads();
        double pre = 0.0;
        for (int w = 0; w < wave; ++w) pre = wredd[w] > pre ? wredd[w] : pre;
        double before = wave_prev_lane(scd, scd);
        if (lane > 0) pre = before > pre ? before : pre;
        run = pre;                           // exclusive prefix for this thread's first chunk
        for (int ch = c0; ch < c1; ++ch) {
            pm[ch] = run;
            double vch = chunk_offset(ch) + A.chunk_mx1[ch];
            run = vch > run ? vch : run;
        }
        __syncthreads();
    }
    auto lo_at = [&](long long i, double s1m) -> int {      // final offspring offset of particle i (0 < i < Np)
        const int ch = (int)((i - 1) >> 6);
        double incl = chunk_offset(ch) + s1m;
        double pmx = pm[ch];
        incl = pmx > incl ? pmx : incl;
        double rhs = dn * incl;
        double guess = floor(rhs * invS1 - u);
        long long g = guess < 0 ? 0 : (guess > dn ? Np : (long long)guess);
        while (g > 0 && !((((double)(g - 1)) + u) * S1 < rhs)) --g;
        while (g < Np && ((((double)g) + u) * S1 < rhs)) ++g;
        return (int)g;
    };
    int* lo = A.lo + (size_t)(G % A.Gcap) * (Np + 1);
    int lo_i = 0, lo_n = 0;
    const bool act = i_own < Np;
    if (act) {
        lo_i = i_own > 0 ? lo_at(i_own, own_scan1m) : 0;
        lo[i_own] = lo_i;
        slo[tid] = lo_i;
    }
    __syncthreads();
    int cnt = 0;
    if (act) {
        if (i_own + 1 >= Np) { lo_n = (int)Np; lo[Np] = (int)Np; }
        else if (tid + 1 < PF_BS) lo_n = slo[tid + 1];
        else lo_n = lo_at(i_own + 1, next_scan1m);          // first particle of the next workgroup (recomputed)
        cnt = lo_n - lo_i;
        for (int q = lo_i; q < lo_n; ++q) A.parent[q] = (int)i_own;
    }
    // survivors per workgroup (k_resample turns them into the run list of the ending generation)
    unsigned long long bal = __ballot(cnt > 0);
    if (lane == 0) wred[wave] = __popcll(bal);
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < nwaves; ++w) tot += wred[w];
        A.blkcnt2[A.sp][pf_bx()] = tot;
        if (pf_bx() == 0) {
            // toggle buffers / open the next generation
            int ev = (int)n_res;
            if (ev < A.max_trace_events) A.ev_seg[ev] = (int)s;
            c->cur ^= 1;
            c->gen = G + 1;
            A.gen_x0[(G + 1) % A.Gcap] = pos;
            c->n_resample = (long long)n_res + 1;
            if (G + 1 - c->g_retain >= A.Gcap - 1) c->err = ERR_GEN_OVERFLOW;
            if (A.rec_trees && G + 2 >= A.Gcap) c->err = ERR_GEN_OVERFLOW;      // -arg keeps every generation
        }
    }
}

// ------------------------------------------------------------------ k_count
// update_all_counts_single_evolevent (count.cpp:495-555) evaluated from the compact per-slot
// records.  blockIdx.y = epoch; the x dimension strides over the live ancestors (runs of the
// composite ancestor maps) of every generation whose positions intersect the epoch's window.
// per-thread statistics of one epoch: [coal count, opp, weight][P], recomb count, opp, weight and -- for
// structured models -- [migration count][P][P], [migration opp, weight][P]  (count.hpp:95-110)
// NC columns in this order are what a workgroup adds to its accumulator (KArgs::partial) and what pf_get_counts reads.
// More than PF_PMAX populations (MIG_LDS, the instance of PF_PWIDE): a thread keeps the per-population statistics only -- NR = 5P + 3 = 43
// doubles at P = 8, next to the 39 of P = 4 -- and the P x P migration counts, which would make it 107 doubles (214 VGPRs before anything
// else), are collected per workgroup in LDS (count_mig) and meet the others at the workgroup's reduction.  CC .. RW, MO, MW index v[];
// MC is the first column of the migration counts in both arrangements, and the reduction of count_body puts v[k] behind them for k >= MC.
template <int P>
struct AccT {
    static constexpr bool MIG_LDS = P > PF_PMAX;
    static constexpr int NC = P == 1 ? 6 : 3 * P + 3 + P * P + 2 * P;
    static constexpr int NR = MIG_LDS ? NC - P * P : NC;
    static constexpr int CC = 0, CO = P, CW = 2 * P, RC = 3 * P, RO = 3 * P + 1, RW = 3 * P + 2;
    static constexpr int MC = 3 * P + 3, MO = 3 * P + 3 + (MIG_LDS ? 0 : P * P), MW = MO + P;
    double v[NR];
};
// the migration counts of a count workgroup of the PF_PWIDE instance: [from][to], zeroed at its entry, added to with ds_add_f64
// (the address space is in the pointer's type, as in lmap_add: a flat atomic would find out per lane)
typedef __attribute__((address_space(3))) double pf_lds_double;
__device__ __forceinline__ double* count_mig() {
    __shared__ double mig[PF_PWIDE * PF_PWIDE];
    return mig;
}

__device__ __forceinline__ double ovl(double a0, double a1, double b0, double b1) {
    double lo = a0 > b0 ? a0 : b0;
    double hi = a1 < b1 ? a1 : b1;
    double d = hi - lo;
    return d > 0.0 ? d : 0.0;
}

// sum_i (nl - i) * |[S_{i-1}, S_i] n [max(T0,lo_t), min(T1,hi_t)]|, optionally including the single
// lineage above the top node (coalescence paths).  S lives in registers (NI compile-time).
template <int NI>
__device__ __forceinline__ double slice_len(const double (&S)[NI], int nint, int nl, double T0, double T1, double lo_t,
                                            double hi_t, bool above_top) {
    double a = T0 > lo_t ? T0 : lo_t;
    double b = T1 < hi_t ? T1 : hi_t;
    if (!(b > a)) return 0.0;
    double acc = 0.0, prev = 0.0;
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (i < nint) {
            double top = S[i];
            acc += (double)(nl - i) * ovl(prev, top, a, b);
            prev = top;
        }
    if (above_top) acc += (double)(nl - nint) * ovl(prev, PF_INF, a, b);
    return acc;
}

// (dead: ancient samples -- the part of slice_len's answer for the whole epoch that does not exist yet, KArgs::anc; 0.0, known when the kernel is
// compiled, in every count body but that of k_count_anc)
struct Win { int e, rf; double T0, T1, a_e, b_e; bool end_seq; double dead; };

// local recombination map (record_local_recomb_events, count.cpp:559-613): per workgroup the differential
// opportunity of its window is collected in LDS bins and flushed with one global atomic per touched bin
#define PF_LBINS 2048
struct LMap {
    double* lds;          // [PF_LBINS] bins of this workgroup, bin 0 = interval b0
    int nlds;             // bins in use: the window of the step spans few of them (the rest of a step's additions, if any, go to memory)
    long long b0;
    double* gopp;         // global differential opportunity (null: map not recorded)
    double* gcnt;         // global counts [(n+2)][nbins]
    long long nbins;
    int ncnt;             // bins whose (n+2) count rows are collected in LDS too, behind the nlds opportunity bins (0: the counts go to memory)
};
__device__ __forceinline__ void lmap_add(const LMap& L, long long idx, double v) {
    if (idx < 0 || idx >= L.nbins) return;
    long long k = idx - L.b0;
    // the bins are LDS: said in the pointer's type, so that the addition is a ds_add_f64 and not a flat atomic that finds out per lane
    typedef __attribute__((address_space(3))) double lds_double;
    if (k >= 0 && k < L.nlds) __hip_atomic_fetch_add((lds_double*)L.lds + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else atomicAdd(&L.gopp[idx], v);
}
// constant opportunity density over [x_lo, x_hi): the differential encoding of count.cpp:578-588.  When the stretch spans more than one
// interval the two additions at its left end depend on (x_lo, density) only and the two at its right end on (x_hi, density) only.
__device__ __forceinline__ void lmap_left(const LMap& L, double x_lo, double dens) {
    const double iv = 100.0;
    const long long first = (long long)(x_lo / iv);
    const double fi = (double)(first + 1) * iv - x_lo;
    lmap_add(L, first, fi * dens);
    lmap_add(L, first + 1, (iv - fi) * dens);
}
__device__ __forceinline__ void lmap_right(const LMap& L, double x_hi, double dens) {
    const double iv = 100.0;
    const long long last = (long long)(1 + x_hi / iv);
    const double li = x_hi - (double)(last - 1) * iv;
    lmap_add(L, last - 1, (li - iv) * dens);
    lmap_add(L, last, -(li * dens));
}
__device__ __forceinline__ void lmap_opportunity(const LMap& L, double x_lo, double x_hi, double weight, double opp) {
    const double iv = 100.0;
    long long first = (long long)(x_lo / iv);
    long long last = (long long)(1 + x_hi / iv);
    double dens = weight * opp / (x_hi - x_lo);
    if (first == last - 1) {
        double top = (double)(first + 1) * iv;
        double first_interval = (top < x_hi ? top : x_hi) - x_lo;
        lmap_add(L, first, first_interval * dens);
        lmap_add(L, first + 1, -(first_interval * dens));
    } else {
        // (keeping the densities of the ends that coincide with the window's -- most of them -- in two registers per lane and adding them
        // once per wavefront was measured: slower, 3.29e4 -> 3.20e4 segments/s for one chunk, the registers cost more than the conflicts)
        lmap_left(L, x_lo, dens);
        lmap_right(L, x_hi, dens);
    }
}
// a recombination event at event_base, height h, below which the samples `desc` hang (count.cpp:590-612)
// (M: the 32-bit masks of the records' meta word, or the 64-bit word of a record written by the wide kernels)
template <class M>
__device__ __forceinline__ void lmap_event(const LMap& L, int n, double event_base, double h, M desc, double weight) {
    long long idx = (long long)(event_base / 100.0);
    if (idx < 0 || idx >= L.nbins) return;
    const int nd = sizeof(M) == 8 ? __popcll((unsigned long long)desc) : __popc((unsigned)desc);
    const long long k = idx - L.b0;
    if (k >= 0 && k < L.ncnt) {
        // the workgroup's own rows of the counts: a row's events all fall into the few intervals of its epoch's window, and every one
        // of them used to be n + 2 additions on memory, to the same handful of addresses as everybody else's
        typedef __attribute__((address_space(3))) double lds_double;
        lds_double* base = (lds_double*)L.lds + L.nlds + k;
        for (int i = 0; i < n; ++i)
            if ((desc >> i) & (M)1) __hip_atomic_fetch_add(base + (size_t)i * L.ncnt, weight / nd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(base + (size_t)n * L.ncnt, weight * h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(base + (size_t)(n + 1) * L.ncnt, weight * dlog(h + 1.0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
    for (int i = 0; i < n; ++i)
        if ((desc >> i) & (M)1) atomicAdd(&L.gcnt[(size_t)i * L.nbins + idx], weight / nd);
    atomicAdd(&L.gcnt[(size_t)n * L.nbins + idx], weight * h);
    atomicAdd(&L.gcnt[(size_t)(n + 1) * L.nbins + idx], weight * dlog(h + 1.0));
}

template <int NI, int P, class KA>
__device__ __forceinline__ void stretch_contrib(AccT<P>& acc, const KA& A, const Win& W, const LMap& L, double w, double x0,
                                                double x1, const double (&S)[NI], int lim_start) {
    if (!(W.rf & REC_RECOMB) || W.e > lim_start) return;
    double xs = ovl(x0, x1, W.a_e, W.b_e);
    if (!(xs > 0.0)) return;
    double len = slice_len<NI>(S, A.n - 1, A.n, W.T0, W.T1, 0.0, PF_INF, false) - W.dead;
    // a tree that does not reach the epoch has no opportunity there: nothing to add to the sums (adding zero leaves them as
    // they are) and nothing to the map -- most (record, epoch) pairs of the old epochs, whose windows hold the most records
    if (!(len > 0.0)) return;
    double opp = len * xs;
    acc.v[AccT<P>::RO] += w * opp;
    acc.v[AccT<P>::RW] += w * w * opp;
    if (L.gopp) lmap_opportunity(L, x0 > W.a_e ? x0 : W.a_e, x1 < W.b_e ? x1 : W.b_e, w, opp);
}

// What one record adds to the sums of one epoch window (update_all_counts_single_evolevent, count.cpp:495-555): f0..f4 are the
// record's head [x0, x1, h, t_c | piece reference, meta], S the heights of the tree in force over [x0, x1].
template <int NI, int P, class KA>
__device__ __forceinline__ void record_contrib_one(AccT<P>& acc, const KA& A, const Win& W, const LMap& L, double w, long long a,
                                                   double f0, double f1, double f2, double f3, double f4, const double (&S)[NI],
                                                   unsigned long long desc_wide = 0) {
    using AC = AccT<P>;
    const int n = A.n;
    double x0 = f0, x1 = f1;
    if (x1 < W.a_e) return;        // consumed by earlier windows
    unsigned long long meta = (unsigned long long)__double_as_longlong(f4);
    int type = (int)(meta & 0xff);
    int lim_start = (int)((meta >> 8) & 0xff) - 1;
    int lim_event = (int)((meta >> 16) & 0xff) - 1;
    int n_eff = (int)((meta >> 24) & 0xff);
    if (type <= 1) stretch_contrib<NI, P>(acc, A, W, L, w, x0, x1, S, lim_start);
    if (type == 0 || type == 2) {
        double h = f2;
        bool inwin = (W.a_e <= x1) && (x1 < W.b_e);
        if constexpr (P == 1) {
            double tc = f3;
            if (inwin && (W.rf & REC_COALMIGR) && W.e <= lim_event && tc >= W.T0 && h < W.T1) {      // (the floating lineage's path [h, t_c] meets the epoch)
                double opp = slice_len<NI>(S, n_eff - 1, n_eff, W.T0, W.T1, h, tc, true);
                acc.v[AC::CO] += w * opp;
                acc.v[AC::CW] += w * w * opp;
                if (W.T0 <= tc && tc < W.T1) acc.v[AC::CC] += w;
            }
        } else {
            // structured models: the walk of the update left pieces (pf_mp.h PLog) -- population, partners, [t0, t1),
            // event at t1 -- that are clipped to this epoch here; record flags and the epoch limit as above
            (void)n_eff;
            // without a tree dump the record says which epochs its pieces touch (piece_span, pf_mp.h)
            const unsigned span = (unsigned)((meta >> 48) & 0xffff);
            const bool elsewhere = !A.rec_trees && (span & 0x1000u) && (W.e < (int)(span & 63u) || W.e > (int)((span >> 6) & 63u));
            if (inwin && (W.rf & REC_COALMIGR) && W.e <= lim_event && !elsewhere) {
                unsigned long long ref = (unsigned long long)__double_as_longlong(f3);
                unsigned pstart = (unsigned)(ref & 0xffffffffu), np_ = (unsigned)(ref >> 32);
                if (A.pidx[a] - pstart > A.pcap || np_ > A.pcap) { if (!A.ctrl->err) A.ctrl->err = ERR_LOG_OVERFLOW; np_ = 0; }
                for (unsigned j = 0; j < np_; ++j) {
                    const double* q = A.plog + ((size_t)a * A.pcap + ((pstart + j) % A.pcap)) * 3;
                    long long tag = __double_as_longlong(q[0]);
                    const double t0 = q[1], t1 = q[2];
                    const int pop = (int)(tag & 0xff), kind = (int)((tag >> 8) & 0xff), to = (int)((tag >> 16) & 0xff);
                    const double lo = t0 > W.T0 ? t0 : W.T0, hi = t1 < W.T1 ? t1 : W.T1;
                    const double mo = hi > lo ? hi - lo : 0.0;
                    const bool ev = (kind & 3) != 0 && W.T0 <= t1 && t1 < W.T1;
                    if (!(mo > 0.0) && !ev) continue;
                    const double co = (double)((tag >> 24) & 0xff) * mo;
#pragma unroll
                    for (int pp = 0; pp < P; ++pp)
                        if (pp == pop) {
                            acc.v[AC::CO + pp] += w * co;
                            acc.v[AC::CW + pp] += w * w * co;
                            acc.v[AC::MO + pp] += w * mo;
                            acc.v[AC::MW + pp] += w * w * mo;
                            if (ev && (kind & 1)) acc.v[AC::CC + pp] += w;
                            if (ev && (kind & 2)) {
                                if constexpr (AC::MIG_LDS) {
                                    if (to < P) __hip_atomic_fetch_add((pf_lds_double*)count_mig() + pp * P + to, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                } else {
#pragma unroll
                                for (int qq = 0; qq < P; ++qq)
                                    if (qq == to) acc.v[AC::MC + pp * P + qq] += w;
                                }
                            }
                        }
                }
            }
        }
        if (type == 0) {
            bool inwin_r = (W.a_e <= x1) && ((x1 < W.b_e) || W.end_seq);
            if (inwin_r && (W.rf & REC_RECOMB) && W.e <= lim_event && W.T0 <= h && h < W.T1) {
                acc.v[AC::RC] += w;
                if constexpr (NI >= PF_NMAX) { if (L.gopp) lmap_event(L, n, x1, h, desc_wide, w); }     // the wide kernels' records
                else { if (L.gopp) lmap_event(L, n, x1, h, (unsigned)((meta >> 32) & 0xffff), w); }
            }
        }
    }
}

// All fields of a record are fetched in one round of independent loads before anything is tested:
// the kernel is bound by dependent-load latency, not by bytes.
template <int NI, int P, class KA>
__device__ __forceinline__ void records_contrib(AccT<P>& acc, const KA& A, const Win& W, const LMap& L, double w, long long a,
                                                unsigned k0, unsigned k1) {
    const int n = A.n;
    // A slot appends its records in the order of their positions.  Those that end before the window were consumed by earlier windows
    // (record_contrib_one's first test), those that start at or behind its end add nothing yet: on a row that lies thirty rows behind
    // the last resampling a live particle has twenty records of which the window of an old epoch meets one, and the lane with the most
    // records is what its wavefront waits for.  So the first record that can matter is looked for with three probes at a time
    // (independent loads: a round trip narrows the range to a quarter), and the walk stops at the first record past the window.
    unsigned lo = k0, len = k1 - k0;
    while (len > 4) {
        const unsigned q = len >> 2;
        const double xa = rec_ptr(A, a, lo + q)[1], xb = rec_ptr(A, a, lo + 2 * q)[1], xc = rec_ptr(A, a, lo + 3 * q)[1];
        // (x1 does not decrease along the records: the first one with x1 >= a_e lies behind every probe that is still below a_e)
        if (xc < W.a_e) { lo += 3 * q + 1; len -= 3 * q + 1; }
        else if (xb < W.a_e) { lo += 2 * q + 1; len = q; }
        else if (xa < W.a_e) { lo += q + 1; len = q; }
        else len = q;
    }
    for (unsigned k = lo; k != k1; ++k) {
        const double* rec = rec_ptr(A, a, k);
        double f0 = rec[0], f1 = rec[1], f2 = rec[2], f3 = rec[3], f4 = rec[4];
        double S[NI];
#pragma unroll
        for (int r = 0; r < NI; ++r) S[r] = r < n - 1 ? rec[5 + r] : 0.0;
        if (f0 >= W.b_e && !W.end_seq) break;           // this record and all behind it start past the window
        unsigned long long dw = 0;
        if constexpr (NI >= PF_NMAX) if (L.gopp) dw = (unsigned long long)__double_as_longlong(rec[4 + n]);
        record_contrib_one<NI, P>(acc, A, W, L, w, a, f0, f1, f2, f3, f4, S, dw);
    }
}

// Where a count step finds the particles of its row and the ancestor maps in force.  The general kernels keep these by
// step parity (snapshots written by k_extend) and update the run lists in place; the single-launch pipeline reads the
// row's slot of the state ring and the run-list copy that was in force for the row.
struct RunLists { int* st; int* anc; int* nruns; };
struct CountSrc {
    const double* w; const double* S; const double* xm; const int* ml; const unsigned* widx;   // the row's live particles
    const unsigned* widx_live;                    // records appended per slot as of now (ring-overwrite check)
    const double* scanp; const double* offp;      // posterior scan inside the wavefronts, exclusive offsets of the wavefronts
    RunLists lists;
    double inv; int G, g_lo, g_hi;                // normalisation of the row, its generation, generations of the epoch's window
};
template <class KA>
__device__ __forceinline__ RunLists run_lists(const KA& A, int ver) {
    RunLists r;
    r.st = ver ? A.run_st2 : A.run_st; r.anc = ver ? A.run_anc2 : A.run_anc; r.nruns = ver ? A.nruns2 : A.nruns;
    return r;
}
template <class KA>
__device__ __forceinline__ CountSrc count_src_parity(const KA& A, int sp, int e) {
    const Ctrl* c = A.ctrl;
    CountSrc q;
    q.w = A.snap_w[sp]; q.S = A.snap_S[sp]; q.xm = A.snap_xm[sp]; q.ml = A.snap_ml[sp]; q.widx = A.snap_widx[sp];
    q.widx_live = A.widx;
    q.scanp = A.scanp2[sp]; q.offp = A.chunk_offp2[sp];
    q.lists = run_lists(A, c->lver);
    q.inv = c->step[sp].inv_T; q.G = c->step[sp].G;
    q.g_lo = e < A.E ? c->g_lo[e] : 0; q.g_hi = e < A.E ? c->g_hi[e] : 0;
    return q;
}

// LDS bins of the local recombination map: one array for whichever count body the workgroup runs
__device__ __forceinline__ double* count_bins() {
    __shared__ double bins[PF_LBINS];
    return bins;
}

// LDS of a count role: one buffer per body (only the launch of the split arrangement carries both bodies)
#define PF_COUNT_LDS_BYTES 14336
template <int BYTES>
__device__ __forceinline__ char* count_lds() {
    __shared__ __attribute__((aligned(16))) char buf[BYTES];
    return buf;
}

#define PF_CNT_TILE 2048      // generations whose run counts are staged in LDS at a time
#define PF_CNT_WIDE 128       // run lists longer than this are strided over by the whole grid column
#define PF_CNT_BATCH 2        // count tasks whose first two rounds of loads a thread has in flight together

template <int NI, int P, class KA>
__device__ __forceinline__ void count_run(AccT<P>& acc, const KA& A, const CountSrc& Q, const Win& W, const LMap& L, int g, long long i,
                                          int nr, const int* rst, const int* ran, double inv) {
    const long long Np = A.Np;
    int q0 = rst[i];
    int q1 = i + 1 < nr ? rst[i + 1] : (int)Np;
    long long a = ran[i];
    // a ledger ring that has overflowed (reported by k_decide, ERR_GEN_OVERFLOW) aliases generations: whatever is
    // read then must at least stay inside the arrays and every loop must stay bounded until the host sees the error
    if (q1 <= q0 || q1 > (int)Np || q0 < 0 || a < 0 || a >= Np) return;
    // posterior mass of the descendants of (g, a): difference of the inclusive posterior scan
    const double* offp = Q.offp;
    const double* scp_ = Q.scanp;
    double hi = offp[(q1 - 1) >> 6] + scp_[q1 - 1];
    double lo = q0 > 0 ? offp[(q0 - 1) >> 6] + scp_[q0 - 1] : 0.0;
    double w = (hi - lo) * inv;
    if (!(w > 0.0)) return;
    unsigned k0 = A.gstart[(size_t)(g % A.Gcap) * Np + a];
    unsigned k1 = A.gstart[(size_t)((g + 1) % A.Gcap) * Np + a];
    if (Q.widx_live[a] - k0 > A.cap || k1 - k0 > A.cap) { if (!A.ctrl->err) A.ctrl->err = ERR_LOG_OVERFLOW; return; }
    records_contrib<NI, P>(acc, A, W, L, w, a, k0, k1);
}

// LDS of the flattened record walk of count_body: the weight, slot and first record of the task each thread found in a trip, and the
// exclusive prefix sum of the tasks' record counts
struct FlatTask { double w; int a; unsigned k0; };
__device__ __forceinline__ FlatTask* count_flat_tasks() {
    __shared__ FlatTask ft[PF_BS];
    return ft;
}
__device__ __forceinline__ int* count_flat_prefix() {
    __shared__ int pre[PF_BS + 1];
    return pre;
}

// The body of k_count for the workgroup (bx, by) of a column of nbxg workgroups; `sp` = parity of the step whose
// weights and snapshot it reads.  Called from k_count and from the count workgroups of k_row.
// ACC_AT_ENTRY (k_sweep_blc4): the workgroup's accumulator -- it belongs to the position (e, bx), and the launches that write it are serial on one
// stream -- is requested here, with the first loads, and not read, added to and written back behind the last sum, where the round trip of
// the read was the tail of every count workgroup.  The same addition on the same two numbers; a workgroup that leaves early stores nothing.
// ANC (k_count_anc): the model has sample times; the recombination opportunity of a record leaves out the length of the samples that enter later.
template <int NM, int P, bool EXACT = false, bool ACC_AT_ENTRY = false, bool ANC = false, class KA>
__device__ __forceinline__ void count_body(const KA& A, const CountSrc& Q, int e, double win_a, double win_b, int bx, int nbxg) {
    constexpr int NI = NM - 1;
    using AC = AccT<P>;
    double acc_before = 0.0;
    if constexpr (ACC_AT_ENTRY) { if (threadIdx.x < AC::NC) acc_before = A.partial[((size_t)e * A.nbx + bx) * AC::NC + threadIdx.x]; }
    constexpr int LDS_BYTES = (int)(((sizeof(AC) * (PF_BS / 64) + 15) & ~(size_t)15) + sizeof(int) * (PF_CNT_TILE + 1 + PF_BS / 64) + 16);
    char* const cl = count_lds<LDS_BYTES>();
    AC* const red = (AC*)cl;
    int* const s_off = (int*)(cl + ((sizeof(AC) * (PF_BS / 64) + 15) & ~(size_t)15));
    int* const s_wsum = s_off + PF_CNT_TILE + 1;
    const long long Np = A.Np;
    const int n = EXACT ? NM : A.n;
    const int G = Q.G;                                  // the generation the weights belong to
    const double inv = Q.inv;
    Win W;
    W.e = e; W.rf = A.recflags[e];
    W.T0 = A.T[e]; W.T1 = e + 1 < A.E ? A.T[e + 1] : PF_INF;
    W.a_e = win_a; W.b_e = win_b;
    W.end_seq = (A.L == W.b_e);
    if constexpr (ANC) W.dead = A.anc[A.n + e]; else W.dead = 0.0;
    double* const s_lbins = count_bins();
    LMap L;
    L.lds = s_lbins; L.b0 = (long long)(W.a_e / 100.0); L.gopp = A.lmap_opp; L.gcnt = A.lmap_cnt; L.nbins = A.lmap_bins;
    {
        const long long span = (long long)(W.b_e / 100.0) - L.b0 + 4;
        L.nlds = span < 1 ? 1 : (span > PF_LBINS ? PF_LBINS : (int)span);
        L.ncnt = (A.n + 3) * L.nlds <= PF_LBINS ? L.nlds : 0;       // room for the n + 2 count rows of the same intervals
    }
    bool bins_ready = false;
    const int g_lo = Q.g_lo, g_hi = Q.g_hi;
    if (g_hi < g_lo) return;                                  // an empty window: nothing to add to this workgroup's accumulators
    const int lane = threadIdx.x & 63;
    const long long gtid = (long long)bx * PF_BS + threadIdx.x;
    const long long nthreads = (long long)nbxg * PF_BS;
    AC acc;
#pragma unroll
    for (int k = 0; k < AC::NR; ++k) acc.v[k] = 0.0;
    if constexpr (AC::MIG_LDS) { if (threadIdx.x < P * P) count_mig()[threadIdx.x] = 0.0; }       // (the barrier that opens the first tile is between this and the first addition)
    // Work = all (generation, run) pairs of the window plus the live particles, flattened into one task index
    // space with an LDS prefix sum of the run counts: every thread takes tasks gtid, gtid+nthreads, ... so deep
    // windows are spread over the grid column instead of being walked generation by generation.
    for (int tile_hi = g_hi; tile_hi >= g_lo; tile_hi -= PF_CNT_TILE) {
        const int tile_lo = tile_hi - PF_CNT_TILE + 1 > g_lo ? tile_hi - PF_CNT_TILE + 1 : g_lo;
        const int ntile = tile_hi - tile_lo + 1;
        __syncthreads();
        // stage run counts (live generation: Np tasks) and their exclusive prefix sum
        constexpr int PER = PF_CNT_TILE / PF_BS;
        int loc[PER];
        int lsum = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            int idx = threadIdx.x * PER + k;
            int v = 0;
            if (idx < ntile) {
                int g = tile_hi - idx;
                v = g == G ? (int)Np : Q.lists.nruns[g % A.Gcap];
            }
            loc[k] = v;
            lsum += v;
        }
        int incl = lsum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wsum[threadIdx.x >> 6] = incl;
        __syncthreads();
        int base = 0;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) base += s_wsum[w];
        int run = base + incl - lsum;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            int idx = threadIdx.x * PER + k;
            if (idx <= ntile) s_off[idx] = run;
            run += loc[k];
        }
        if (threadIdx.x == PF_BS - 1) s_off[ntile] = run;      // total (idx == ntile is only reached when ntile == TILE)
        __syncthreads();
        const long long T = s_off[ntile];
        // PF_CNT_BATCH tasks per thread and trip: a task is three dependent rounds of loads (run list -> posterior scan and
        // record range -> records) and little arithmetic, and the count workgroups hide latency badly (three per CU), so
        // the first two rounds of four tasks are in flight together.  The contributions are still added in task order
        // (t, t + nthreads, ...): the sums do not change.
        // A column is launched with as many workgroups as its busiest epochs need; the window of a younger epoch sits far behind
        // the front, where few ancestors are left: most of its workgroups have no task at all and leave here, before the bins,
        // the barriers and the reduction (adding zero to their accumulators is leaving them alone).
        if (tile_hi == g_hi && tile_lo == g_lo && (long long)bx * PF_BS >= T) return;
        if (A.flags & (1 << 20)) return;          // probe: what the workgroups cost before their first task
        if (L.gopp && !bins_ready) {
            for (int k = threadIdx.x; k < L.nlds + (A.n + 2) * L.ncnt; k += PF_BS) s_lbins[k] = 0.0;
            __syncthreads();
            bins_ready = true;
        }
        // A trip of the workgroup: one task per thread -- its weight and its records found in two rounds of loads -- then the RECORDS of
        // the 256 tasks dealt out over the threads, one record per thread and pass.  A task's records used to be walked by the thread
        // that owned the task, a load and a wait each, and a wavefront lasted as long as its lane with the most records: on the rows
        // where many epochs catch up the count role ended ten microseconds after the extend role (profiles/round4/wg_trace.md).  The
        // sums are grouped differently than before round 4 (by the thread that evaluates a record, not by the task's owner), in the
        // same way in every run.
        FlatTask* const s_ft = count_flat_tasks();
        int* const s_fpre = count_flat_prefix();
        for (long long base = (long long)bx * PF_BS; base < T; base += nthreads) {          // (the same trips for every thread: barriers inside)
            const long long t = base + threadIdx.x;
            const bool tval = t < T;
            // generation of task t: last idx with s_off[idx] <= t
            int lo_i = 0, hi_i = ntile;
            while (tval && hi_i - lo_i > 1) {
                int mid = (lo_i + hi_i) >> 1;
                if ((long long)s_off[mid] <= t) lo_i = mid; else hi_i = mid;
            }
            const int tg = tile_hi - lo_i;
            const long long ti = t - s_off[lo_i];
            const int tnr = s_off[lo_i + 1] - s_off[lo_i];
            const bool tlive = tval && tg == G;
            // round 1: the run (slots [q0, q1) of the row descend from slot a of generation g)
            int q0 = 0, q1 = 0;
            long long aa = -1;
            if (tval && !tlive) {
                const int* rst = Q.lists.st + (size_t)(tg % A.Gcap) * Np;
                const int* ran = Q.lists.anc + (size_t)(tg % A.Gcap) * Np;
                q0 = rst[ti];
                q1 = ti + 1 < tnr ? rst[ti + 1] : (int)Np;
                aa = ran[ti];
            }
            // round 2: posterior mass of the run's slots (difference of the inclusive posterior scan) and the ancestor's records of that
            // generation; for a live particle its own weight, its open stretch and the records it wrote this generation.  A ledger ring
            // that has overflowed (reported by the bookkeeping, ERR_GEN_OVERFLOW) aliases generations: whatever is read then must stay
            // inside the arrays until the host sees the error.
            double w = 0.0;
            long long a_t = 0;
            unsigned k0 = 0, nrec = 0;
            if (tlive) {
                const long long a = ti;
                w = Q.w[a] * inv;
                double S[NI];
#pragma unroll
                for (int r = 0; r < NI; ++r) S[r] = r < n - 1 ? Q.S[(size_t)r * Np + a] : 0.0;
                const double xm = Q.xm[a];
                const int ml = Q.ml[a];
                const unsigned g0 = A.gstart[(size_t)(tg % A.Gcap) * Np + a];
                const unsigned g1 = Q.widx[a];
                if (!(A.flags & (1 << 21)) && w != 0.0) {
                    stretch_contrib<NI, P>(acc, A, W, L, w, xm, PF_INF, S, ml);
                    if (g1 - g0 > A.cap) { if (!A.ctrl->err) A.ctrl->err = ERR_LOG_OVERFLOW; }
                    else { a_t = a; k0 = g0; nrec = g1 - g0; }
                }
            } else if (tval && !(q1 <= q0 || q1 > (int)Np || q0 < 0 || aa < 0 || aa >= Np)) {
                const double mhi = Q.offp[(q1 - 1) >> 6] + Q.scanp[q1 - 1];
                const double mlo = q0 > 0 ? Q.offp[(q0 - 1) >> 6] + Q.scanp[q0 - 1] : 0.0;
                const unsigned rk0 = A.gstart[(size_t)(tg % A.Gcap) * Np + aa];
                const unsigned rk1 = A.gstart[(size_t)((tg + 1) % A.Gcap) * Np + aa];
                const unsigned rwl = Q.widx_live[aa];
                w = (mhi - mlo) * inv;
                if (!(A.flags & (1 << 21)) && w > 0.0) {
                    if (rwl - rk0 > A.cap || rk1 - rk0 > A.cap) { if (!A.ctrl->err) A.ctrl->err = ERR_LOG_OVERFLOW; }
                    else { a_t = aa; k0 = rk0; nrec = rk1 - rk0; }
                }
            }
            // the records of the trip's tasks, numbered through: exclusive prefix sum of the record counts over the workgroup
            int incl_r = (int)nrec;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl_r, d, 64);
                if (lane >= d) incl_r += o;
            }
            if (lane == 63) s_wsum[threadIdx.x >> 6] = incl_r;
            __syncthreads();
            int base_r = 0;
            for (int wv = 0; wv < (int)(threadIdx.x >> 6); ++wv) base_r += s_wsum[wv];
            s_fpre[threadIdx.x] = base_r + incl_r - (int)nrec;
            if (threadIdx.x == PF_BS - 1) s_fpre[PF_BS] = base_r + incl_r;
            s_ft[threadIdx.x].w = w; s_ft[threadIdx.x].a = (int)a_t; s_ft[threadIdx.x].k0 = k0;
            __syncthreads();
            const int nrec_all = s_fpre[PF_BS];
            for (int r = (int)threadIdx.x; r < nrec_all; r += PF_BS) {
                int lo_j = 0, hi_j = PF_BS;                  // the task of record r: last j with s_fpre[j] <= r (its own count is not zero)
                while (hi_j - lo_j > 1) { const int mid = (lo_j + hi_j) >> 1; if (s_fpre[mid] <= r) lo_j = mid; else hi_j = mid; }
                const double w_r = s_ft[lo_j].w;
                const long long a_r = s_ft[lo_j].a;
                const double* rec = rec_ptr(A, a_r, s_ft[lo_j].k0 + (unsigned)(r - s_fpre[lo_j]));
                double f0 = rec[0], f1 = rec[1], f2 = rec[2], f3 = rec[3], f4 = rec[4];
                double S[NI];
#pragma unroll
                for (int q = 0; q < NI; ++q) S[q] = q < n - 1 ? rec[5 + q] : 0.0;
                unsigned long long dw = 0;
                if constexpr (NI >= PF_NMAX) if (L.gopp) dw = (unsigned long long)__double_as_longlong(rec[4 + n]);
                record_contrib_one<NI, P>(acc, A, W, L, w_r, a_r, f0, f1, f2, f3, f4, S, dw);
            }
            __syncthreads();                                 // (the next trip, or the next tile's staging, writes the arrays again)
        }
    }
    // deterministic workgroup reduction: butterfly per wavefront, then wavefronts in order
    if (L.gopp && bins_ready) {
        __syncthreads();
        for (int k = threadIdx.x; k < L.nlds; k += PF_BS) {
            double v = s_lbins[k];
            long long idx = L.b0 + k;
            if (v != 0.0 && idx < L.nbins) atomicAdd(&L.gopp[idx], v);
        }
        for (int k = threadIdx.x; k < (A.n + 2) * L.ncnt; k += PF_BS) {
            const double v = s_lbins[L.nlds + k];
            const long long idx = L.b0 + k % L.ncnt;
            if (v != 0.0 && idx < L.nbins) atomicAdd(&L.gcnt[(size_t)(k / L.ncnt) * L.nbins + idx], v);
        }
    }
#pragma unroll
    for (int k = 0; k < AC::NR; ++k) acc.v[k] = wave_tree_sum(acc.v[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x < AC::NC) {
        const int k = threadIdx.x;
        double t;
        if constexpr (AC::MIG_LDS) {
            // column k: a migration count from the workgroup's LDS table, or the register statistic that lands there (AccT::column)
            if (k >= AC::MC && k < AC::MC + P * P) t = count_mig()[k - AC::MC];
            else {
                const int kr = k < AC::MC ? k : k - P * P;
                t = red[0].v[kr];
                for (int w = 1; w < PF_BS / 64; ++w) t += red[w].v[kr];
            }
        } else {
        t = red[0].v[k];
        for (int w = 1; w < PF_BS / 64; ++w) t += red[w].v[k];
        }
        // this workgroup's own accumulator (folded by k_count_fin)
        if constexpr (ACC_AT_ENTRY) A.partial[((size_t)e * A.nbx + bx) * AC::NC + k] = acc_before + t;
        else A.partial[((size_t)e * A.nbx + bx) * AC::NC + k] += t;
    }
}

// (Round 4 also built the counting by generation -- units of 256 tasks of one generation, their weights and record ranges fetched once
// for all the epochs whose windows meet that generation, records flattened over the workgroup: count_units_body, commit 9818bcc and
// before.  It was slower in every regime (profiles/round4/count_rebuild.md); the part of it that paid, the flattened record walk, is in
// count_body now, and the rest was taken out.)

template <int NM, int P>
__global__ __launch_bounds__(PF_BS) void k_count(KArgs A, int e0, Windows Wn) {
    const int e = e0 + (int)blockIdx.y;
    if (e < Wn.first || e >= A.E) return;
    count_body<NM, P>(A, count_src_parity(A, A.sp, e), e, Wn.a[e], Wn.b[e], (int)blockIdx.x, (int)gridDim.x);
}

// k_count for a model with sample times (KArgs::anc; structured models on the general path only)
template <int NM, int P>
__global__ __launch_bounds__(PF_BS) void k_count_anc(KArgs A, int e0, Windows Wn) {
    const int e = e0 + (int)blockIdx.y;
    if (e < Wn.first || e >= A.E) return;
    count_body<NM, P, false, false, true>(A, count_src_parity(A, A.sp, e), e, Wn.a[e], Wn.b[e], (int)blockIdx.x, (int)gridDim.x);
}

// k_count with the column widths of the row pipeline (KArgs::cw_off: pf_params.count_wgs was set): grid = (widest column, epochs).
// For the handles whose chunks pf_run_many takes through k_sweep_blc<16, 1, *> while pf_run, pf_finish and the step API count here:
// a column's sums are grouped by its workgroups (count_body), so both have to give it the same number (pipe_count_item)
template <int NM, int P>
__global__ __launch_bounds__(PF_BS) void k_count_cw(KArgs A, int e0, Windows Wn) {
    const int e = e0 + (int)blockIdx.y;
    if (e < Wn.first || e >= A.E) return;
    const int j = A.E - 1 - e;
    const int cnb = A.cw_off[j + 1] - A.cw_off[j];
    if ((int)blockIdx.x >= cnb) return;
    count_body<NM, P>(A, count_src_parity(A, A.sp, e), e, Wn.a[e], Wn.b[e], (int)blockIdx.x, cnb);
}

// ------------------------------------------------------------------ k_row
// One launch per row on a single stream: workgroups [0, nb) extend the particles over row s (and complete row s-1 on
// load), the remaining workgroups evaluate the lagged counts of row s-1 (k_count's body).  The two halves touch
// disjoint data -- everything the counts read from row s-1 is immutable or double-buffered by row parity -- so the
// counting costs no synchronisation at all: no second stream, no event record / wait packets on the critical path.
template <int NM, bool BIASED, bool EXACT, bool TREES = false>
__global__ __launch_bounds__(PF_BS) void k_row(KArgs A, long long s, int fuse, int nb, int count_first, Windows Wprev) {
    if ((int)blockIdx.x < nb) {
        extend_reg_body<NM, BIASED, EXACT, TREES>(A, s, fuse);
    } else {
        const int idx = (int)blockIdx.x - nb;
        const int e = count_first + idx / nb;
        if (e < Wprev.first || e >= A.E) return;
        count_body<NM, 1, EXACT>(A, count_src_parity(A, A.sp ^ 1, e), e, Wprev.a[e], Wprev.b[e], idx % nb, nb);
    }
}

__global__ void k_count_fin(KArgs A) {
    __shared__ double stage[PF_FIN_PAIRS * PF_FIN_TILE_B];
    Ctrl* c = A.ctrl;
    if (c->pending_fin) finalize_counts(A, c, threadIdx.x, blockDim.x, stage);
}

// ------------------------------------------------------------------ k_resample (+ ledger blocks)
// Blocks [0, nblocks): no resampling -> normalise in place (pc.cpp:435-437); resampling ->
// implement_resampling (pc.cpp:321-392) as a gather from the old buffer into the new one.
// Blocks [nblocks, gridDim.x): after a resampling, re-base the run-length encoded composite
// ancestor maps of all retained generations onto the new slots (st' = lo[st], empty runs dropped).
#define PF_LEDGER_PER 8       // rounds per tile: a tile holds PF_LEDGER_PER * blockDim.x runs
#define PF_LEDGER_MAXT 1024   // largest workgroup the ledger code is launched with
#define PF_LEDGER_NEW 64      // the newest generations (long run lists) are re-based by a whole workgroup each

template <class KA>
__device__ __forceinline__ void ledger_update(const KA& A, int lb, int nlb, int G, int g_ret, RunLists src, RunLists dst) {
    __shared__ int scnt[PF_LEDGER_PER * (PF_LEDGER_MAXT / 64)], sexc[PF_LEDGER_PER * (PF_LEDGER_MAXT / 64)];
    __shared__ int stot;
    const long long Np = A.Np;
    const int* lo = A.lo + (size_t)(G % A.Gcap) * (Np + 1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = (int)blockDim.x, NW = NT >> 6;
    const int NCNT = PF_LEDGER_PER * NW;                 // <= 128: scanned by one wavefront, two counts per lane
    // ---- pass 1: workgroup per generation, newest PF_LEDGER_NEW generations (G itself: written by k_decide) ----
    // Compaction of a tile of PF_LEDGER_PER * blockDim.x runs with coalesced traffic only: element i of the tile
    // belongs to (round j, wavefront, lane) = (i / NT, (i % NT) / 64, i % 64).  All starts and ancestors of the tile
    // are requested at once, then all offspring offsets: two memory round trips per tile, and with the 1024
    // threads of k_decide_ledger the newest list (the survivors of the last resampling) is a single tile.  The
    // survivors of each (round, wavefront) are counted with a ballot, the counts are scanned by the first
    // wavefront, and every lane writes its survivors to their final places.  In place is safe: every input of the
    // tile is in registers before the first barrier, and the output never passes the tile's first input.
    for (int k = 1 + lb; k < PF_LEDGER_NEW; k += nlb) {
        const int g = G - k;
        if (g < g_ret) break;
        const int* rst = src.st + (size_t)(g % A.Gcap) * Np;
        const int* ran = src.anc + (size_t)(g % A.Gcap) * Np;
        int* wst = dst.st + (size_t)(g % A.Gcap) * Np;
        int* wan = dst.anc + (size_t)(g % A.Gcap) * Np;
        const int nr = src.nruns[g % A.Gcap];
        int out_base = 0;
        for (int tile0 = 0; tile0 < nr; tile0 += PF_LEDGER_PER * NT) {
            int ns[PF_LEDGER_PER], an[PF_LEDGER_PER], nx[PF_LEDGER_PER];
#pragma unroll
            for (int j = 0; j < PF_LEDGER_PER; ++j) {
                const int i = tile0 + j * NT + tid;
                ns[j] = i < nr ? rst[i] : 0;
                an[j] = i < nr ? ran[i] : 0;
                nx[j] = (lane == 63 && i < nr) ? (i + 1 < nr ? rst[i + 1] : (int)Np) : 0;     // successor of the last lane
            }
#pragma unroll
            for (int j = 0; j < PF_LEDGER_PER; ++j) {
                const int i = tile0 + j * NT + tid;
                ns[j] = i < nr ? lo[ns[j]] : 0;
                nx[j] = (lane == 63 && i < nr) ? lo[nx[j]] : 0;
            }
            unsigned keep = 0;
#pragma unroll
            for (int j = 0; j < PF_LEDGER_PER; ++j) {
                const int i = tile0 + j * NT + tid;
                int ne = __shfl_down(ns[j], 1, 64);
                if (lane == 63) ne = nx[j];
                else if (i + 1 >= nr) ne = (int)Np;                           // successor of the list's last run: lo[Np] = Np
                const bool kp = i < nr && ne > ns[j];
                const unsigned long long bal = __ballot(kp);
                if (kp) keep |= 1u << j;
                if (lane == 0) scnt[j * NW + wave] = __popcll(bal);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the ancestors too have arrived before anyone stores
            __syncthreads();
            if (tid < 64) {
                const int c0 = 2 * lane < NCNT ? scnt[2 * lane] : 0;
                const int c1 = 2 * lane + 1 < NCNT ? scnt[2 * lane + 1] : 0;
                int incl = c0 + c1;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    int o = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += o;
                }
                const int excl = incl - (c0 + c1);
                if (2 * lane < NCNT) sexc[2 * lane] = excl;
                if (2 * lane + 1 < NCNT) sexc[2 * lane + 1] = excl + c0;
                if (lane == 63) stot = incl;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < PF_LEDGER_PER; ++j) {
                const bool kp = (keep >> j) & 1u;
                const unsigned long long bal = __ballot(kp);
                if (kp) {
                    const int pos = out_base + sexc[j * NW + wave] + __popcll(bal & ((1ULL << lane) - 1ULL));
                    wst[pos] = ns[j];
                    wan[pos] = an[j];
                }
            }
            out_base += stot;
            __syncthreads();                 // the count arrays are reused by the next tile
        }
        if (tid == 0) dst.nruns[g % A.Gcap] = out_base;
    }
    // ---- pass 2: wavefront per generation for everything older (short lists, no workgroup barriers) ----
    const int wl = lb * NW + wave;
    const int nwl = nlb * NW;
    for (int g = G - PF_LEDGER_NEW - wl; g >= g_ret; g -= nwl) {
        const int* rst = src.st + (size_t)(g % A.Gcap) * Np;
        const int* ran = src.anc + (size_t)(g % A.Gcap) * Np;
        int* wst = dst.st + (size_t)(g % A.Gcap) * Np;
        int* wan = dst.anc + (size_t)(g % A.Gcap) * Np;
        const int nr = src.nruns[g % A.Gcap];
        int base = 0;
        for (int off = 0; off < nr; off += 64) {
            int i = off + lane;
            bool valid = i < nr;
            int stv = 0, nxt = 0, anc = 0;
            if (valid) {
                stv = rst[i];
                nxt = (i + 1 < nr) ? rst[i + 1] : (int)Np;
                anc = ran[i];
            }
            int ns = valid ? lo[stv] : 0;
            int ne = valid ? lo[nxt] : 0;
            bool keep = valid && ne > ns;
            unsigned long long bal = __ballot(keep);
            int pos = __popcll(bal & ((1ULL << lane) - 1ULL));
            // all 64 lanes loaded their inputs before anyone stores (stores depend on the ballot)
            if (keep) { wst[base + pos] = ns; wan[base + pos] = anc; }
            base += __popcll(bal);
        }
        if (lane == 0) dst.nruns[g % A.Gcap] = base;
    }
}

// ------------------------------------------------------------------ k_ledger (counting stream)
// After a resampling: workgroups [0, nblocks) write the run list of the generation that ended (its survivors,
// in slot order: start = lo[a], ancestor = a); the others re-base the run-length encoded composite ancestor
// maps of all retained generations onto the new slots (st' = lo[st], empty runs dropped).  Only k_count reads
// these lists, so the whole maintenance lives on the counting stream, off the filter's critical path.
// body of k_ledger for workgroup bx of nbt; `sp` = parity of the step whose resampling it follows up
// run list of the generation Gx that ends with a resampling: its survivors, in slot order (start = lo[a], ancestor = a).
// Position = survivors in earlier workgroups (blkcnt, counted where the offspring table was made) + rank inside this one.
template <class KA>
__device__ __forceinline__ void ledger_new_list(const KA& A, RunLists dst, const int* blkcnt, int nblocks, int bx, int Gx, int gran = 1) {
    const long long Np = A.Np;
    const long long i = (long long)bx * PF_BS + threadIdx.x;
    __shared__ int wsum[PF_BS / 64];
    const int* lox = A.lo + (size_t)(Gx % A.Gcap) * (Np + 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int l0 = 0, l1 = 0;
    if (i < Np) { l0 = lox[i]; l1 = lox[i + 1]; }
    const bool surv = l1 > l0;
    unsigned long long bal = __ballot(surv);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __shared__ int sblk[1024];
    // survivors per block of 256 particles; the structured extend workgroups own 64 particles each and leave four entries per block
    for (int b = threadIdx.x; b < nblocks; b += PF_BS) {
        int v = 0;
        for (int j = 0; j < gran; ++j) v += blkcnt[b * gran + j];
        sblk[b] = v;
    }
    __syncthreads();
    int base = 0;
    for (int b = 0; b < bx; ++b) base += sblk[b];
    for (int w = 0; w < wave; ++w) base += wsum[w];
    if (surv) {
        int pos = base + __popcll(bal & ((1ULL << lane) - 1ULL));
        dst.st[(size_t)(Gx % A.Gcap) * Np + pos] = l0;
        dst.anc[(size_t)(Gx % A.Gcap) * Np + pos] = (int)i;
    }
    if (bx == nblocks - 1 && threadIdx.x == PF_BS - 1) {
        int tot = base + __popcll(bal);           // base already holds the earlier wavefronts of this workgroup
        dst.nruns[Gx % A.Gcap] = tot;
    }
}

template <class KA>
__device__ __forceinline__ void ledger_body(const KA& A, int sp, int nblocks, int bx, int nbt) {
    const Ctrl* c = A.ctrl;
    if (!c->step[sp].flag) return;
    const int Gx = c->step[sp].G;
    const RunLists lists = run_lists(A, c->lver);       // the general kernels re-base in place
    if (bx >= nblocks) {
        ledger_update(A, bx - nblocks, nbt - nblocks, Gx, c->g_retain, lists, lists);
        return;
    }
    ledger_new_list(A, lists, A.blkcnt2[sp], nblocks, bx, Gx);
}

// ------------------------------------------------------------------ k_pipe: one launch per row
// The single-launch pipeline of the register-tree kernels (one population, n <= 8, no look-ahead).  Launch s carries
//   X(s)    workgroups [0, nb): extend the particles over row s.  On load they complete row s-1 themselves: decision
//           (decide_row), offspring offsets, parent search, gather or normalisation -- nothing from k_decide is read;
//   B(s-1)  one workgroup: the bookkeeping of row s-1 (log-likelihood, traces, generations of the count windows,
//           posterior-scan offsets), published in Ctrl::ri[(s-1) & (PF_RING-1)];
//   L(s-2)  ledger upkeep after the resampling of row s-2: reads the run lists in force, writes the other copy;
//   C(s-2)  the lagged counts of row s-2 from the lists in force for that row and its slot of the state ring.
// What a role reads was written by an earlier launch (stream order) or is private to it; nothing waits inside the
// launch.  The decide kernel and its two dependent kernel boundaries per row are gone from the critical path.
__global__ void k_pipe_seed(KArgs A, int slot) {
    Ctrl* c = A.ctrl;
    Ctrl::RowInfo& r = c->ri[slot];
    r.n_res = c->n_resample; r.gen = c->gen; r.flag = 0; r.lver = c->lver; r.g_retain = c->g_retain; r.first = A.E;
    r.inv_T = 1.0; r.T = 1.0; r.S1 = 0.0; r.u = 0.0; r.pos = c->cur_pos;
    c->xr[slot].n_res = c->n_resample; c->xr[slot].gen = c->gen; c->xr[slot].flag = 0;
}

template <bool BIASED, class KA>
__device__ __forceinline__ void pipe_bookkeeping(const KA& A, const PipeLds& q, const PipeLaunch& PL, const Windows& W) {
    Ctrl* c = A.ctrl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = PF_BS / 64;
    const int E = A.E, nc = A.nc, ng = (nc + 63) / 64;
    const int slot = PL.b_slot;
    const long long n_res = c->n_resample;        // as the bookkeeping of the previous row left them (previous launch)
    const int G = c->gen;
    RowDecision d = decide_row<false>(A, q, slot, n_res);
    __syncthreads();
    // exclusive offsets of the posterior scan of the row's wavefronts: the counts turn differences of that scan into
    // the posterior mass of a particle's descendants
    const double* cpp = A.rg_cpp + (size_t)slot * nc;
    for (int g = wave; g < ng; g += nwaves) {
        int ch = g * 64 + lane;
        double vq = ch < nc ? cpp[ch] : 0.0;
        double scq = wave_hs_scan(vq, lane);
        if (ch < nc) q.pmx[ch] = scq;
        if (lane == 63) q.l2_post[g] = scq;
    }
    __syncthreads();
    for (int ch = tid; ch < nc; ch += PF_BS) {
        double runp = 0.0;
        for (int g = 0; g < ch / 64; ++g) runp = runp + q.l2_post[g];
        double offp = (ch % 64 == 0) ? 0.0 : q.pmx[ch - 1];
        A.rg_coffp[(size_t)slot * nc + ch] = runp + offp;
    }
    Ctrl::RowInfo& r = c->ri[slot];
    // generations that hold the ends of the row's count windows (both monotone along the sweep)
    // (the windows are a kernel argument: indexed with a uniform epoch so that they are read with scalar loads)
    // k_sweep / k_sweep_blc keep the windows in LDS: thread e takes epoch e (each of the two searches is a chain of dependent
    // loads; one epoch after the other, as the by-value form below has to, they were 20 us of a launch)
    constexpr bool W_IN_LDS = !std::is_same<KA, KArgs>::value;
    for (int e = W_IN_LDS ? (tid < E ? tid : E) : 0; e < E; e = W_IN_LDS ? E : e + 1) {
        const double wa = W.a[e], wb = W.b[e];
        if (tid != e) continue;
        int g = c->g_lo[e];
        while (g < G && A.gen_x0[(g + 1) % A.Gcap] <= wa) ++g;
        c->g_lo[e] = g;
        int h = c->g_hi[e];
        if (e >= W.first) {
            if (h < g) h = g;
            while (h < G && A.gen_x0[(h + 1) % A.Gcap] < wb) ++h;
            c->g_hi[e] = h;
        }
        r.g_lo[e] = g; r.g_hi[e] = h; r.wa[e] = wa; r.wb[e] = wb;
    }
    __syncthreads();
    if (tid == 0) {
        int gr = c->g_lo[0];
        for (int e = 1; e < E; ++e) gr = c->g_lo[e] < gr ? c->g_lo[e] : gr;
        c->g_retain = gr;
        // (the entry of two rows ago, or what the seed of the call left there; where the bookkeeping itself runs ahead of the counts with the
        // extend role -- run_sweep_split -- the oldest entry of the ring: the counts in flight are at most fifteen rows behind this one)
        c->g_safe = c->ri[(slot + PF_RING - (PL.nL == -3 ? PF_RING - 1 : 2)) & (PF_RING - 1)].g_retain;
        c->delayed_opp += W.b[E - 1] - W.a[E - 1];
        if (BIASED) {
            long long npend = 0;      // update_delayed_weight_count (count.cpp:395-397)
            for (int k = 0; k < nc; ++k) npend += A.rg_dpend[(size_t)slot * nc + k];
            c->delayed_count += (double)npend * (W.b[E - 1] - W.a[E - 1]);
        }
        c->first_epoch = W.first;
        c->count_active = W.first < E;
        if (W.first < E) c->pending_fin = 1;
        c->nbx_used = A.nbx;
        c->wq[PL.b_slot] = 0;                 // the next step deals out the ledger and count work of this row (pipe_roles)
        if (!(d.T > 0.0) && !c->err) c->err = ERR_ZERO_PROB;
        double logl = c->logl + dlog(d.T);
        c->logl = logl;
        const long long row = PL.b_row;
        A.tr_T[row] = d.T; A.tr_ess[row] = d.ess; A.tr_flag[row] = d.flag; A.tr_logl[row] = logl;
        c->cur_pos = PL.b_pos;
        c->T = d.T; c->inv_T = d.inv; c->S1 = d.S1; c->S2 = d.S2; c->ess = d.ess; c->u = d.u; c->flag = 0;
        r.T = d.T; r.inv_T = d.inv; r.S1 = d.S1; r.u = d.u; r.pos = PL.b_pos;
        r.n_res = n_res; r.gen = G; r.flag = d.flag; r.g_retain = gr; r.first = W.first; r.lver = c->lver;
        if (d.flag) {
            int ev = (int)n_res;
            if (ev < A.max_trace_events) A.ev_seg[ev] = (int)row;
            c->gen = G + 1;
            A.gen_x0[(G + 1) % A.Gcap] = PL.b_pos;
            c->n_resample = n_res + 1;
            c->lver ^= 1;                    // the ledger upkeep of this row (next launch) writes the other copy
            // an extend role that is a launch of its own is already writing offspring tables and log marks of up to PF_RING newer generations
            if (G + 1 - gr >= A.Gcap - 1 - (PL.ahead ? PF_RING : 0)) c->err = ERR_GEN_OVERFLOW;
            if (A.rec_trees && G + 2 >= A.Gcap) c->err = ERR_GEN_OVERFLOW;      // -arg keeps every generation
        }
        c->gen_prev = c->gen; c->nres_prev = c->n_resample;
        if (PL.b_set_cur >= 0) c->cur = PL.b_set_cur;
    }
}

// The draw table (one-population rows of k_sweep).  The random numbers of a slot are a function of (seed, slot, draw index)
// alone -- the stream belongs to the slot, not to the particle that sits in it -- so the numbers the slot's next genealogy
// updates will ask for can be made before they are asked for, by workgroups that are off the critical path: a third of
// an update's instructions are its two Philox blocks and the logarithms of two of the four uniforms.  Step s brings the
// table of every slot up to PF_DRAW_RING blocks past the counter the slot had at the start of row s (written by the extend
// role of step s - 1); the extend role of step s + 1 reads it.  What the extend role of step s reads at the same time lies
// below the old mark, what is written here at or above it, and the ring holds PF_DRAW_RING blocks: no entry is read and
// written in one launch.  A slot that outruns its table (more than sixteen updates in a row) computes its own numbers, and
// the table skips ahead.
template <class KA>
__device__ __forceinline__ void draw_role(const KA& A, int tb, int nT, int par) {
    const long long Np = A.Np;
    const unsigned long long* c_in = A.dt_ctr + (size_t)(par ^ 1) * Np;
    const unsigned long long* f_in = A.dt_filled + (size_t)(par ^ 1) * Np;
    unsigned long long* f_out = A.dt_filled + (size_t)par * Np;
    const unsigned long long seed = A.seed;
    for (long long p = (long long)tb * PF_BS + threadIdx.x; p < Np; p += (long long)nT * PF_BS) {
        const unsigned long long c0 = c_in[p], f_old = f_in[p];
        const unsigned long long to = c0 + PF_DRAW_RING;
        double2* tab = (double2*)A.dt_tab + (size_t)p * PF_DRAW_RING;
        for (unsigned long long cc = f_old > c0 ? f_old : c0; cc < to; ++cc) {
            double u0, u1;
            philox_pair(seed, (unsigned)p, 0u, cc, u0, u1);
            tab[(unsigned)cc & (PF_DRAW_RING - 1)] = make_double2(u0, -dlog(u1));
        }
        f_out[p] = to;
    }
}

// one block of the ledger upkeep of the row in ring slot PL.lc_slot (a resampling row): the new run list, or a share of the old ones
template <class KA>
__device__ __forceinline__ void pipe_ledger_item(const KA& A, const PipeLaunch& PL, const Ctrl::RowInfo& r, int lb) {
    const RunLists src = run_lists(A, r.lver), dst = run_lists(A, r.lver ^ 1);
    const int nblk = PL.nblk;              // particle blocks of 256 (the extend workgroups of the one-population kernels)
    if (lb < nblk) ledger_new_list(A, dst, A.rg_blkcnt + (size_t)PL.lc_slot * nblk * A.blk_gran, nblk, lb, r.gen, A.blk_gran);
    else ledger_update(A, lb - nblk, PL.nL - nblk, r.gen, r.g_retain, src, dst);
}

// count work item idx of that row: part cbx of cnb of the column of epoch e
template <int NM, bool EXACT, int P, bool ACC_AT_ENTRY = false, class KA>
__device__ __forceinline__ void pipe_count_item(const KA& A, const PipeLaunch& PL, const Ctrl::RowInfo& r, int idx) {
    // the columns of the oldest epochs first: their lags are the shortest, their windows sit right behind the front where
    // nearly every particle is still its own ancestor, and their workgroups are the long ones -- dispatched last they were
    // what a launch ended with
    // (bit 512 of KArgs::flags is set by nobody any more -- it chose the ascending order until that lost its A/B.  Its two tests stay for
    // k_pipe's sake, the comparator of the sweep tests: without them the register allocation of five k_pipe instances comes out with 36 to
    // 68 bytes of scratch memory where it had none -- profiles/round6/r6_kernel_meta.md)
    int e, cbx, cnb;
    if (A.cw_off && !(A.flags & 512)) {
        int j = 0, hi = A.E;                       // the column of workgroup idx: last j with cw_off[j] <= idx
        while (hi - j > 1) { const int mid = (j + hi) >> 1; if (A.cw_off[mid] <= idx) j = mid; else hi = mid; }
        e = A.E - 1 - j; cbx = idx - A.cw_off[j]; cnb = A.cw_off[j + 1] - A.cw_off[j];
    } else {
        e = (A.flags & 512) ? r.first + idx / PL.ncw : A.E - 1 - idx / PL.ncw;
        cbx = idx % PL.ncw; cnb = PL.ncw;
    }
    if (e >= A.E || e < r.first) return;
    if (A.flags & (1 << 22)) return;          // probe: the count workgroups do nothing at all
    const DState st = state_slot(A, PL.lc_slot);
    CountSrc Q;
    Q.w = st.w_post; Q.S = st.S; Q.xm = st.x_mark; Q.ml = st.mark_limit;
    Q.widx = A.rg_widx + (size_t)PL.lc_slot * A.Np;
    Q.widx_live = A.rg_widx + (size_t)PL.live_slot * A.Np;
    Q.scanp = A.rg_scanp + (size_t)PL.lc_slot * A.Np;
    Q.offp = A.rg_coffp + (size_t)PL.lc_slot * A.nc;
    Q.lists = run_lists(A, r.lver);
    Q.inv = r.inv_T; Q.G = r.gen; Q.g_lo = r.g_lo[e]; Q.g_hi = r.g_hi[e];
    count_body<NM, P, EXACT, ACC_AT_ENTRY>(A, Q, e, r.wa[e], r.wb[e], cbx, cnb);
}

// (NO_EXTEND: the caller has run the extend role itself -- sweep_kernel_body with the row header; ACC_AT_ENTRY: count_body)
template <int NM, bool BIASED, bool EXACT, bool TREES, int P = 1, bool BLC = false, bool QUEUE = false, bool LEAN = false, bool NO_EXTEND = false, bool LOOK = false,
          bool ACC_AT_ENTRY = false, class KA>
__device__ __forceinline__ void pipe_roles(const KA& A, long long s, const PipeLaunch& PL, const Windows& Wb) {
    const int bx = pf_bx();
    const int nb = PL.nb;
    // (LEAN: the launch of the ledger and count roles alone -- run_sweep_split -- is compiled without the other three: their registers and LDS
    // are what would keep it from four workgroups per compute unit)
    if constexpr (!LEAN) {
        if (bx < nb) {
            if constexpr (P == 1 && !BLC && !NO_EXTEND) { if (PL.row.extend || PL.row.complete) extend_reg_body<NM, BIASED, EXACT, TREES, true, false, LOOK>(A, s, 0, PL.row); }
            return;
        }
        if (bx == nb) {
            if (PL.b_slot < 0) return;
            extern __shared__ double smem[];
            PipeLds q = pipe_carve(smem + (2 * PF_EPAD + A.E + 2 * PF_BIAS_MAX + 3), A.nc);
            pipe_bookkeeping<BIASED>(A, q, PL, Wb);
            return;
        }
        if (bx - (nb + 1) < PL.nT) {
            if constexpr (P == 1 && !BLC) draw_role(A, bx - (nb + 1), PL.nT, PL.row.draws - 1);
            return;
        }
    } else {
        if (bx <= nb) return;
    }
    if (PL.lc_slot < 0 || PL.nL < -1) return;          // nL = -3: the extend launch of a split step (run_sweep_split)
    const Ctrl* c = A.ctrl;
    const Ctrl::RowInfo& r = c->ri[PL.lc_slot];
    const int lb = bx - (nb + 1) - PL.nT;
    // The ledger and count work of the step: items -- a ledger block of a resampling row, or part cbx of the count column of an
    // epoch.  Without pf_params.count_workers every item is a workgroup of this launch (ledger blocks first, then the columns,
    // oldest epoch first).
    if constexpr (!QUEUE) {
        if (lb < PL.nL) { if (r.flag) pipe_ledger_item(A, PL, r, lb); }
        else pipe_count_item<NM, EXACT, P, ACC_AT_ENTRY>(A, PL, r, lb - PL.nL);
    } else {
        // With it, `workers` workgroups take the items -- the columns first, then the ledger's blocks -- off a counter until none is
        // left: an item writes the same accumulators whoever runs it, the sums do not change.  What that saves several chunks per
        // GPU: the 232 ledger workgroups per chunk and step that find no resampling and leave (2 us of a slot each), the prologue
        // of 260 count workgroups, and the dispatcher's strict order -- workgroup i + 1 is not placed before workgroup i, so one
        // full XCD holds up the other seven while long count workgroups run (profiles/round4/wg_trace.md).  A kernel instance of
        // its own (k_sweep4q): in the static form the count body is the last thing a workgroup does and nothing is live across it;
        // what this loop needs after an item comes back from LDS.
        __shared__ int s_wk[8];
        if (lb >= PL.workers) return;
        if (threadIdx.x == 0) { s_wk[0] = PL.lc_slot; s_wk[1] = PL.live_slot; s_wk[2] = PL.nL; s_wk[3] = PL.nblk; s_wk[4] = PL.ncw; }
        const KA* Ap = &A;
        for (;;) {
            // (the argument block behind a pointer the compiler cannot see through: otherwise it loads every field the item bodies use once,
            // before the loop, keeps them all in registers across the items and spills vector registers to scratch memory to do so)
            asm volatile("" : "+s"(Ap));
            const KA& A2 = *Ap;
            __syncthreads();
            if (threadIdx.x == 0) s_wk[6] = (int)__hip_atomic_fetch_add(&A2.ctrl->wq[s_wk[0]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            PipeLaunch Q2;
            Q2.lc_slot = s_wk[0]; Q2.live_slot = s_wk[1]; Q2.nL = s_wk[2]; Q2.nblk = s_wk[3]; Q2.ncw = s_wk[4];
            const int it = s_wk[6];
            const Ctrl::RowInfo& r2 = A2.ctrl->ri[Q2.lc_slot];
            const int ncnt = r2.first < A2.E ? (A2.cw_off ? A2.cw_off[A2.E - r2.first] : (A2.E - r2.first) * Q2.ncw) : 0;
            if (it >= ncnt + (r2.flag ? Q2.nL : 0)) return;                  // (every workgroup gets here: the counter only grows)
            // (inlined: as real calls the item bodies save and restore 124 registers per item in scratch memory -- 5.7e4 segments/s
            // against 8.0e4 for eight chunks with 264 workers each, and 9.4e4 without the queue)
            if (it < ncnt) pipe_count_item<NM, EXACT, P>(A2, Q2, r2, it);
            else pipe_ledger_item(A2, Q2, r2, it - ncnt);
        }
    }
}

template <int NM, bool BIASED, bool EXACT, bool TREES>
__global__ __launch_bounds__(PF_BS) void k_pipe(KArgs A, long long s, PipeLaunch PL, Windows Wb) {
    pipe_roles<NM, BIASED, EXACT, TREES>(A, s, PL, Wb);
}

// ------------------------------------------------------------------ k_sweep: several chunks per launch
// The same four roles as k_pipe, for C independent chunks at once: blockIdx.x is the chunk (pf_bx(), pf_device.h), each with its own argument
// block in device memory (SweepChunk::A, read through the constant address space: every field is a scalar load where it
// is used, nothing of the block is a kernel argument any more), its own Ctrl, rings and event log.  All chunks step in
// lockstep: launch t handles row s = s_begin + t of every chunk that still has one (then its two flush steps).  What
// k_pipe is told per launch by the host is derived here: the plan of the step (sweep_plan = the `launch` lambda of
// run_pipeline) from (s, s_begin, s_last), and the count windows of row s - 1 by the bookkeeping workgroup from the
// chunk's own window state (sweep_windows = host_windows, operation for operation), so the host only supplies t.
// One chunk per GPU uses a sixth of the SIMDs; the reference's data parallelism is one process per chunk, all at once
// (smcsmc/model.py:1094-1098), which is what a grid over chunks is here.
// extract_and_update_count's window rule (count.cpp:363-385) for the row that ends at `pos`: host_windows() on the device,
// the same operations in the same order on the same doubles; the window state lives in Ctrl::counted_to.  Called by all
// threads of the bookkeeping workgroup; W is in LDS.
template <class KA>
__device__ __forceinline__ void sweep_windows(const KA& A, Ctrl* c, double pos, Windows& W) {
    const int e = threadIdx.x, E = A.E;
    if (e < 64) {
        const bool in = e < E;
        const double lagging = in ? A.lags[e] : 0.0;
        const double x_end = pos - lagging;
        const double ct = in ? c->counted_to[e] : 0.0;
        const bool small = (x_end - ct) < lagging * 0.1;
        const unsigned long long moved = __ballot(in && !small);
        const int first = moved ? (int)__builtin_ctzll(moved) : E;
        if (in) {
            const double b = (small && first > e) ? ct : x_end;
            W.a[e] = ct; W.b[e] = b;
            c->counted_to[e] = b;
        }
        if (e == 0) { W.first = first; W.end_data = 0; }
    }
    __syncthreads();
}

// where a workgroup of a traced step (pf_set_wg_trace) leaves its four words: start and end on the 100 MHz clock, HW_ID | XCC_ID << 32,
// index within the chunk | chunk << 32
__device__ __forceinline__ unsigned long long* wg_trace_slot(SweepChunkC& ch, long long t) {
    if (!ch.trace || t < ch.trace_t0 || t >= ch.trace_t0 + ch.trace_n) return nullptr;
    const size_t lin = blockIdx.x + (size_t)gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z);
    return ch.trace + ((size_t)(t - ch.trace_t0) * (size_t)ch.trace_stride + lin) * 4;
}

// HEAD: the extend workgroups take the plan of the step and the addresses of their head from the chunk's row header (SweepHead,
// pf_pipe.h): entry t & (PF_RING - 1), which lies in front of the chunk table at an address the kernel arguments give (sweep_head_of),
// loaded in one batch -- two dependent scalar round trips in front of the first request where sweep_plan and the argument block had
// ten.  The other roles plan as before.
// PAIR (with HEAD): the extend workgroups run the paired form of the role (extend_pair_body, pf_pair.h), 128 particles each.
template <int NM, bool BIASED, bool EXACT, bool TREES, bool TRACE = false, bool QUEUE = false, bool HEAD = false, bool LOOK = false, bool PAIR = false>
__device__ __forceinline__ void sweep_kernel_body(const SweepChunk* tab_g, long long t, int nb) {
    SweepChunkC* tab = (SweepChunkC*)tab_g;
    SweepChunkC& ch = tab[pf_chunk()];
    KArgsC& A = ch.A;
    __shared__ Windows W;           // written and read by the bookkeeping workgroup only
    if constexpr (TRACE) {
        if (threadIdx.x == 0) {
            if (unsigned long long* w = wg_trace_slot(ch, t)) {
                w[0] = wall_clock64();
                w[2] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);
                w[3] = (unsigned long long)(unsigned)pf_bx() | ((unsigned long long)(unsigned)pf_chunk() << 32);
            }
        }
    }
    if (HEAD && pf_bx() < nb) {
        if constexpr (HEAD) {
            // (nothing is outstanding here: said so that no request of the other roles' code is taken for pending in this one's)
            __builtin_amdgcn_s_waitcnt(0x0F70);
            const SweepHeadR H(sweep_head_of((SweepHeadC*)tab_g, pf_chunk(), t));
            // sweep_plan for the extend role, from the entry alone (the second flush step has nothing for this role)
            const long long s_begin = PF_HL(H, s_begin), s_last = PF_HL(H, s_last), sx = s_begin + t;
            if (s_last >= s_begin && sx <= s_last + 1) {
                PipeRow PR;
                PR.extend = sx <= s_last ? 1 : 0;
                PR.complete = sx > s_begin ? 1 : 0;
                PR.slot_prev = PR.complete ? (int)((sx - 1) & (PF_RING - 1)) : -1;
                PR.slot_out = (int)(sx & (PF_RING - 1));
                PR.pos_prev = 0.0;                                 // (the end of row s - 1 is requested with the head)
                PR.draws = PF_HI(H, nT) > 0 ? 1 + (int)(sx & 1) : 0;
                PR.ahead = (PF_HI(H, split) || PF_HI(H, P) > 1) ? 1 : 0;
                if constexpr (PAIR) extend_pair_body<EXACT>(A, sx, nb, PR, H);
                else extend_reg_body<NM, BIASED, EXACT, TREES, true, true>(A, sx, 0, PR, H);
            }
        }
    } else {
        const long long s = ch.s_begin + t;
        PipeLaunch PL;
        if (sweep_plan(ch, s, nb, PL)) {
            if (ch.split == 2) PL.nL = -3;                 // extend, bookkeeping and draw roles only: ledger and counts are k_sweep_blc's (run_sweep_split)
            if (pf_bx() == nb && PL.b_slot >= 0) sweep_windows(A, A.ctrl, PL.b_pos, W);
            pipe_roles<NM, BIASED, EXACT, TREES, 1, false, QUEUE, false, HEAD, LOOK>(A, s, PL, W);
        }
    }
    if constexpr (TRACE) {
        __syncthreads();
        if (threadIdx.x == 0) if (unsigned long long* w = wg_trace_slot(ch, t)) w[1] = wall_clock64();
    }
}
// (LOOK: with the look-ahead factor in the extend role -- pf_lookahead.flags bit 0; BIASED = TREES = false, NM 4 and 8)
template <int NM, bool BIASED, bool EXACT, bool TREES, bool LOOK = false>
__global__ __launch_bounds__(PF_BS) void k_sweep(const SweepChunk* tab_g, long long t, int nb) {
    sweep_kernel_body<NM, BIASED, EXACT, TREES, false, false, false, LOOK>(tab_g, t, nb);
}
// The headline instance (at most four haplotypes, no focused sampling) with the occupancy stated: three workgroups per compute
// unit, i.e. at most 168 registers a thread -- several chunks per GPU lose 15 % with two.  Left to itself
// the register allocator aims at the occupancy the kernel's LDS allows: that gave 168 while the count roles' LDS was 8 KB
// larger and 172-174 since round 4.  (The instances for more haplotypes or focused sampling need about 190 registers and would
// spill to scratch memory under the same attribute; they stay as they are.)
template <bool EXACT, bool TREES>
__global__ __launch_bounds__(PF_BS) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_sweep4(const SweepChunk* tab_g, long long t, int nb) {
    sweep_kernel_body<4, false, EXACT, TREES, false, false, true>(tab_g, t, nb);
}
// the headline instance with the extend role in its paired form (run_sweep_split, where every extend workgroup has a compute unit of its own: the
// occupancy is one workgroup, the registers are what the two roles need)
template <bool EXACT>
__global__ __launch_bounds__(PF_BS) void k_sweep4p(const SweepChunk* tab_g, long long t, int nb) {
    sweep_kernel_body<4, false, EXACT, false, false, false, true, false, true>(tab_g, t, nb);
}
// the headline instance with the ledger and count work of a step taken off a queue (pf_params.count_workers; the traced form too)
template <bool EXACT, bool TRACE>
__global__ __launch_bounds__(PF_BS) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_sweep4q(const SweepChunk* tab_g, long long t, int nb) {
    sweep_kernel_body<4, false, EXACT, false, TRACE, true, true>(tab_g, t, nb);
}
// the headline instance with a time stamp at either end of every workgroup (pf_set_wg_trace: where do the slots of a step go?)
template <bool EXACT>
__global__ __launch_bounds__(PF_BS) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_sweep4t(const SweepChunk* tab_g, long long t, int nb) {
    sweep_kernel_body<4, false, EXACT, false, true, false, true>(tab_g, t, nb);
}

// The bookkeeping, ledger and count roles of a step as a launch of their own: what the structured models run on the counting
// stream beside their extend launch (k_sweep_xmp, pf_mp.hip).  The extend workgroups of those models carry their trees'
// migration events in LDS (61 KB per 64 particles at the default capacity); in one launch every count workgroup would be
// given the same allocation and one would fit a CU.
// COUNTS_ONLY (k_sweep_blc4, with LEAN): the launch is only ever the second one of a split step (SweepChunk::split = 2, run_sweep_split), said at
// compile time -- the plan is made without the end of row s - 1, which only the bookkeeping wants (sweep_plan<false>), the word `split` is not
// read, and a count workgroup asks for its accumulator when it starts (count_body, ACC_AT_ENTRY): three dependent scalar round trips fewer in
// front of the first vector request of every workgroup of the launch, and one memory round trip fewer behind the last sum of a count workgroup.
template <int NM, int P, bool BIASED, bool EXACT = false, bool LEAN = false, bool QUEUE = false, bool COUNTS_ONLY = false>
__device__ __forceinline__ void sweep_blc_body(const SweepChunk* tab_g, long long t) {
    SweepChunkC* tab = (SweepChunkC*)tab_g;
    SweepChunkC& ch = tab[pf_chunk()];
    KArgsC& A = ch.A;
    const long long s = ch.s_begin + t;
    __shared__ Windows W;
    Ctrl* c = A.ctrl;
    PipeLaunch PL;
    if constexpr (COUNTS_ONLY) {
        static_assert(LEAN && !QUEUE, "the second launch of a split step in its static form");
        if (sweep_plan<false>(ch, s, 0, PL)) {
            PL.nT = 0; PL.b_slot = -1;
            pipe_roles<NM, BIASED, EXACT, false, P, true, false, true, false, false, true>(A, s, PL, W);
        }
    } else if (sweep_plan(ch, s, 0, PL)) {
        PL.nT = 0;                                         // the draw role rides with the extend launch
        if (ch.split == 2) PL.b_slot = -1;                 // ... and so does the bookkeeping (run_sweep_split)
        if (pf_bx() == 0 && PL.b_slot >= 0) sweep_windows(A, c, PL.b_pos, W);
        pipe_roles<NM, BIASED, EXACT, false, P, true, QUEUE, LEAN>(A, s, PL, W);
    }
}

template <int NM, int P, bool BIASED>
__global__ __launch_bounds__(PF_BS) void k_sweep_blc(const SweepChunk* tab_g, long long t) {
    sweep_blc_body<NM, P, BIASED>(tab_g, t);
}
// the ledger and count roles of several chunks beside their extend launches (run_sweep_split): at most four haplotypes, no focused
// sampling, and no dynamic LDS -- four workgroups to a compute unit (128 registers, 36.6 KB)
template <bool EXACT>
__global__ __launch_bounds__(PF_BS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_sweep_blc4(const SweepChunk* tab_g, long long t) {
    sweep_blc_body<4, 1, false, EXACT, true, false, true>(tab_g, t);
}
// ... with the ledger and count items of a step taken off a queue by a fixed number of workgroups (pf_params.count_workers)
template <bool EXACT>
__global__ __launch_bounds__(PF_BS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_sweep_blc4q(const SweepChunk* tab_g, long long t) {
    sweep_blc_body<4, 1, false, EXACT, true, true>(tab_g, t);
}

// The extend role of the row pipeline on the per-lane LDS tree (one population, 9 to 16 haplotypes; extend_lds_pipe_body,
// pf_lds_pipe.h): step t of the chunk table, blockIdx.y is the chunk, 256 particles per workgroup.  A chunk that is finished or
// sits the call out leaves before it touches LDS or memory other than its table entry.  The bookkeeping, ledger and count
// roles of the step are k_sweep_blc<16, 1, *> on the counting stream: in one launch every count workgroup would be given the
// extend workgroups' tree columns (100 KB at 16 haplotypes) and one would fit a compute unit.
// (LOOK: with the look-ahead factor in the extend role -- pf_lookahead.flags bit 2; BIASED = false)
template <bool BIASED, bool LOOK = false>
__global__ __launch_bounds__(PF_BS) void k_sweep_xl(const SweepChunk* tab_g, long long t) {
    SweepChunkC* tab = (SweepChunkC*)tab_g;
    SweepChunkC& ch = tab[pf_chunk()];
    KArgsC& A = ch.A;
    const long long s = ch.s_begin + t;
    PipeLaunch PL;
    if (!sweep_plan(ch, s, 0, PL)) return;
    if (!(PL.row.extend || PL.row.complete)) return;
    extern __shared__ double smem[];
    extend_lds_pipe_body<BIASED, LOOK>(A, s, PL.row, smem);
}

// first step of a call: the seed of k_pipe_seed, and the chunk's window state
__global__ void k_sweep_seed(const SweepChunk* tab_g) {
    SweepChunkC* tab = (SweepChunkC*)tab_g;
    SweepChunkC& ch = tab[blockIdx.x];
    KArgsC& A = ch.A;
    if (ch.s_last < ch.s_begin) return;              // nothing to do for this chunk in this call
    Ctrl* c = A.ctrl;
    const int slot = (int)((ch.s_begin + PF_RING - 1) & (PF_RING - 1));
    if (threadIdx.x == 0) {
        Ctrl::RowInfo& r = c->ri[slot];
        r.n_res = c->n_resample; r.gen = c->gen; r.flag = 0; r.lver = c->lver; r.g_retain = c->g_retain; r.first = A.E;
        r.inv_T = 1.0; r.T = 1.0; r.S1 = 0.0; r.u = 0.0; r.pos = c->cur_pos;
        c->xr[slot].n_res = c->n_resample; c->xr[slot].gen = c->gen; c->xr[slot].flag = 0;
    }
    if ((int)threadIdx.x < A.E) c->counted_to[threadIdx.x] = ch.counted_to[threadIdx.x];
    if ((int)threadIdx.x < PF_RING) c->wq[threadIdx.x] = 0;
    if (ch.nT > 0) {
        // the draw table starts every call empty, from the counters the slots have now
        const size_t par = (size_t)((ch.s_begin + 1) & 1);          // parity of row s_begin - 1
        for (long long p = threadIdx.x; p < A.Np; p += blockDim.x) {
            A.dt_ctr[par * A.Np + p] = A.rng_ctr[p];
            A.dt_filled[par * A.Np + p] = 0;
        }
    }
}

__global__ __launch_bounds__(PF_BS) void k_ledger(KArgs A, int nblocks) {
    ledger_body(A, A.sp, nblocks, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(PF_BS) void k_decide(KArgs A, long long s, int mode, Windows W, int nblocks) {
    decide_body(A, s, mode, W, nblocks);
}

// k_decide of row s with the ledger maintenance of row s-1 riding along in extra workgroups (single-stream pipeline:
// it has to follow the counts of row s-1, which ran inside k_row(s), and precede those of row s)
// Launched with PF_LEDGER_MAXT threads per workgroup: the re-basing of a run list is bound by memory round trips per
// tile, and with 1024 threads the longest list is one tile.  The decide, bookkeeping and run-list workgroups are
// written for PF_BS threads; their other wavefronts leave at once.
// Hardware-specific: the wavefronts that leave do so before the first barrier of the body, and on gfx9-class hardware
// (gfx950 included) a wavefront that has ended no longer counts towards s_barrier, so the remaining four synchronise
// among themselves; HIP itself leaves a barrier under divergent exit undefined.  Since round 2 this kernel is only
// launched with PF_DEBUG_TWO_LAUNCH (the A/B form of the row pipeline); tests/test_gpu_headline.py
// ::test_rings_wrap_many_times[...-8] pins the behaviour on the target.
__global__ __launch_bounds__(PF_LEDGER_MAXT) void k_decide_ledger(KArgs A, long long s, int mode, Windows W, int nblocks, int ledger_nbt) {
    if ((int)blockIdx.x <= nblocks) {
        if (threadIdx.x < PF_BS) decide_body(A, s, mode, W, nblocks);
    } else {
        const int bx = (int)blockIdx.x - (nblocks + 1);
        if (bx >= nblocks || threadIdx.x < PF_BS) ledger_body(A, A.sp ^ 1, nblocks, bx, ledger_nbt);
    }
}

__global__ __launch_bounds__(PF_BS) void k_resample(KArgs A, long long s, int nblocks) {
    Ctrl* c = A.ctrl;
    if (blockIdx.x == 0 && threadIdx.x == 0) { c->gen_prev = c->gen; c->nres_prev = c->n_resample; }
    const long long Np = A.Np;
    const long long i = (long long)blockIdx.x * PF_BS + threadIdx.x;
    const double inv = c->inv_T;
    if (!c->flag) {
        if (i >= Np) return;
        const DState st = state_slot(A, __builtin_amdgcn_readfirstlane(c->cur));
        st.w_post[i] *= inv;
        st.w_pilot[i] *= inv;
        return;
    }
    if (i >= Np) return;
    const int n = A.n;
    const int G = c->gen - 1;                  // the generation that ends here (k_decide already advanced gen)
    const DState src = state_slot(A, __builtin_amdgcn_readfirstlane(c->cur ^ 1));
    const DState dst = state_slot(A, __builtin_amdgcn_readfirstlane(c->cur));
    const int* lo = A.lo + (size_t)(G % A.Gcap) * (Np + 1);
    const double pos = c->cur_pos;
    // ---- role 1: old slot i closes its stretch if it has offspring ----
    unsigned widx = A.widx[i];
    if (lo[i + 1] > lo[i]) {
        double* rec = rec_ptr(A, i, widx);
        rec[0] = src.x_mark[i];
        rec[1] = pos;
        rec[2] = 0.0; rec[3] = 0.0;
        rec[4] = __longlong_as_double((long long)make_meta(1, src.mark_limit[i], -1, n));
        for (int r = 0; r < n - 1; ++r) rec[5 + r] = src.S[(size_t)r * Np + i];
        ++widx;
        A.widx[i] = widx;
    }
    A.gstart[(size_t)((G + 1) % A.Gcap) * Np + i] = widx;
    // ---- role 2: new slot q = i copies its parent (table written by k_decide) ----
    const int q = (int)i;
    const long long a = A.parent[q];
    int ev = (int)c->n_resample - 1;
    if (ev < A.max_trace_events) A.ev_parents[(size_t)ev * Np + q] = (int)a;
    for (int r = 0; r < n - 1; ++r) {
        dst.S[(size_t)r * Np + q] = src.S[(size_t)r * Np + a];
        dst.C[(size_t)(2 * r) * Np + q] = src.C[(size_t)(2 * r) * Np + a];
        dst.C[(size_t)(2 * r + 1) * Np + q] = src.C[(size_t)(2 * r + 1) * Np + a];
    }
    if (A.P > 1) {
        for (int r = 0; r < n - 1; ++r) dst.Pn[(size_t)r * Np + q] = src.Pn[(size_t)r * Np + a];
        const int nmv = src.nm[a];
        dst.nm[q] = nmv;
        for (int k = 0; k < nmv; ++k) {
            dst.Mt[(size_t)k * Np + q] = src.Mt[(size_t)k * Np + a];
            dst.Mb[(size_t)k * Np + q] = src.Mb[(size_t)k * Np + a];
            dst.Mq[(size_t)k * Np + q] = src.Mq[(size_t)k * Np + a];
        }
    }
    // weights: normalise, then adjustment = sum / (N * pilot)   (pc.cpp:350-351)
    double wp = src.w_post[a] * inv;
    double wq = src.w_pilot[a] * inv;
    double sumn = c->S1 * inv;
    double adj = sumn / ((double)Np * wq);
    dst.w_post[q] = wp * adj;
    dst.w_pilot[q] = wq * adj;
    double Lt = src.Ltree[a];
    dst.Ltree[q] = Lt;
    dst.x_mark[q] = pos;
    dst.mark_limit[q] = src.mark_limit[a];
    if (A.apf > 0) dst.lookahead[q] = src.lookahead[a];
    if (A.g_K > 0) dst.ridx[q] = src.ridx[a];
    if (A.n_bias > 0 || A.g_K > 0) {
        // the copy constructor copies the pending factors (particle.cpp:122-123)
        int dc = src.dcount[a];
        dst.dcount[q] = dc;
        dst.total_delayed[q] = src.total_delayed[a];
        row_copy_pending(dst, src, (size_t)Np, q, a, dc);
    }
    double nb = src.next_base[a];
    if (q != lo[a] && pos < A.L) {
        // a copy: draw a fresh recombination position from slot q's own stream (pc.cpp:357-368)
        Lane ln;
        ln.E = A.E; ln.n = n; ln.L = A.L; ln.mu = A.mu; ln.rho = A.rho; ln.seed = A.seed;
        ln.slot = (unsigned)q; ln.stream = 0; ln.ctr = A.rng_ctr[q]; ln.ebuf = A.ebuf[q]; ln.Ltree = Lt;
        ln.S = nullptr; ln.C = nullptr; ln.T = nullptr; ln.I = nullptr; ln.RF = nullptr;
        if (A.g_K > 0) {
            // with a guide: the rate of the copy's segment, the draw limited to the segment
            const int ri = src.ridx[a];
            ln.rho = A.g_rho[ri];
            if (ri + 1 < A.g_K && A.g_pos[ri + 1] < A.L) ln.L = A.g_pos[ri + 1];
        }
        nb = sample_next_base(ln, pos);
        A.rng_ctr[q] = ln.ctr;
        A.ebuf[q] = ln.ebuf;
    }
    dst.next_base[q] = nb;
}

// recompute the level-1 partials from the stored weights (used by pf_finish: smcsmc.cpp:371)
__global__ __launch_bounds__(PF_BS) void k_partials(KArgs A) {
    const Ctrl* c = A.ctrl;
    const long long p = (long long)blockIdx.x * PF_BS + threadIdx.x;
    const bool active = p < A.Np;
    const int lane = threadIdx.x & 63;
    const DState st = state_slot(A, __builtin_amdgcn_readfirstlane(c->cur));
    double w_post = active ? st.w_post[p] : 0.0;
    double w_pilot = active ? st.w_pilot[p] : 0.0;
    if (active) {
        for (int r = 0; r < A.n - 1; ++r) A.snap_S[A.sp][(size_t)r * A.Np + p] = st.S[(size_t)r * A.Np + p];
        A.snap_w[A.sp][p] = w_post; A.snap_xm[A.sp][p] = st.x_mark[p]; A.snap_ml[A.sp][p] = st.mark_limit[p];
        A.snap_widx[A.sp][p] = A.widx[p];
    }
    double sc = wave_hs_scan(w_pilot, lane);       // first: its running maximum below is the longest chain of the five
    double sp = wave_tree_sum(w_post);
    double sq = wave_tree_sum(w_pilot * w_pilot);
    double scp = wave_hs_scan(w_post, lane);
    double scm = wave_max_scan_d(sc, lane);     // running max of the pilot scan (a parallel FP scan need not be monotone)
    long long chunk = p >> 6;
    if (active) { A.scan1[p] = sc; A.scanp2[A.sp][p] = scp; A.scan1m[p] = scm; }
    if (lane == 63 && chunk < (A.Np + 63) / 64) {
        A.chunk_post[chunk] = sp;
        A.chunk_sq[chunk] = sq;
        A.chunk_pil[chunk] = sc;
        A.chunk_pp[chunk] = scp;
        A.chunk_mx1[chunk] = scm;
    }
}

// ------------------------------------------------------------------ k_calibrate (body in pf_lds_body.h)
template <int NM>
__global__ __launch_bounds__(PF_BS) void k_calibrate(KArgs A, unsigned long long seed, long long rep0, long long nrep,
                                                     int* out_epoch, double* out_dist) {
    extern __shared__ double smem[];
    calibrate_lds_body<NM>(A, seed, rep0, nrep, out_epoch, out_dist, smem);
}

// ------------------------------------------------------------------ k_lookahead
// update_lookahead_likelihood (pc.cpp:227-240) with ForestState::includeLookaheadLikelihood (particle.cpp:439-617):
// the previous look-ahead factor leaves the pilot weight, the new one enters it.  Runs after k_extend (the pilot
// weight is a product of the same factors in either order) and rewrites the pilot part of the per-wavefront
// partials that k_decide consumes.  One population.
// The same arithmetic on the register tree, inside the extend role of k_sweep<..., LOOK>, is look_factor (pf_look_reg.h): a fix to one of
// them belongs in both; tests/test_gpu_lookahead_rows.py holds the two to the same bits.
static size_t smem_bytes_la(int n, int E) { return smem_bytes(n, E) + (size_t)PF_BS * (2 * n * 8 + n * 4); }

__global__ __launch_bounds__(PF_BS) void k_lookahead(KArgs A, long long row) {
    extern __shared__ double smem[];
    Smem m = carve(smem, A.n, A.E);
    double* s_lh = (double*)((char*)smem + smem_bytes(A.n, A.E)) + threadIdx.x;       // [n] stride PF_BS
    double* s_mp = s_lh + (size_t)A.n * PF_BS;                                           // [n]
    int* s_par = (int*)((double*)((char*)smem + smem_bytes(A.n, A.E)) + (size_t)2 * A.n * PF_BS) + threadIdx.x;   // [n]
    load_model(A, m);
    __syncthreads();
    const Ctrl* c = A.ctrl;
    const int n = A.n, Q = A.la_Q, D = A.la_D;
    const long long p = (long long)blockIdx.x * PF_BS + threadIdx.x;
    const bool active = p < A.Np;
    const int lane = threadIdx.x & 63;
    double w_pilot = 0.0;
    if (active) {
        const DState st = state_slot(A, __builtin_amdgcn_readfirstlane(c->cur));
        Lane ln = make_lane(A, m, p);
        for (int r = 0; r < n - 1; ++r) {
            LS(ln, r) = st.S[(size_t)r * A.Np + p];
            LC(ln, r, 0) = st.C[(size_t)(2 * r) * A.Np + p];
            LC(ln, r, 1) = st.C[(size_t)(2 * r + 1) * A.Np + p];
        }
        const double Ltree = st.Ltree[p];
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
            double hgt = LS(ln, pr);
            if (A.P > 1) {
                // structured models: the first local node above a leaf may be a migration on its branch (the events
                // of a particle are sorted by time, so the first hit is the lowest)
                const int nmig = st.nm[p];
                for (int mi = 0; mi < nmig; ++mi)
                    if (st.Mb[(size_t)mi * A.Np + p] == i) { hgt = st.Mt[(size_t)mi * A.Np + p]; pr = -2 - mi; break; }
            }
            s_par[i * PF_BS] = pr;
            s_lh[i * PF_BS] = hgt;
            s_mp[i * PF_BS] = 0.0;
        }
        for (int i = 0; i < n; i++) {
            double pp = 0;
            const double si = fsd[i];
            double li = s_lh[i * PF_BS];
            const bool up = unph[i] != 0;
            if (up) li += s_lh[(i + 1) * PF_BS];
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
                        if (s_par[a * PF_BS] == s_par[b * PF_BS]) {
                            double l = s_lh[a * PF_BS];
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
            double p_splitdata = site_lik_lane(ln, one_mask, zero_mask, false, m.t0 + threadIdx.x, m.t1 + threadIdx.x);
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
        // removeLookaheadLikelihood + includeLookaheadLikelihood (particle.hpp:182, particle.cpp:614-616)
        w_pilot = st.w_pilot[p];
        w_pilot /= st.lookahead[p];
        double la_w = 1.0;
        la_w *= likelihood;
        w_pilot *= likelihood;
        st.lookahead[p] = la_w;
        st.w_pilot[p] = w_pilot;
    }
    double sq = wave_tree_sum(w_pilot * w_pilot);
    double sc = wave_hs_scan(w_pilot, lane);
    double scm = wave_max_scan_d(sc, lane);
    long long chunk = p >> 6;
    if (active) { A.scan1[p] = sc; A.scan1m[p] = scm; }
    if (lane == 63 && chunk < (A.Np + 63) / 64) {
        A.chunk_sq[chunk] = sq;
        A.chunk_pil[chunk] = sc;
        A.chunk_mx1[chunk] = scm;
    }
}

// k_lookahead where its scratch columns do not fit beside the tree: at 15 and 16 haplotypes smem_bytes_la is more than the 160 KB a
// workgroup can have (16 haplotypes, 256 lanes: 100 KB of tree columns and 80 KB of scratch), and the launch above is refused.  The same
// factor through look_factor_lds (pf_look_lds.h: k_lookahead's statements with the scratch inside the columns t0 / t1), in the LDS of
// k_extend; the migration events of a structured model are read from the state, as k_lookahead reads them.  Everything around the factor
// is k_lookahead's, statement for statement.  pf_load_lookahead picks it (pf_handle::la_xl) only where k_lookahead cannot run.
struct LookMigG {
    static constexpr bool on = true;
    const DState& st;
    long long p, Np;
    __device__ __forceinline__ int count() const { return st.nm[p]; }
    __device__ __forceinline__ int branch(int mi) const { return st.Mb[(size_t)mi * Np + p]; }
    __device__ __forceinline__ double time(int mi) const { return st.Mt[(size_t)mi * Np + p]; }
};
__global__ __launch_bounds__(PF_BS) void k_lookahead_xl(KArgs A, long long row) {
    extern __shared__ double smem[];
    Smem m = carve(smem, A.n, A.E);
    load_model(A, m);
    __syncthreads();
    const Ctrl* c = A.ctrl;
    const int n = A.n;
    const long long p = (long long)blockIdx.x * PF_BS + threadIdx.x;
    const bool active = p < A.Np;
    const int lane = threadIdx.x & 63;
    double w_pilot = 0.0;
    if (active) {
        const DState st = state_slot(A, __builtin_amdgcn_readfirstlane(c->cur));
        Lane ln = make_lane(A, m, p);
        for (int r = 0; r < n - 1; ++r) {
            LS(ln, r) = st.S[(size_t)r * A.Np + p];
            LC(ln, r, 0) = st.C[(size_t)(2 * r) * A.Np + p];
            LC(ln, r, 1) = st.C[(size_t)(2 * r + 1) * A.Np + p];
        }
        const double Ltree = st.Ltree[p];
        double likelihood;
        if (A.P > 1) likelihood = look_factor_lds(A, ln, row, Ltree, m.t0 + threadIdx.x, m.t1 + threadIdx.x, LookMigG{st, p, A.Np});
        else likelihood = look_factor_lds(A, ln, row, Ltree, m.t0 + threadIdx.x, m.t1 + threadIdx.x);
        // removeLookaheadLikelihood + includeLookaheadLikelihood (particle.hpp:182, particle.cpp:614-616)
        w_pilot = st.w_pilot[p];
        w_pilot /= st.lookahead[p];
        double la_w = 1.0;
        la_w *= likelihood;
        w_pilot *= likelihood;
        st.lookahead[p] = la_w;
        st.w_pilot[p] = w_pilot;
    }
    double sq = wave_tree_sum(w_pilot * w_pilot);
    double sc = wave_hs_scan(w_pilot, lane);
    double scm = wave_max_scan_d(sc, lane);
    long long chunk = p >> 6;
    if (active) { A.scan1[p] = sc; A.scan1m[p] = scm; }
    if (lane == 63 && chunk < (A.Np + 63) / 64) {
        A.chunk_sq[chunk] = sq;
        A.chunk_pil[chunk] = sc;
        A.chunk_mx1[chunk] = scm;
    }
}

// calculate_terminal_branch_length_quantiles (smcsmc.cpp:128-166): one prior tree per lane (Philox stream 3); reports
// every sample's coalescent parent height and the tree length
__global__ __launch_bounds__(PF_BS) void k_tbl(KArgs A, unsigned long long seed, long long rep0, long long nrep,
                                               double* out_h /* [n][nrep] */, double* out_len /* [nrep] */) {
    extern __shared__ double smem[];
    Smem m = carve(smem, A.n, A.E);
    load_model(A, m);
    __syncthreads();
    long long r = (long long)blockIdx.x * PF_BS + threadIdx.x;
    if (r >= nrep) return;
    const int n = A.n;
    Lane ln = make_lane(A, m, rep0 + r);
    ln.seed = seed;
    ln.stream = 3;
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
    out_len[r] = tree_length(ln, n);
    for (int i = 0; i < n; ++i) {
        int pr = -1;
        for (int k = 0; k < n - 1 && pr < 0; ++k)
            if (LC(ln, k, 0) == i || LC(ln, k, 1) == i) pr = k;
        out_h[(size_t)i * nrep + r] = LS(ln, pr);
    }
}

// exp_digamma(c)/c for every event count (particle.cpp:266-272), with the device's own exp / log
__global__ void k_vb_table(const double* counts, long long n, double* out) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = exp_digamma(counts[i]) / counts[i];
}

// ------------------------------------------------------------------ unit-test kernels
__global__ void k_test_math(const double* x, long long n, double* oe, double* ol, double* of) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    oe[i] = dexp(x[i]);
    ol[i] = x[i] > 0 ? dlog(x[i]) : 0.0;
    of[i] = fastexp(x[i]);
}
__global__ void k_test_div(const double* a, const double* b, long long n, double* o) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = a[i] / b[i];
}
__global__ void k_test_uniform(unsigned long long seed, unsigned slot, unsigned stream, unsigned long long first, long long n,
                               double* o) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = philox_uniform(seed, slot, stream, first + (unsigned long long)i);
}

// ------------------------------------------------------------------ k_simulate (body in pf_lds_body.h)
__global__ __launch_bounds__(PF_BS) void k_simulate(KArgs A, unsigned long long seed, int nchunks, long long max_sites,
                                                    double* pos_out, unsigned* mask_out, long long* n_out) {
    extern __shared__ double smem[];
    simulate_lds_body(A, seed, nchunks, max_sites, pos_out, mask_out, n_out, smem);
}

// ------------------------------------------------------------------ host side: the C-ABI, in the headers below and nowhere above
#include "pf_devmem.h"
#include "pf_handle.h"
#include "pf_create.h"
#include "pf_run.h"
#include "pf_get.h"
#include "pf_tools.h"
