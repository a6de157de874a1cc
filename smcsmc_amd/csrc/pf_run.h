// The run layer: which kernels take the rows of a handle, and the host loops that enqueue them.  Included once by pf_hip.hip, behind the
// kernels and pf_handle (one translation unit).

// the particle-independent window rule of extract_and_update_count (count.cpp:363-385)
static Windows host_windows(pf_handle* h, double current_base, bool end_data) {
    const int E = h->E;
    Windows W;
    memset(&W, 0, sizeof(W));
    W.first = E;
    W.end_data = end_data ? 1 : 0;
    for (int e = 0; e < E; ++e) {
        double lagging = end_data ? 0.0 : h->h_lags[e];
        double x_end = current_base - lagging;
        W.a[e] = h->h_counted_to[e];
        if ((x_end - h->h_counted_to[e]) < lagging * 0.1 && W.first > e) {
            W.b[e] = h->h_counted_to[e];
        } else {
            W.b[e] = x_end;
            W.first = std::min(W.first, e);
        }
    }
    for (int e = 0; e < E; ++e) h->h_counted_to[e] = W.b[e];
    return W;
}

static bool timing_on(pf_handle* h, long long s) { return h->timing_period > 0 && (s % h->timing_period) == 0; }

static Windows no_windows(pf_handle* h) {
    Windows W;
    memset(&W, 0, sizeof(W));
    W.first = h->E;
    for (int e = 0; e < h->E; ++e) { W.a[e] = h->h_counted_to[e]; W.b[e] = h->h_counted_to[e]; }
    return W;
}

static bool dbg(const pf_handle* h, int bits) { return (h->debug & bits) != 0; }
// focused sampling (bias heights) or a recombination guide: the BIASED instances
static bool is_biased(const pf_handle* h) { return h->A.n_bias > 0 || h->A.g_K > 0; }
// dynamic LDS of the register-tree kernels outside the row pipeline: the epoch tables and the bias bands
static size_t reg_smem_bytes(int E) { return (size_t)(2 * PF_EPAD + E + 2 * PF_BIAS_MAX + 3) * 8; }
// segment s ends the data (smcsmc.cpp:353-356)
static bool ends_data(const pf_handle* h, long long s) { return h->h_seg_start[s] + h->h_seg_len[s] >= h->h_L; }

// ------------------------------------------------------------------ which path runs when
// The one place that says which runner takes the rows of a handle ("Which path runs when").  pf_run, pf_run_many and
// run_many_refusal switch on it and choose by nothing else.  The values, and what each path launches, are with pf_get_run_path in smcsmc_pf.h.
enum class RunPath {
    General = PF_PATH_GENERAL, TwoLaunch = PF_PATH_TWO_LAUNCH, KPipe = PF_PATH_K_PIPE, Sweep = PF_PATH_SWEEP, SweepSplit = PF_PATH_SWEEP_SPLIT,
    SweepXmp = PF_PATH_SWEEP_XMP, SweepXl = PF_PATH_SWEEP_XL, SweepXlmp = PF_PATH_SWEEP_XLMP
};

// The look-ahead was loaded with PF_LA_ROW_PIPELINE and the handle is one the LOOK instances of k_sweep are built for: one population of at
// most 8 haplotypes with the rings of the row pipeline, no focused sampling, no guide, no -arg, no queue of count workers (k_sweep4q has no
// such instance) and no debug switch that selects a path
static bool look_on_rows(const pf_handle* h) {
    return (h->la_flags & PF_LA_ROW_PIPELINE) && h->P == 1 && h->n <= 8 && !h->wide && h->rings == Rings::Reg && !is_biased(h) && !h->A.rec_trees &&
           h->workers == 0 && !dbg(h, PF_DEBUG_FORCE_LDS | PF_DEBUG_NO_FUSE | PF_DEBUG_TWO_LAUNCH | PF_DEBUG_K_PIPE);
}

// The same for structured models: the look-ahead was loaded with PF_LA_ROW_PIPELINE_MP and the handle is one the LOOK instance of k_sweep_xmp
// is built for -- two to four populations with the rings of their row pipeline (at most 8 haplotypes, the tree in registers, no -arg and no
// debug switch that selects a path: plan_create gives the rings to no other), no focused sampling and no guide
static bool look_on_rows_mp(const pf_handle* h) {
    return (h->la_flags & PF_LA_ROW_PIPELINE_MP) && h->P > 1 && h->rings == Rings::Xmp && !is_biased(h) && !h->A.rec_trees &&
           !dbg(h, PF_DEBUG_FORCE_LDS | PF_DEBUG_NO_FUSE | PF_DEBUG_TWO_LAUNCH | PF_DEBUG_K_PIPE);
}

// And on the per-lane LDS tree, 9 to 16 haplotypes: the look-ahead was loaded with PF_LA_ROW_PIPELINE_LDS and the handle has the rings the LOOK
// instances of k_sweep_xl (one population) or k_sweep_xlmp (structured, PF_FLAG_MP_LDS_ROWS) run on -- create_plan gives them to no handle with
// -arg or a path switch, and the instances take the dynamic LDS of the plain ones, so every handle with the rings qualifies -- no focused
// sampling and no guide
static bool look_on_rows_lds(const pf_handle* h) {
    return (h->la_flags & PF_LA_ROW_PIPELINE_LDS) && (h->rings == Rings::Xl || h->rings == Rings::Xlmp) && !is_biased(h) && !h->A.rec_trees &&
           !dbg(h, PF_DEBUG_FORCE_LDS | PF_DEBUG_NO_FUSE | PF_DEBUG_TWO_LAUNCH | PF_DEBUG_K_PIPE);
}

// `many`: as pf_run_many takes the handle (it refuses General, TwoLaunch and KPipe), otherwise as pf_run does
static RunPath run_path(const pf_handle* h, bool many) {
    // the look-ahead (loaded after creation): on the general kernels, or by its flag in the extend role of k_sweep -- one launch a step at any
    // number of haplotypes up to 8, like focused sampling -- or of k_sweep_xmp, the path a structured model has without a look-ahead, or of
    // k_sweep_xlmp / k_sweep_xl (the latter for pf_run_many only, as without a look-ahead)
    if (h->A.apf != 0) {
        if (look_on_rows(h)) return RunPath::Sweep;
        if (look_on_rows_mp(h)) return RunPath::SweepXmp;
        if (look_on_rows_lds(h)) {
            if (h->rings == Rings::Xlmp) return RunPath::SweepXlmp;
            if (many) return RunPath::SweepXl;
        }
        return RunPath::General;
    }
    // the register-tree kernels of one population, which complete the previous row while loading the particle (fused k_resample)
    if (h->P == 1 && h->n <= 8 && !h->wide && !dbg(h, PF_DEBUG_FORCE_LDS | PF_DEBUG_NO_FUSE)) {
        if (h->rings != Rings::Reg || dbg(h, PF_DEBUG_TWO_LAUNCH)) return RunPath::TwoLaunch;
        if (dbg(h, PF_DEBUG_K_PIPE) && !many) return RunPath::KPipe;      // (k_pipe takes one chunk per launch: several go through k_sweep)
        // at most four haplotypes, no focused sampling, no -arg: a step is two launches unless the switch says one
        return split_shape(h->rings == Rings::Reg, h->P, h->n, is_biased(h), h->A.rec_trees != 0, h->debug) ? RunPath::SweepSplit : RunPath::Sweep;
    }
    if (h->rings == Rings::Xmp) return RunPath::SweepXmp;     // (create_impl gives these rings to no handle with -arg or a path switch)
    if (h->rings == Rings::Xl && many) return RunPath::SweepXl;
    if (h->rings == Rings::Xlmp) return RunPath::SweepXlmp;   // (PF_FLAG_MP_LDS_ROWS; create_plan gives these rings to no handle with -arg or a path switch)
    return RunPath::General;
}
static bool runs_many(RunPath p) { return p >= RunPath::Sweep; }

// ------------------------------------------------------------------ one dispatch per kernel family
template <int V> using ic = std::integral_constant<int, V>;

// The register-tree row kernels (k_extend_reg, k_row, k_pipe, k_sweep*) are instantiated over
//   NM      4 or 8 haplotypes the unrolled tree loops are written for
//   BIASED  is_biased()
//   EXACT   the handle has exactly NM haplotypes and records no trees
//   TREES   -arg (never together with EXACT)
// twelve instances a family.  f is a generic lambda that takes the four as std::integral_constant values.
template <class F>
static void with_row_instance(const pf_handle* h, F&& f) {
    auto pick = [&](auto NM, auto BIASED) {
        if (h->A.rec_trees) f(NM, BIASED, std::false_type(), std::true_type());
        else if (h->n == NM) f(NM, BIASED, std::true_type(), std::false_type());
        else f(NM, BIASED, std::false_type(), std::false_type());
    };
    const bool biased = is_biased(h);
    if (h->n <= 4) { if (biased) pick(ic<4>(), std::true_type()); else pick(ic<4>(), std::false_type()); }
    else { if (biased) pick(ic<8>(), std::true_type()); else pick(ic<8>(), std::false_type()); }
}

// k_count<NM, P>: the record width (4, 8, PF_NMAX, or the wide kernels' own) and 1, 2, PF_PMAX or PF_PWIDE populations (five to eight share the
// last as three and four share PF_PMAX)
template <class F>
static void with_count_instance(const pf_handle* h, F&& f) {
    auto pick = [&](auto P) {
        if constexpr (P < PF_PMAX) { if (h->n <= 4) return f(ic<4>(), P); }       // (three and four populations share the instances of four: none for NM = 4)
        if (h->n <= 8) f(ic<8>(), P); else f(ic<PF_NMAX>(), P);
    };
    if (h->P == 1 && h->wide) f(ic<PF_NMAX_WIDE>(), ic<1>());      // the wide records (descendants in their own word)
    else if (h->P == 1) pick(ic<1>());
    else if (h->P == 2) pick(ic<2>());
    else if (h->P <= PF_PMAX) pick(ic<PF_PMAX>());
    else pick(ic<PF_PWIDE>());
}

// k_sweep_blc<NM, P, BIASED>, the second launch of run_sweep_x: the LDS tree of one population, or a structured model in registers or on the LDS tree
template <class F>
static void with_blc_instance(const pf_handle* h, F&& f) {
    auto pick = [&](auto NM, auto P) { if (is_biased(h)) f(NM, P, std::true_type()); else f(NM, P, std::false_type()); };
    if (h->P == 1) pick(ic<PF_NMAX>(), ic<1>());
    else if (h->n <= 8) { if (h->P == 2) pick(ic<8>(), ic<2>()); else pick(ic<8>(), ic<PF_PMAX>()); }
    // records sixteen wide: the structured models on the LDS tree (RunPath::SweepXlmp)
    else if (h->P == 2) pick(ic<PF_NMAX>(), ic<2>());
    else pick(ic<PF_NMAX>(), ic<PF_PMAX>());
}

static int launch_extend(pf_handle* h, long long s, int fuse = 0) {
    const bool t = timing_on(h, s);
    {
        Timed tm(h, 0, t);
        if (h->P > 1)
            pf_mp_launch_extend(h->A, s, h->smem, h->stream, dbg(h, PF_DEBUG_FORCE_LDS), fuse);
        else if (h->wide)
            pf_wide_launch_extend(h->A, s, h->smem, h->stream);
        else if (h->n <= 8 && !dbg(h, PF_DEBUG_FORCE_LDS))
            with_row_instance(h, [&](auto NM, auto BIASED, auto, auto TREES) {
                hipLaunchKernelGGL((k_extend_reg<NM, BIASED, TREES>), dim3(h->nblocks), dim3(PF_BS), reg_smem_bytes(h->E), h->stream, h->A, s, fuse);
            });
        else
            hipLaunchKernelGGL(k_extend, dim3(h->nblocks), dim3(PF_BS), h->smem, h->stream, h->A, s);
    }
    if (check_launch("k_extend")) return -1;
    if (h->A.apf > 0) {
        if (h->la_xl) hipLaunchKernelGGL(k_lookahead_xl, dim3(h->nblocks), dim3(PF_BS), h->smem_la, h->stream, h->A, s);
        else hipLaunchKernelGGL(k_lookahead, dim3(h->nblocks), dim3(PF_BS), h->smem_la, h->stream, h->A, s);
        return check_launch("k_lookahead");
    }
    return 0;
}

static int launch_decide(pf_handle* h, long long s, int mode, const Windows& W) {
    const bool t = timing_on(h, s);
    // k_decide rewrites what k_count / k_ledger read
    // (window generations, offspring tables): it must not start before the counting stream is done with them
    if (h->ev_cnt) hipStreamWaitEvent(h->stream, h->ev_cnt, 0);
    {
        Timed tm(h, 1, t);
        if (!h->no_count) {
            // the event the counting stream waits on is the kernel's own completion signal (no marker packet between
            // this kernel and the next row's extend)
            h->ev_dec = next_sync_event(h);
            hipExtLaunchKernelGGL(k_decide, dim3(h->nblocks + 1), dim3(PF_BS), 0, h->stream, nullptr, h->ev_dec, 0, h->A, s, mode, W, h->nblocks);
        } else {
            hipLaunchKernelGGL(k_decide, dim3(h->nblocks + 1), dim3(PF_BS), 0, h->stream, h->A, s, mode, W, h->nblocks);
        }
    }
    return check_launch("k_decide");
}

// the lagged counts of the windows W, epochs [W.first, E), on stream st
static void enqueue_count(pf_handle* h, hipStream_t st, const Windows& W) {
    const int first = W.first;
    with_count_instance(h, [&](auto NM, auto P) {
        if constexpr (NM == PF_NMAX && P == 1) {
            if (h->rings == Rings::Xl && h->A.cw_off) {        // count_wgs set: the columns as wide as pf_run_many makes them
                hipLaunchKernelGGL((k_count_cw<PF_NMAX, 1>), dim3(h->ncw, h->E - first), dim3(PF_BS), 0, st, h->A, first, W);
                return;
            }
        }
        if constexpr (P > 1) {
            if (h->A.anc) {                                    // sample times: the recombination opportunity without the samples that enter later
                hipLaunchKernelGGL((k_count_anc<NM, P>), dim3(h->nblocks, h->E - first), dim3(PF_BS), 0, st, h->A, first, W);
                return;
            }
        }
        hipLaunchKernelGGL((k_count<NM, P>), dim3(h->nblocks, h->E - first), dim3(PF_BS), 0, st, h->A, first, W);
    });
    h->fin_pending = true;
}

static int launch_count(pf_handle* h, long long s, const Windows& W) {
    if (h->no_count) return 0;
    if (W.first >= h->E) return 0;
    const bool t = timing_on(h, s);
    if (h->ev_dec) hipStreamWaitEvent(h->cstream, h->ev_dec, 0);
    {
        Timed tm(h, 2, t, h->cstream);
        enqueue_count(h, h->cstream, W);
    }
    return check_launch("k_count");
}

// ancestor-ledger maintenance of this step (no-op unless the step resampled); closes the step on the counting stream
static int launch_ledger(pf_handle* h, long long) {
    if (h->no_count) return 0;
    if (h->ev_dec) hipStreamWaitEvent(h->cstream, h->ev_dec, 0);
    hipLaunchKernelGGL(k_ledger, dim3(h->nblocks + PF_LEDGER_BLOCKS), dim3(PF_BS), 0, h->cstream, h->A, h->nblocks);
    h->ev_cnt = next_sync_event(h);
    hipEventRecord(h->ev_cnt, h->cstream);
    return check_launch("k_ledger");
}

static int launch_resample(pf_handle* h, long long s) {
    const bool t = timing_on(h, s);
    {
        Timed tm(h, 3, t);
        hipLaunchKernelGGL(k_resample, dim3(h->nblocks), dim3(PF_BS), 0, h->stream, h->A, s, h->nblocks);
    }
    return check_launch("k_resample");
}

static double seg_pos(pf_handle* h, long long s) {
    return std::min(h->h_seg_start[s] + h->h_seg_len[s], h->h_L);
}

// Single steps.  update and count of one segment share the window set: pf_update_segment evaluates the
// window rule for segment s (the bookkeeping workgroup of k_decide needs it), pf_count launches the sums.
int pf_update_segment(pf_handle* h, int64_t s) {
    HIPCHK(hipSetDevice(h->device));
    if (s < 0 || s >= h->n_segs) { g_err = "segment index out of range"; return -1; }
    h->step_windows = host_windows(h, seg_pos(h, s), false);
    h->A.sp = (int)(s & 1);
    if (launch_extend(h, s)) return -1;
    return launch_decide(h, s, 0, h->step_windows);
}
int pf_count(pf_handle* h, int64_t s, int end_data) {
    HIPCHK(hipSetDevice(h->device));
    (void)end_data;
    return launch_count(h, s, h->step_windows);
}
int pf_resample(pf_handle* h, int64_t s) {
    HIPCHK(hipSetDevice(h->device));
    int rc = launch_resample(h, s);
    if (!rc) rc = launch_ledger(h, s);
    h->seg_done = std::max<long long>(h->seg_done, s + 1);
    return rc;
}

// keep the timing-event pool bounded without stalling the queue: only harvest finished spans
static void trim_spans(pf_handle* h) {
    if (h->spans.empty() || hipEventQuery(h->spans.front().b) != hipSuccess) return;
    size_t done = 0;
    while (done < h->spans.size() && hipEventQuery(h->spans[done].b) == hipSuccess) ++done;
    std::vector<pf_handle::Span> rest(h->spans.begin() + done, h->spans.end());
    h->spans.resize(done);
    harvest_spans(h);
    h->spans = rest;
}

// The single-stream pipeline of the register-tree kernels.  Per row two launches and nothing else:
//   k_row(s)           extend over row s (completing row s-1 while loading)  ||  lagged counts of row s-1
//   k_decide_ledger(s) normalisation / ESS / offspring table of row s        ||  ancestor-ledger upkeep of row s-1
// Stream order provides every dependency; the two halves of each launch touch disjoint (immutable or parity
// double-buffered) data.  The last row of the call is flushed with the stand-alone kernels so that the state is
// whole when the call returns.
static int run_single_stream(pf_handle* h, long long s_begin, long long s_end) {
    bool pending = false;             // counts + ledger of the previous row still to be launched
    Windows Wprev = no_windows(h);
    // whatever the two-stream kernels of an earlier call left on the counting stream must be done first
    if (h->ev_cnt) { hipStreamWaitEvent(h->stream, h->ev_cnt, 0); h->ev_cnt = nullptr; }
    for (long long s = s_begin; s < s_end; ++s) {
        h->step_windows = host_windows(h, seg_pos(h, s), false);
        h->A.sp = (int)(s & 1);
        const bool t = timing_on(h, s);
        {
            Timed tm(h, 0, t);
            const int cf = pending ? Wprev.first : h->E, nb = h->nblocks;
            const int fuse = s > s_begin ? 1 : 0;
            const int ncount = cf < h->E ? nb * (h->E - cf) : 0;
            with_row_instance(h, [&](auto NM, auto BIASED, auto EXACT, auto TREES) {
                hipLaunchKernelGGL((k_row<NM, BIASED, EXACT, TREES>), dim3(nb + ncount), dim3(PF_BS), reg_smem_bytes(h->E), h->stream, h->A, s, fuse, nb, cf, Wprev);
            });
            if (pending && Wprev.first < h->E) h->fin_pending = true;
        }
        if (check_launch("k_row")) return -1;
        {
            Timed tm(h, 1, t);
            // decide and ledger workgroups each hold ~120 KB of LDS, one per CU: keep the launch within one wave of 256 CUs
            const int lroom = 256 - (h->nblocks + 1) - h->nblocks;
            const int lnbt = pending ? h->nblocks + std::max(16, std::min(PF_LEDGER_BLOCKS, lroom)) : 0;
            hipLaunchKernelGGL(k_decide_ledger, dim3(h->nblocks + 1 + lnbt), dim3(PF_LEDGER_MAXT), 0, h->stream, h->A, s, 0, h->step_windows,
                               h->nblocks, lnbt);
        }
        if (check_launch("k_decide")) return -1;
        pending = true;
        Wprev = h->step_windows;
        h->seg_done = s + 1;
        const bool last = (s + 1 == s_end) || ends_data(h, s);
        if (last) {
            // flush: complete the row, then its counts and ledger with the stand-alone kernels (same stream)
            if (launch_resample(h, s)) return -1;
            if (Wprev.first < h->E) {
                enqueue_count(h, h->stream, Wprev);
                h->k_launches[2] += 1;
            }
            hipLaunchKernelGGL(k_ledger, dim3(h->nblocks + PF_LEDGER_BLOCKS), dim3(PF_BS), 0, h->stream, h->A, h->nblocks);
            if (check_launch("k_count/k_ledger")) return -1;
            break;
        }
        if ((s & 1023) == 1023) trim_spans(h);
    }
    return 0;
}

// The single-launch pipeline (k_pipe): per row ONE launch on one stream, see the kernel's header.  Rows [s_begin, s_end)
// are followed by two flush launches (completion of the last row with the bookkeeping / ledger / counts still owed)
// after which the handle's state is in the form the general kernels expect.
static int run_pipeline(pf_handle* h, long long s_begin, long long s_end) {
    if (s_begin >= s_end) return 0;
    const int nb = h->nblocks, E = h->E;
    // whatever the two-stream kernels of an earlier call left on the counting stream must be done first
    if (h->ev_cnt) { hipStreamWaitEvent(h->stream, h->ev_cnt, 0); h->ev_cnt = nullptr; }
    hipLaunchKernelGGL(k_pipe_seed, dim3(1), dim3(1), 0, h->stream, h->A, (int)((s_begin + PF_RING - 1) & (PF_RING - 1)));
    Windows W1 = no_windows(h), W2 = no_windows(h);      // windows of rows s-1 and s-2
    long long last = s_begin - 1;                        // last row extended so far
    const int nL_full = nb + h->ledger_wgs;
    // one launch: extend row s (or only complete row s-1 / nothing), bookkeeping of row s-1, ledger + counts of row s-2
    auto launch = [&](long long s, bool extend, bool have_b, bool have_lc, int set_cur) -> int {
        PipeLaunch PL;
        memset(&PL, 0, sizeof(PL));
        PL.nb = nb; PL.nblk = nb;
        PL.row.extend = extend ? 1 : 0;
        PL.row.complete = (s > s_begin && s - 1 <= last && (extend || have_b)) ? 1 : 0;
        if (!extend && !have_b) PL.row.complete = 0;
        PL.row.slot_prev = PL.row.complete ? (int)((s - 1) & (PF_RING - 1)) : -1;
        PL.row.slot_out = (int)(s & (PF_RING - 1));
        PL.row.pos_prev = (PL.row.complete && s > s_begin) ? seg_pos(h, s - 1) : 0.0;   // row s - 1 of the second flush step may lie past the table
        PL.b_slot = have_b ? (int)((s - 1) & (PF_RING - 1)) : -1;
        PL.b_row = s - 1;
        PL.b_pos = have_b ? seg_pos(h, s - 1) : 0.0;
        PL.b_set_cur = set_cur;
        PL.lc_slot = (have_lc && !h->no_count) ? (int)((s - 2) & (PF_RING - 1)) : -1;
        PL.live_slot = (int)((s - 1) & (PF_RING - 1));
        PL.nL = PL.lc_slot >= 0 ? nL_full : 0;
        PL.ncw = h->ncw;
        PL.nT = 0; PL.row.draws = 0;               // k_pipe keeps no draw table
        const int ncount_wg = (PL.lc_slot >= 0 && W2.first < E) ? h->cw_off[E - W2.first] : 0;
        if (ncount_wg > 0) h->fin_pending = true;
        const bool t = extend && timing_on(h, s);
        {
            Timed tm(h, 0, t);
            if (!extend) h->k_launches[0] -= 1;          // flush launches are not rows
            const dim3 grid((unsigned)(PL.nb + 1 + PL.nL + ncount_wg));
            with_row_instance(h, [&](auto NM, auto BIASED, auto EXACT, auto TREES) {
                hipLaunchKernelGGL((k_pipe<NM, BIASED, EXACT, TREES>), grid, dim3(PF_BS), h->smem_pipe, h->stream, h->A, s, PL, W1);
            });
        }
        return check_launch("k_pipe");
    };
    long long s = s_begin;
    for (; s < s_end; ++s) {
        if (launch(s, true, s > s_begin, s > s_begin + 1, -1)) return -1;
        last = s;
        W2 = W1;
        W1 = host_windows(h, seg_pos(h, s), false);
        h->step_windows = W1;
        h->seg_done = s + 1;
        if ((s & 1023) == 1023) trim_spans(h);
        if (ends_data(h, s)) { ++s; break; }
    }
    // flush 1: complete row `last` into the next ring slot (the general kernels continue from there), its bookkeeping,
    // ledger + counts of the row before it; flush 2: ledger + counts of row `last`
    if (launch(last + 1, false, true, last - 1 >= s_begin, (int)((last + 1) & (PF_RING - 1)))) return -1;
    W2 = W1;
    if (launch(last + 2, false, false, true, -1)) return -1;
    return 0;
}

// Rows [s_begin, s_end) of several chunks (handles on one device, same shape) in lockstep, one k_sweep launch per step on
// the leader's stream.  Every chunk is bit-identical to its own pf_run (tests/test_gpu_sweep.py): a chunk never reads
// another chunk's memory, and the launch geometry a chunk sees is the one k_pipe gives it.
static void launch_sweep(pf_handle* h, const dim3& grid, long long t) {
    const dim3 blk(PF_BS);
    const size_t lds = h->smem_pipe;
    if (h->A.apf > 0) {
        // RunPath::Sweep with a look-ahead (look_on_rows): the LOOK instances, the same launch otherwise
        auto look = [&](auto NM, auto EXACT) { hipLaunchKernelGGL((k_sweep<NM, false, EXACT, false, true>), grid, blk, lds, h->stream, h->d_sweep, t, h->nblocks); };
        if (h->n <= 4) { if (h->n == 4) look(ic<4>(), std::true_type()); else look(ic<4>(), std::false_type()); }
        else { if (h->n == 8) look(ic<8>(), std::true_type()); else look(ic<8>(), std::false_type()); }
        return;
    }
    with_row_instance(h, [&](auto NM, auto BIASED, auto EXACT, auto TREES) {
        if constexpr (NM == 4 && !BIASED) {
            // the headline instance has kernels of its own: k_sweep4, with the count workers' queue (4q) and with time stamps (4t, 4q)
            const bool traced = h->d_trace && t >= h->trace_t0 && t < h->trace_t0 + h->trace_n;
            if constexpr (!TREES) {                 // (neither the queue nor the trace with -arg: create_impl, pf_set_wg_trace)
                if (h->h_sweep[0].workers > 0) {
                    if (traced) hipLaunchKernelGGL((k_sweep4q<EXACT, true>), grid, blk, lds, h->stream, h->d_sweep, t, h->nblocks);
                    else hipLaunchKernelGGL((k_sweep4q<EXACT, false>), grid, blk, lds, h->stream, h->d_sweep, t, h->nblocks);
                    return;
                }
                if (traced) { hipLaunchKernelGGL((k_sweep4t<EXACT>), grid, blk, lds, h->stream, h->d_sweep, t, h->nblocks); return; }
            }
            hipLaunchKernelGGL((k_sweep4<EXACT, TREES>), grid, blk, lds, h->stream, h->d_sweep, t, h->nblocks);
        } else {
            hipLaunchKernelGGL((k_sweep<NM, BIASED, EXACT, TREES>), grid, blk, lds, h->stream, h->d_sweep, t, h->nblocks);
        }
    });
}

// two handles pf_run_many accepts, each on its own, can share the launches of a step
static bool sweep_compatible(const pf_handle* a, const pf_handle* b) {
    const RunPath path = run_path(a, true);
    const bool x = path == RunPath::SweepXmp || path == RunPath::SweepXl || path == RunPath::SweepXlmp;
    // the look-ahead: off in both, or the same level, flags (both bits) and table sizes in both (one kernel instance and one set of loop bounds a launch)
    const bool look = a->A.apf == b->A.apf && (a->A.apf == 0 || (a->la_flags == b->la_flags && a->A.la_D == b->A.la_D && a->A.la_Q == b->A.la_Q));
    return look && a->device == b->device && a->Np == b->Np && a->n == b->n && a->E == b->E && a->P == b->P && is_biased(a) == is_biased(b) &&
           a->A.rec_trees == b->A.rec_trees && a->ncw == b->ncw && a->workers == b->workers && a->ledger_wgs == b->ledger_wgs && path == run_path(b, true) && a->cw_off == b->cw_off && a->smem_pipe == b->smem_pipe && a->no_count == b->no_count &&
           (a->A.dt_tab != nullptr) == (b->A.dt_tab != nullptr) &&
           // two launches a step: what they take from the leader (the extend launch's LDS -- n = 12 does not run with n = 16 -- and the capacities)
           (!x || (a->smem_sweep_x == b->smem_sweep_x && a->A.dcap == b->A.dcap && a->A.n_bias == b->A.n_bias)) &&
           ((path != RunPath::SweepXmp && path != RunPath::SweepXlmp) || (a->A.mcap == b->A.mcap && a->A.pcap == b->A.pcap));
}

// completion events of the last sixteen extend launches (ev_x) and of the last sixteen launches of the other roles (ev_blc)
static int sweep_event_ring(pf_handle* h) {
    if (!h->ev_x.empty()) return 0;
    // all thirty-two or none: a vector left half filled would pass for complete on the next call, and launches with null
    // completion events lose the ordering between the two streams without a word
    std::vector<hipEvent_t> ev(32, nullptr);
    bool ok = true;
    for (auto& e : ev) if (ok && hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) { e = nullptr; ok = false; }
    if (!ok) {
        for (auto e : ev) if (e) hipEventDestroy(e);
        g_err = "hipEventCreate failed";
        return -1;
    }
    h->ev_x.assign(ev.begin(), ev.begin() + 16); h->ev_blc.assign(ev.begin() + 16, ev.end());
    return 0;
}

// The frame of a sweep, the same for the three runners below; what they launch in the middle of a step, and the events and waits that
// order those launches, are their own.  Steps are counted from 0: step t extends row s_begin + t, the last two steps are flushes.
struct SweepFrame {
    pf_handle* const* hs; int nh; long long s_begin;
    pf_handle* h;                     // the leader: a sweep runs on its streams, with its table
    int nb, nL_full;
    bool two_streams;                 // the second launch of a step on the counting stream (event ring, seed event, closing wait)
    long long steps = 0;
    hipEvent_t seeded = nullptr;      // two_streams: the table and the seed are in place
    std::vector<Windows> W1, W2;      // per chunk: windows of rows s - 1 and s - 2

    SweepFrame(pf_handle* const* hs_, int nh_, long long s_begin_, bool two_streams_)
        : hs(hs_), nh(nh_), s_begin(s_begin_), h(hs_[0]), nb(hs_[0]->nblocks), nL_full(hs_[0]->nblocks + hs_[0]->ledger_wgs), two_streams(two_streams_) {}

    // the other handles' streams, and anything they still have in flight, come first
    int join() {
        for (int k = 0; k < nh; ++k) {
            pf_handle* g = hs[k];
            if (g->ev_cnt) { hipStreamWaitEvent(h->stream, g->ev_cnt, 0); g->ev_cnt = nullptr; }
            if (k > 0) {
                hipEvent_t ev = next_sync_event(g);
                hipEventRecord(ev, g->stream);
                hipStreamWaitEvent(h->stream, ev, 0);
            }
        }
        return two_streams ? sweep_event_ring(h) : 0;
    }
    // the per-chunk table in the leader's device buffer (split: SweepChunk::split of every chunk), the seed and the windows;
    // 1: there are steps to run, 0: none, -1: failed
    int table(long long s_end, int split) {
        if (h->d_sweep_cap < nh) {
            // one allocation: the row headers of the chunks, chunk 0's last, and behind them the chunk table (sweep_head_of, pf_pipe.h)
            if (h->d_sweep_base && hipStreamSynchronize(h->stream) != hipSuccess) return -1;
            h->sweep_mem.clear();
            h->d_sweep_base = nullptr; h->d_sweep = nullptr; h->d_sweep_cap = 0;
            if (h->sweep_mem.reserve(&h->d_sweep_base, (sizeof(SweepHead) * PF_RING + sizeof(SweepChunk)) * (size_t)nh)) {
                h->d_sweep_base = nullptr; g_err = "hipMalloc of the chunk table failed"; return -1;
            }
            h->d_sweep = (SweepChunk*)(h->d_sweep_base + sizeof(SweepHead) * PF_RING * (size_t)nh);
            h->d_sweep_cap = nh;
        }
        // the table of the previous call may still be read by its launches: a fresh host copy per call, uploaded in stream order
        if (hipStreamSynchronize(h->stream) != hipSuccess) { g_err = "hipStreamSynchronize failed"; return -1; }
        h->h_sweep.assign((size_t)nh, SweepChunk());
        for (int k = 0; k < nh; ++k) {
            pf_handle* g = hs[k];
            SweepChunk& ch = h->h_sweep[k];
            memset(&ch, 0, sizeof(ch));
            ch.A = g->A;
            ch.s_begin = s_begin;
            long long e = std::min<long long>(s_end, g->n_segs), last = s_begin - 1;
            for (long long s = s_begin; s < e; ++s) { last = s; if (ends_data(g, s)) break; }
            ch.s_last = last;
            for (int q = 0; q < h->E; ++q) ch.counted_to[q] = g->h_counted_to[q];
            ch.no_count = g->no_count ? 1 : 0;
            ch.nL_full = nL_full;
            ch.ncw = g->ncw;
            ch.nblk = g->nblocks;
            ch.nT = (g->A.dt_tab && g->P == 1) ? g->nblocks : 0;
            ch.split = split;
            ch.workers = g->workers;
            ch.trace = h->d_trace; ch.trace_t0 = h->trace_t0; ch.trace_n = h->d_trace ? h->trace_n : 0; ch.trace_stride = h->trace_stride;
            if (last >= s_begin) steps = std::max(steps, last - s_begin + 3);
        }
        if (steps == 0) return 0;
        // the row headers of the call (SweepHead, pf_pipe.h): PF_RING entries a chunk, from the chunk's pointers and s_begin / s_last
        // (read by k_sweep4, k_sweep4p, k_sweep4q and k_sweep4t only: launch_sweep, run_sweep_split), uploaded with the chunk table in one copy
        const size_t head_bytes = sizeof(SweepHead) * PF_RING * (size_t)nh, chunk_bytes = sizeof(SweepChunk) * (size_t)nh;
        h->h_table.assign(head_bytes + chunk_bytes, 0);
        SweepHead* heads_end = (SweepHead*)(h->h_table.data() + head_bytes);
        if (h->P == 1 && h->n <= 4 && !is_biased(h))
            for (int k = 0; k < nh; ++k)
                for (int j = 0; j < PF_RING; ++j) *sweep_head_of(heads_end, k, j) = sweep_head_entry(h->h_sweep[k].A, h->h_sweep[k], j);
        memcpy(h->h_table.data() + head_bytes, h->h_sweep.data(), chunk_bytes);
        if (hipMemcpyAsync((char*)h->d_sweep - head_bytes, h->h_table.data(), head_bytes + chunk_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            g_err = "upload of the chunk table failed"; return -1;
        }
        hipLaunchKernelGGL(k_sweep_seed, dim3(nh), dim3(PF_BS), 0, h->stream, h->d_sweep);
        if (two_streams) {
            // the counting stream starts behind the table and the seed
            seeded = next_sync_event(h);
            hipEventRecord(seeded, h->stream);
        }
        W1.resize((size_t)nh); W2.resize((size_t)nh);
        for (int k = 0; k < nh; ++k) { W1[k] = no_windows(hs[k]); W2[k] = W1[k]; }
        return 1;
    }
    // Ring slot reuse with two streams: the extend launch of step t overwrites the slot of row t - PF_RING, which the counts read in step
    // t - PF_RING + 2.  One wait every eight steps, for the second launch of seven steps ago, covers the eight steps that
    // follow (t + 7 - 14 <= t - 7); between two waits the extend launches are dispatched back to back.
    // (sweep_ring_awaited, pf_pipe.h)
    void ring_wait(long long t) const {
        if (const long long u = sweep_ring_awaited(t); u >= 0) hipStreamWaitEvent(h->stream, blc_done(u), 0);
    }
    // whether anything waits for the second launch of step u: the ring wait of step u + 7, or leave().  One definition for both sides
    // (run_sweep_split signals only where this says so): a wait on an entry that step u did not record would return at once, on the
    // record an earlier step left there.
    bool blc_awaited(long long u) const { return sweep_blc_awaited(u, steps); }
    hipEvent_t x_done(long long t) const { return h->ev_x[(size_t)(t & 15)]; }        // completion of step t's extend launch ...
    hipEvent_t blc_done(long long t) const { return h->ev_blc[(size_t)(t & 15)]; }    // ... and of its second launch
    // Ledger and count workgroups per chunk in step t.  They belong to row s - 2, whose windows (W2) the host knows as well as the device
    // does: the grid ends with the last epoch column any chunk needs (epochs before a chunk's first moving one are not launched at all)
    int lc_wgs(long long t) const {
        int columns = 0;
        bool any_lc = false;
        for (int k = 0; k < nh; ++k)
            if (t >= 2 && s_begin + t - 2 <= h->h_sweep[k].s_last && !hs[k]->no_count) { any_lc = true; columns = std::max(columns, h->E - W2[k].first); }
        const int workers = h->h_sweep[0].workers;
        return workers > 0 ? (any_lc ? workers : 0) : nL_full + h->cw_off[columns];
    }
    // after step t: W1 / W2 become the windows of rows s and s - 1 of every chunk
    void step_done(long long t) {
        if ((t & 1023) == 1023) trim_spans(h);
        const long long s = s_begin + t;
        for (int k = 0; k < nh; ++k) {
            pf_handle* g = hs[k];
            W2[k] = W1[k];
            if (s <= h->h_sweep[k].s_last) {
                W1[k] = host_windows(g, seg_pos(g, s), false);
                g->step_windows = W1[k];
                if (W1[k].first < g->E && !g->no_count) g->fin_pending = true;
            } else {
                W1[k] = no_windows(g);
            }
        }
    }
    // each chunk's own stream continues after the sweep
    int leave() {
        h->k_launches[0] -= 2;                                      // flush steps are not rows
        // what follows on any chunk's stream waits for the last launch of the other roles
        if (two_streams) hipStreamWaitEvent(h->stream, blc_done(steps - 1), 0);
        for (int k = 0; k < nh; ++k) {
            pf_handle* g = hs[k];
            const long long last = h->h_sweep[k].s_last;
            if (last >= s_begin) g->seg_done = last + 1;
            if (k > 0) {
                hipEvent_t ev = next_sync_event(h);
                hipEventRecord(ev, h->stream);
                hipStreamWaitEvent(g->stream, ev, 0);
            }
        }
        return 0;
    }
};

// Every role of a step in one k_sweep launch on the leader's stream.
//   per step t:  k_sweep(t)
static int run_sweep(pf_handle* const* hs, int nh, long long s_begin, long long s_end) {
    if (s_begin >= s_end) return 0;
    SweepFrame F(hs, nh, s_begin, false);
    pf_handle* h = F.h;
    const int nb = F.nb, E = h->E;
    F.join();
    if (h->trace_n > 0 && !h->d_trace) {
        // pf_set_wg_trace: room for the largest grid a step of these chunks can have
        const int nT = (h->A.dt_tab && h->P == 1) ? nb : 0;
        h->trace_stride = nh * (nb + 1 + nT + F.nL_full + h->cw_off[E]);
        h->trace_words = (size_t)h->trace_n * (size_t)h->trace_stride * 4;
        if (h->trace_mem.alloc(&h->d_trace, h->trace_words, h->stream)) { h->d_trace = nullptr; g_err = "hipMalloc of the workgroup trace failed"; return -1; }
    }
    if (const int rc = F.table(s_end, 0); rc <= 0) return rc;
    for (long long t = 0; t < F.steps; ++t) {
        const unsigned per_chunk = (unsigned)(nb + 1 + h->h_sweep[0].nT + F.lc_wgs(t));
        const dim3 grid(per_chunk, (unsigned)nh);          // (pf_bx() / pf_chunk(), pf_device.h)
        {
            Timed tm(h, 0, timing_on(h, s_begin + t));
            launch_sweep(h, grid, t);
        }
        if (check_launch("k_sweep")) return -1;
        F.step_done(t);
    }
    return F.leave();
}

// One or several chunks in lockstep as TWO launches per step (the default for one population, at most four haplotypes, no focused sampling;
// PF_DEBUG_ONE_LAUNCH = run_sweep): the extend, bookkeeping and draw roles of all chunks
// (k_sweep4, or k_sweep4p where every extend workgroup can have a compute unit of its own; one launch after the other on the leader's stream: the chain of dependent loads that is the critical path of a step) and
// their ledger and count roles (k_sweep_blc4, on the counting stream, behind the extend launch of the step before by its completion
// signal and paced by the sixteen-slot ring as in run_sweep_x).  The second launch needs no dynamic LDS -- that is the bookkeeping
// role's -- and fewer registers than the extend role: four of its workgroups share a compute unit where the single launch has room for
// three, and its tail no longer holds up the next row's extend role.  Same bits as run_sweep.
//   per step t:  [every 8 steps: stream waits blc_done(t - 7)]  k_sweep4(t), signalling x_done(t) at the end of a batch
//   per batch:   cstream waits x_done(last t of the batch); k_sweep_blc4(u) for every step u of the batch, signalling blc_done(u) where a wait reads it
// Completion signals of the second launches: the counting stream is the longer chain of a row, and a signal is a packet of its own behind the
// kernel.  Only two waits read one -- the ring wait of step u + 7 (SweepFrame::ring_wait: steps u with (u & 7) == 1) and leave() (the last step) --
// so only those launches carry one (SweepFrame::blc_awaited); the others are plain launches.  (PF_DEBUG_SIGNAL_ALL_COUNTS: every one, the A/B.)
// The invariant: every hipStreamWaitEvent on an ev_blc entry waits for a record made by the launch it means, IN THIS CALL.  The entries outlive
// a call, and a wait on one that its step did not record returns at once, on what an earlier step or call left there: the extend role would
// overwrite a ring slot the counts still read, and nothing would report it.  That is why the signalling steps and the awaited steps are one
// definition (sweep_ring_awaited, pf_pipe.h) and not two conditions that happen to agree, and why the record of step u is enqueued (with its batch, at most
// three steps later) before the wait of step u + 7 is.
static int run_sweep_split(pf_handle* const* hs, int nh, long long s_begin, long long s_end) {
    if (s_begin >= s_end) return 0;
    SweepFrame F(hs, nh, s_begin, true);
    pf_handle* h = F.h;
    const int nb = F.nb;
    if (F.join()) return -1;
    if (const int rc = F.table(s_end, 2); rc <= 0) return rc;
    // The paired form of the extend role (k_sweep4p, pf_pair.h: 128 particles a workgroup, a weight wavefront beside each tree wavefront) where every
    // extend workgroup of the call can have a compute unit of its own -- one or two headline chunks; with more the chip is full, a helper wavefront
    // would take its slot from another chunk's chain, and the one-wavefront form stays.  (vb_coal multiplies the weights inside the loop: those
    // handles keep the one-wavefront form too.)
    const int nbp = (int)((h->Np + PF_PAIR_N - 1) / PF_PAIR_N);
    bool paired = !dbg(h, PF_DEBUG_NO_PAIR) && (long long)nh * nbp <= pf_device_cus(h->device);
    for (int k = 0; k < nh; ++k) if (hs[k]->A.vb_coal || dbg(hs[k], PF_DEBUG_NO_PAIR)) paired = false;
    for (int k = 0; k < nh; ++k) hs[k]->row_form = paired ? PF_ROW_FORM_PAIRED : PF_ROW_FORM_SINGLE;
    const int nbx = paired ? nbp : nb;                      // extend workgroups of a chunk
    if (paired && !h->pair_lds_set) {
        // (the ring of the pairs is static LDS: with the tables of the decision the workgroup asks for more than 64 KB; once per handle)
        hipError_t rc = hipSuccess;
        with_row_instance(h, [&](auto NM, auto BIASED, auto EXACT, auto TREES) {
            if constexpr (NM == 4 && !BIASED && !TREES) rc = hipFuncSetAttribute((const void*)k_sweep4p<EXACT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem_pipe);
        });
        if (rc != hipSuccess) { g_err = "k_sweep4p: the LDS of the paired row kernel was refused (PF_DEBUG_NO_PAIR runs the other form)"; return -1; }
        h->pair_lds_set = true;
    }
    const dim3 gx((unsigned)(nbx + 1 + h->h_sweep[0].nT), (unsigned)nh), blk(PF_BS);
    // (at most four: the second launch of step t - 7 must be enqueued when step t waits for it.  Several chunks: eight 20 Mb chunks 1.205e5 ->
    // 1.248e5 segments/s with two, 1.272e5 with four.  One chunk was the same with any while its extend launch took 26 us; at 23 us the
    // completion signal on every extend launch is what a row waits for -- 20 Mb, round 12: 4.00e4 segments/s with one, 4.27e4 with two or four)
    const long long batch = std::max(1, std::min(4, h->split_batch > 0 ? h->split_batch : 4));
    std::vector<unsigned> pending_grid((size_t)batch, 1u);
    const bool queue = h->h_sweep[0].workers > 0;          // pf_params.count_workers: the second launch takes its items off a queue
    const bool signal_all = dbg(h, PF_DEBUG_SIGNAL_ALL_COUNTS);   // A/B: a completion signal on every second launch, as up to round 19
    hipStreamWaitEvent(h->cstream, F.seeded, 0);
    for (long long t = 0; t < F.steps; ++t) {
        F.ring_wait(t);
        // The second launches follow in batches of `batch` steps: only the last extend launch of a batch carries a completion signal, and the
        // batch's second launches wait for that one (each needs the extend launch of the step before it: complete by then).
        const bool batch_end = ((t + 1) % batch) == 0 || t == F.steps - 1;
        {
            Timed tm(h, 0, timing_on(h, s_begin + t));
            with_row_instance(h, [&](auto NM, auto BIASED, auto EXACT, auto TREES) {
                if constexpr (NM == 4 && !BIASED && !TREES) {      // (RunPath::SweepSplit is no other instance)
                    if (paired) {
                        if (batch_end) hipExtLaunchKernelGGL((k_sweep4p<EXACT>), gx, blk, h->smem_pipe, h->stream, nullptr, F.x_done(t), 0, h->d_sweep, t, nbx);
                        else hipLaunchKernelGGL((k_sweep4p<EXACT>), gx, blk, h->smem_pipe, h->stream, h->d_sweep, t, nbx);
                    } else if (batch_end) hipExtLaunchKernelGGL((k_sweep4<EXACT, false>), gx, blk, h->smem_pipe, h->stream, nullptr, F.x_done(t), 0, h->d_sweep, t, nb);
                    else hipLaunchKernelGGL((k_sweep4<EXACT, false>), gx, blk, h->smem_pipe, h->stream, h->d_sweep, t, nb);
                }
            });
        }
        if (check_launch(paired ? "k_sweep4p (extend, bookkeeping and draw roles)" : "k_sweep4 (extend, bookkeeping and draw roles)")) return -1;
        pending_grid[(size_t)(t % batch)] = (unsigned)(1 + F.lc_wgs(t));
        if (batch_end) {
            hipStreamWaitEvent(h->cstream, F.x_done(t), 0);
            for (long long u = t - (t % batch); u <= t; ++u) {
                const dim3 grid(pending_grid[(size_t)(u % batch)], (unsigned)nh);
                const bool signal = signal_all || F.blc_awaited(u);
                with_row_instance(h, [&](auto NM, auto BIASED, auto EXACT, auto TREES) {
                    if constexpr (NM == 4 && !BIASED && !TREES) {
                        if (queue) {
                            if (signal) hipExtLaunchKernelGGL((k_sweep_blc4q<EXACT>), grid, blk, 0, h->cstream, nullptr, F.blc_done(u), 0, h->d_sweep, u);
                            else hipLaunchKernelGGL((k_sweep_blc4q<EXACT>), grid, blk, 0, h->cstream, h->d_sweep, u);
                        } else if (signal) hipExtLaunchKernelGGL((k_sweep_blc4<EXACT>), grid, blk, 0, h->cstream, nullptr, F.blc_done(u), 0, h->d_sweep, u);
                        else hipLaunchKernelGGL((k_sweep_blc4<EXACT>), grid, blk, 0, h->cstream, h->d_sweep, u);
                    }
                });
            }
            if (check_launch("k_sweep_blc (ledger and count roles)")) return -1;
        }
        F.step_done(t);
    }
    return F.leave();
}

// Structured models (register-tree kernel) on the row pipeline, one chunk or several in lockstep.  Per step two launches for all
// of them: the extend role (k_sweep_xmp, with the decision on the previous row in its prologue; grid = particle blocks x chunks) on
// the leader's filter stream, the bookkeeping / ledger / count roles (k_sweep_blc, grid = workgroups per chunk x chunks) on the
// leader's counting stream -- separate launches because the extend workgroups' LDS (their trees' migration events) would be
// allocated to every count workgroup too.  Step t's second launch needs the extend launch of step t - 1 (partials, offspring
// table, records), the extend launch of step t must not overwrite ring slot t & (PF_RING - 1) before the counts of step t - 2 are done:
// one wait each way per step, on the kernels' own completion signals; the extend role does not read anything the other
// launch writes (it keeps its own note of n_resample / generation, Ctrl::xr).  k_decide, its boundary and the wait of the
// next row on the previous row's ledger upkeep are gone from the critical stream.  A chunk never reads another chunk's memory and
// takes nothing from the launch geometry but its own blockIdx.x: every chunk is bit-identical to its own pf_run
// (tests/test_gpu_sweep_structured.py).
// The same runner serves one population with the tree in LDS (RunPath::SweepXl: 9 to 16 haplotypes, several chunks through pf_run_many):
// the extend role is k_sweep_xl (256 particles per workgroup, 100 KB of tree columns at 16 haplotypes -- the same reason for two
// launches), the other roles k_sweep_blc<16, 1, *>, and the table says so with SweepChunk::split = 1 (sweep_plan: the extend role
// runs ahead).  Everything else -- the table, the seed, the two waits per step, the windows -- is shared line for line, which is why
// this is one function with two launch sites and not a sibling (tests/test_gpu_sweep_lds.py).
// And a third pair: structured models on the LDS tree (RunPath::SweepXlmp: 9 to 16 haplotypes, handles created with PF_FLAG_MP_LDS_ROWS, pf_run and
// pf_run_many alike).  The extend role is k_sweep_xlmp (pf_mp.hip: 64 particles a workgroup, tree and migration list in LDS), the other roles
// k_sweep_blc<16, 2 or PF_PMAX, *>; the table is that of the structured models in registers (split = 0: sweep_plan knows by P > 1 that the extend
// role runs ahead).  tests/test_gpu_sweep_structured_lds.py.
//   per step t:  [every 8 steps: stream waits blc_done(t - 7)]  k_sweep_xmp / k_sweep_xl / k_sweep_xlmp(t) signalling x_done(t);
//                cstream waits x_done(t - 1) (step 0: the seed); k_sweep_blc(t) signalling blc_done(t)
static int run_sweep_x(pf_handle* const* hs, int nh, long long s_begin, long long s_end, RunPath path) {
    if (s_begin >= s_end) return 0;
    const bool xl = path == RunPath::SweepXl, xlmp = path == RunPath::SweepXlmp;
    SweepFrame F(hs, nh, s_begin, true);
    pf_handle* h = F.h;
    if (F.join()) return -1;
    if (const int rc = F.table(s_end, xl ? 1 : 0); rc <= 0) return rc;
    for (long long t = 0; t < F.steps; ++t) {
        F.ring_wait(t);
        {
            Timed tm(h, 0, timing_on(h, s_begin + t));
            if (xl) {
                const dim3 gx((unsigned)F.nb, (unsigned)nh), bx(PF_BS);
                // a look-ahead on this path (run_path: look_on_rows_lds, never with focused sampling): the LOOK instance, the same launch otherwise
                if (h->A.apf > 0) hipExtLaunchKernelGGL((k_sweep_xl<false, true>), gx, bx, h->smem_sweep_x, h->stream, nullptr, F.x_done(t), 0, h->d_sweep, t);
                else if (is_biased(h)) hipExtLaunchKernelGGL((k_sweep_xl<true>), gx, bx, h->smem_sweep_x, h->stream, nullptr, F.x_done(t), 0, h->d_sweep, t);
                else hipExtLaunchKernelGGL((k_sweep_xl<false>), gx, bx, h->smem_sweep_x, h->stream, nullptr, F.x_done(t), 0, h->d_sweep, t);
            } else if (xlmp) {
                pf_mp_launch_sweep_xl(h->A, h->d_sweep, nh, t, h->smem_sweep_x, h->stream, F.x_done(t));
            } else {
                pf_mp_launch_sweep_x(h->A, h->d_sweep, nh, t, h->smem_sweep_x, h->stream, F.x_done(t));
            }
        }
        if (check_launch(xl ? "k_sweep_xl" : (xlmp ? "k_sweep_xlmp" : "k_sweep_xmp"))) return -1;
        hipStreamWaitEvent(h->cstream, t >= 1 ? F.x_done(t - 1) : F.seeded, 0);
        const dim3 grid((unsigned)(1 + F.lc_wgs(t)), (unsigned)nh), blk(PF_BS);
        with_blc_instance(h, [&](auto NM, auto P, auto BIASED) {
            hipExtLaunchKernelGGL((k_sweep_blc<NM, P, BIASED>), grid, blk, h->smem_pipe, h->cstream, nullptr, F.blc_done(t), 0, h->d_sweep, t);
        });
        if (check_launch("k_sweep_blc")) return -1;
        F.step_done(t);
    }
    return F.leave();
}

// why pf_run_many would refuse these handles (null: it would not)
static const char* run_many_refusal(pf_handle* const* handles, int32_t n_handles) {
    if (n_handles < 1 || !handles || !handles[0]) return "pf_run_many: no handles";
    pf_handle* h = handles[0];
    for (int k = 0; k < n_handles; ++k) {
        pf_handle* g = handles[k];
        if (!g) return "pf_run_many: null handle";
        // Out of scope: structured models above 8 haplotypes without PF_FLAG_MP_LDS_ROWS, -arg above 8 haplotypes, a look-ahead without PF_LA_ROW_PIPELINE (one
        // population) or PF_LA_ROW_PIPELINE_MP (structured) or PF_LA_ROW_PIPELINE_LDS (9 to 16 haplotypes) or on a handle that does not qualify for it
        // (look_on_rows, look_on_rows_mp, look_on_rows_lds),
        // the wide kernels (more than 16 haplotypes); pf_run on one such handle stays on the general kernels
        if (g->P > PF_PMAX)
            return "pf_run_many: a model of more than four populations runs on the general kernels (pf_run), one chunk after the other: the row pipelines stop at four populations";
        if (g->A.anc)
            return "pf_run_many: a model with sample times (-eI, ancient samples) runs on the general kernels (pf_run), one chunk after the other: the row pipelines have no instance for them";
        if (!runs_many(run_path(g, true)))
            return "pf_run_many: the chunks must run on the row pipeline (one population of at most 16 haplotypes, or a structured model of two to "
                   "four populations with the tree in registers, at most 8 haplotypes, or of 9 to 16 haplotypes created with PF_FLAG_MP_LDS_ROWS -- every chunk of the group then; a look-ahead only with PF_LA_ROW_PIPELINE on one "
                   "population of at most 8 haplotypes or with PF_LA_ROW_PIPELINE_MP on such a structured model, without focused sampling; "
                   "no -arg above 8 haplotypes, no debug switch that selects another path)"
                   "; at 9 to 16 haplotypes a look-ahead only with PF_LA_ROW_PIPELINE_LDS, one population or a structured model created with PF_FLAG_MP_LDS_ROWS";
        if (!sweep_compatible(h, g)) return "pf_run_many: the chunks must share device, particle count, haplotypes (and with them the form of the tree: registers up to 8, "
                                              "LDS columns of one width from 9 to 16), populations, epochs and options (mig_cap and piece_cap of a structured model among them, and the look-ahead: all without, or one level and one table size)";
        for (int j = 0; j < k; ++j) if (handles[j] == g) return "pf_run_many: a handle appears twice";
    }
    return nullptr;
}

int pf_can_run_many(pf_handle* const* handles, int32_t n_handles) {
    return run_many_refusal(handles, n_handles) == nullptr ? 1 : 0;
}

int pf_get_run_path(pf_handle* h, int many) {
    const RunPath p = run_path(h, many != 0);
    return many && !runs_many(p) ? -1 : (int)p;
}

int pf_get_row_form(pf_handle* h) { return h->row_form; }

// the general kernels: one launch per role and row
static int run_general(pf_handle* h, long long s_begin, long long s_end) {
    // structured models on the register-tree kernel: the next row's extend completes this row while it loads (two
    // launches per row on the main stream instead of three); the last row of the call is completed by k_resample
    const bool mp_fuse = h->P > 1 && pf_mp_can_fuse(h->A, dbg(h, PF_DEBUG_FORCE_LDS)) && h->A.apf == 0 && !dbg(h, PF_DEBUG_NO_FUSE);
    long long owed = -1;              // row decided but not completed yet
    for (long long s = s_begin; s < s_end; ++s) {
        h->step_windows = host_windows(h, seg_pos(h, s), false);
        h->A.sp = (int)(s & 1);
        if (launch_extend(h, s, owed >= 0 ? 1 : 0)) return -1;
        if (launch_decide(h, s, 0, h->step_windows)) return -1;
        if (mp_fuse) owed = s;
        else if (launch_resample(h, s)) return -1;
        if (launch_count(h, s, h->step_windows)) return -1;
        if (launch_ledger(h, s)) return -1;
        h->seg_done = s + 1;
        if (ends_data(h, s)) break;
        if ((s & 1023) == 1023) trim_spans(h);
    }
    if (owed >= 0 && launch_resample(h, owed)) return -1;
    return 0;
}

// rows [s_begin, s_end) of the handles (one, unless a sweep) on the path run_path() named
static int run_on(RunPath path, pf_handle* const* hs, int nh, long long s_begin, long long s_end) {
    for (int k = 0; k < nh; ++k) hs[k]->row_form = PF_ROW_FORM_NONE;      // (run_sweep_split says which form it ran)
    switch (path) {
    case RunPath::General: return run_general(hs[0], s_begin, s_end);
    case RunPath::TwoLaunch: return run_single_stream(hs[0], s_begin, s_end);
    case RunPath::KPipe: return run_pipeline(hs[0], s_begin, s_end);
    case RunPath::Sweep: return run_sweep(hs, nh, s_begin, s_end);
    case RunPath::SweepSplit: return run_sweep_split(hs, nh, s_begin, s_end);
    case RunPath::SweepXmp: case RunPath::SweepXl: case RunPath::SweepXlmp: return run_sweep_x(hs, nh, s_begin, s_end, path);
    }
    return -1;
}

int pf_run_many(pf_handle* const* handles, int32_t n_handles, int64_t s_begin, int64_t s_end) {
    if (const char* why = run_many_refusal(handles, n_handles)) { g_err = why; return -1; }
    HIPCHK(hipSetDevice(handles[0]->device));
    if (s_begin < 0) { g_err = "segment range out of bounds"; return -1; }        // a chunk with fewer rows sits the call out
    return run_on(run_path(handles[0], true), handles, n_handles, s_begin, s_end);
}

int pf_run(pf_handle* h, int64_t s_begin, int64_t s_end) {
    HIPCHK(hipSetDevice(h->device));
    if (s_begin < 0 || s_end > h->n_segs) { g_err = "segment range out of bounds"; return -1; }
    return run_on(run_path(h, false), &h, 1, s_begin, s_end);
}
