// smcsmc_amd/csrc/pf_handle.h -- the handle of the C-ABI: what it owns, how it is created (refuse, plan, allocate, prepare) and loaded.
// Included once, by pf_hip.hip, behind the kernels.
#pragma once

// The row pipeline a handle's rings were allocated for at creation (create_plan, pf_create.h); run_path() (pf_run.h) picks the runner from this, the debug
// switches and the look-ahead.  None: two copies of the state, the general kernels or k_row.  Reg: one population, n <= 8, tree in registers
// (k_sweep*).  Xmp: two to four populations, n <= 8 (k_sweep_xmp).  Xl: one population, 9 <= n <= 16, tree in LDS (k_sweep_xl, pf_run_many only).
// Xlmp: two to four populations, 9 <= n <= 16, tree and migration list in LDS, only with PF_FLAG_MP_LDS_ROWS (k_sweep_xlmp; pf_run and pf_run_many).
enum class Rings { None, Reg, Xmp, Xl, Xlmp };
// The shape RunPath::SweepSplit takes -- run_path (pf_run.h) asks here, and so does create_impl, which gives these handles one entry of rg_blkcnt
// per wavefront: one population of at most four haplotypes on the rings of the row pipeline, no focused sampling or guide, no -arg, no switch
// to another path.  (A look-ahead loaded later takes the handle off the path; every writer and reader of rg_blkcnt goes by KArgs::blk_gran.)
static bool split_shape(bool reg_rings, int P, int n, bool biased, bool rec_trees, int debug) {
    return reg_rings && P == 1 && n <= 4 && !biased && !rec_trees &&
           !(debug & (PF_DEBUG_FORCE_LDS | PF_DEBUG_NO_FUSE | PF_DEBUG_TWO_LAUNCH | PF_DEBUG_K_PIPE | PF_DEBUG_ONE_LAUNCH | PF_DEBUG_FORCE_WIDE));
}

struct pf_handle {
    int device = 0;
    hipStream_t stream = nullptr;      // filter stream: k_extend, k_decide, k_resample
    hipStream_t cstream = nullptr;     // counting stream: k_count, k_ledger (off the critical path)
    std::vector<hipEvent_t> sync_ev;   // ring of events ordering the two streams
    size_t sync_next = 0;
    hipEvent_t ev_dec = nullptr, ev_cnt = nullptr;   // last decide / last count+ledger
    KArgs A;
    DevMem mem;                        // every device array of the handle; those of an earlier pf_load_segments / pf_load_lookahead stay until it goes
    std::vector<double> h_lags, h_counted_to;
    double h_L = 0;
    std::vector<double> h_seg_start, h_seg_len;
    long long n_segs = 0;
    long long seg_done = 0;
    int E = 0, n = 0, P = 1;
    long long Np = 0;
    int nblocks = 0;
    size_t smem = 0, smem_la = 0;
    bool la_xl = false;           // the look-ahead of the general kernels is k_lookahead_xl (15 and 16 haplotypes: k_lookahead's LDS is more than a workgroup has)
    int max_trace_events = 0;
    bool finished = false;
    bool fin_pending = false;     // k_count partials not yet folded into the totals
    Windows step_windows;         // windows of the step being processed
    int la_flags = 0;             // pf_lookahead.flags of the look-ahead in force (PF_LA_ROW_PIPELINE, PF_LA_ROW_PIPELINE_MP, PF_LA_ROW_PIPELINE_LDS; 0 without one)
    bool pair_lds_set = false;    // the LDS limit of k_sweep4p has been raised for this handle's instance (run_sweep_split)
    int row_form = 0;             // PF_ROW_FORM_*: what the last call ran (pf_get_row_form)
    int debug = 0;                // pf_params.debug: the PF_DEBUG_* switches that select a path are read from here (run_path)
    Rings rings = Rings::None;
    bool wide = false;            // one population on the wide kernels of pf_wide.hip: nsam > PF_NMAX, or PF_DEBUG_FORCE_WIDE (testing)
    bool no_count = false;        // PF_DEBUG_NO_COUNT: no lagged counting, no ledger upkeep (profiling)
    size_t smem_pipe = 0;         // dynamic LDS of the row pipeline's launches (rings != None)
    int ncw = 0;                  // count workgroups per epoch in the row pipeline (pf_params.count_wgs): the most a column gets
    int ledger_wgs = 192;         // workgroups per step that re-base the older generations' run lists after a resampling (beside one per particle block)
    int workers = 0;              // pf_params.count_workers: workgroups per step that take the ledger and count items off a queue (0: one workgroup per item)
    std::vector<int> cw_off;      // [E + 1] first count workgroup of the j-th column, oldest epoch first (KArgs::cw_off)
    int split_batch = 0;          // run_sweep_split: the second launches enqueued in batches of this many steps behind one completion signal (0: chosen by the runner)
    unsigned long long* d_trace = nullptr;   // pf_set_wg_trace (leader of a pf_run_many call): four words per workgroup and step
    size_t trace_words = 0;
    int trace_t0 = 0, trace_n = 0, trace_stride = 0, trace_grid[3] = {0, 0, 0};
    size_t smem_sweep_x = 0;      // dynamic LDS of the extend launch of run_sweep_x (rings Xmp, Xl, Xlmp)
    std::vector<hipEvent_t> ev_x, ev_blc;   // completion of the last 16 extend / bookkeeping-ledger-count launches
    bool no_spec_stage = false;   // PF_DEBUG_NO_SPEC_STAGE
    SweepChunk* d_sweep = nullptr; // device table of the chunks this handle leads through k_sweep
    char* d_sweep_base = nullptr;  // the allocation: the chunks' row headers (SweepHead, PF_RING entries a chunk) in front of the chunk table
    DevMem sweep_mem, trace_mem;   // own d_sweep_base and d_trace: one buffer each, cleared and allocated again when it has to grow
    std::vector<char> h_table;     // host copy of both as uploaded
    int d_sweep_cap = 0;
    std::vector<SweepChunk> h_sweep;
    // timing
    int timing_period = 0;
    struct Span { hipEvent_t a, b; int k; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> ev_pool;
    double span_overhead_ms = 0;  // what a pair of HIP events brackets when nothing is between them (subtracted from every span)
    double k_ms[4] = {0, 0, 0, 0};
    long long k_launches[4] = {0, 0, 0, 0};
    long long k_timed[4] = {0, 0, 0, 0};

    // zeroed on the filter stream
    template <class T>
    int alloc(T** p, size_t count) { return mem.alloc(p, count, stream); }
    pf_handle() = default;
    pf_handle(const pf_handle&) = delete;
    pf_handle& operator=(const pf_handle&) = delete;
    // whatever stage creation reached: what was not made is null or empty
    ~pf_handle() {
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        if (cstream) hipStreamSynchronize(cstream);
        mem.clear(); sweep_mem.clear(); trace_mem.clear();
        for (auto e : sync_ev) if (e) hipEventDestroy(e);
        for (auto e : ev_x) if (e) hipEventDestroy(e);
        for (auto e : ev_blc) if (e) hipEventDestroy(e);
        if (cstream) hipStreamDestroy(cstream);
        for (auto& sp : spans) { hipEventDestroy(sp.a); hipEventDestroy(sp.b); }
        for (auto e : ev_pool) hipEventDestroy(e);
        if (stream) hipStreamDestroy(stream);
    }
};

// the handle's Ctrl as the device left it (the caller has synchronised: pf_sync)
static int read_ctrl(pf_handle* h, Ctrl& c) {
    HIPCHK(hipMemcpy(&c, h->A.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost));
    return 0;
}

// Bucket table of r_search_lut for an ascending table tab[0..E) with tab[0] = 0: lut[j] = the largest e with tab[e] <= the
// lower edge of bucket j, bucket j = the doubles whose upper sixteen bits are kbase + j (bucket 0 also takes everything
// below, the last bucket everything above).  Returns false when the table spans more buckets than PF_LUT_N, when a bucket
// holds more than two entries (the two probes of the device would not finish the search) or when the probes could leave
// the padded table.
static bool lut_build(const double* tab, int E, unsigned char* lut, int* kbase) {
    auto key = [](double v) { uint64_t b; memcpy(&b, &v, 8); return (int)(b >> 48); };
    auto edge = [](int k) { uint64_t b = (uint64_t)k << 48; double v; memcpy(&v, &b, 8); return v; };
    if (E + 2 > PF_EPAD) return false;
    for (int e = 0; e < E; ++e) if (!(tab[e] >= 0.0) || !std::isfinite(tab[e]) || (e > 0 && tab[e] < tab[e - 1])) return false;
    if (E == 1 || !(tab[E - 1] > 0.0)) { memset(lut, 0, PF_LUT_N); *kbase = 0x3ff0; return E == 1; }
    int first = 1;
    while (first < E && tab[first] == 0.0) ++first;              // entries equal to tab[0] (an epoch of zero intensity at the start)
    const int kb = key(tab[first]) - 1;
    if (kb < 1 || key(tab[E - 1]) > kb + PF_LUT_N - 2) return false;
    *kbase = kb;
    for (int j = 0; j < PF_LUT_N; ++j) {
        const double lo = j == 0 ? 0.0 : edge(kb + j);
        int e = 0;
        while (e + 1 < E && tab[e + 1] <= lo) ++e;
        lut[j] = (unsigned char)e;
        if (j + 1 < PF_LUT_N) {
            const double hi = edge(kb + j + 1);
            int inside = 0;
            for (int q = e + 1; q < E && tab[q] < hi; ++q) ++inside;
            if (inside > 2) return false;
        } else if (e != E - 1) return false;
    }
    return true;
}

// cumulative coalescence intensity at the epoch starts, in exactly this order of operations on both sides of the
// parity tests: Hc[0] = 0, Hc[e+1] = Hc[e] + (T[e+1] - T[e]) * inv2N[e]
static std::vector<double> cumulative_intensity(const double* T, const std::vector<double>& inv2N, int E) {
    std::vector<double> H(E, 0.0);
    for (int e = 0; e + 1 < E; ++e) H[e + 1] = H[e] + (T[e + 1] - T[e]) * inv2N[e];
    return H;
}

int pf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// compute units of a device (asked once; 0: unknown)
int pf_device_cus(int device) {
    static std::vector<int> cus;
    static std::mutex mu;             // (handles on several devices may be driven from several threads)
    if (device < 0) return 0;
    std::lock_guard<std::mutex> lock(mu);
    if ((int)cus.size() <= device) cus.resize((size_t)device + 1, 0);
    if (cus[(size_t)device] == 0 && hipDeviceGetAttribute(&cus[(size_t)device], hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus[(size_t)device] = 0;
    return cus[(size_t)device];
}

// Ancient samples (-eI): the model's sample times where the caller says that the field is there (PF_MODEL_SAMPLE_TIMES), else null -- the field is
// never read without the bit.
static const double* model_sample_times(const pf_model* m) { return (m->flags & PF_MODEL_SAMPLE_TIMES) ? m->sample_times : nullptr; }
// What every entry point that takes sample times asks of them (null: they are fine), in the words of `who`.  One population is not in scope: its
// kernels count the lineages of an interval by rank.
static const char* sample_times_refusal(const pf_model* m, std::string& msg, const char* who) {
    const double* st = model_sample_times(m);
    if (!st) return nullptr;
    auto fail = [&](const std::string& what) { msg = std::string(who) + ": " + what; return msg.c_str(); };
    if (m->n_pops < 2) return fail("sample times (-eI, ancient samples) need a structured model: the one-population kernels count lineages by rank");
    double lo = st[0];
    for (int i = 0; i < m->nsam; ++i) {
        bool found = false;
        for (int e = 0; e < m->n_epochs; ++e) found |= m->change_times[e] == st[i];
        if (!found) return fail("sample time " + std::to_string(st[i]) + " of sample " + std::to_string(i) + " is not an entry of change_times (a sample enters at the start of an epoch)");
        if (i && st[i] < st[i - 1]) return fail("sample times must ascend with the sample index");
        lo = std::min(lo, st[i]);
    }
    if (lo != 0.0) return fail("the smallest sample time must be 0");
    return nullptr;
}

// per-epoch, per-population tables of a structured model (scrm Model::population_size / migration_rate /
// single_mig_pop), prepared exactly as the oracle's fill_model does
struct MpTables {
    std::vector<double> inv2Np, mrate, mtot;
    std::vector<double> cum_coal, cum_mig;     // [E*P] integrals of 1/2N_p and of the total emigration rate of p from 0 to the epoch start
    std::vector<double> next_join;             // [E] start of the next epoch after e that moves a whole population (-ej), +inf if none
    std::vector<int> jmap, spop, next_join_epoch;
};
static int build_mp_tables(const pf_model* m, MpTables& t) {
    const int E = m->n_epochs, P = m->n_pops, n = m->nsam;
    t.inv2Np.resize((size_t)E * P);
    for (int i = 0; i < E * P; ++i) t.inv2Np[i] = 1.0 / (2.0 * m->pop_sizes[i]);
    t.mrate.assign((size_t)E * P * P, 0.0);
    if (m->mig_rates) t.mrate.assign(m->mig_rates, m->mig_rates + (size_t)E * P * P);
    t.mtot.assign((size_t)E * P, 0.0);
    for (int e = 0; e < E; ++e)
        for (int a = 0; a < P; ++a) {
            double sum = 0.0;
            for (int b = 0; b < P; ++b) if (b != a) sum += t.mrate[((size_t)e * P + a) * P + b];
            t.mtot[(size_t)e * P + a] = sum;
        }
    t.jmap.resize((size_t)E * P);
    for (int e = 0; e < E; ++e)
        for (int a = 0; a < P; ++a) {
            int cur = a;
            for (int step = 0; step <= P && m->single_mig; ++step) {
                int nxt = cur;
                for (int b = 0; b < P; ++b) {
                    double pr = m->single_mig[((size_t)e * P + cur) * P + b];
                    if (pr != 0.0 && pr != 1.0) { g_err = "partial single migration events (-es/-eps style) are not supported"; return -1; }
                    if (pr == 1.0 && b != cur) { nxt = b; break; }
                }
                if (nxt == cur) break;
                if (step == P) { g_err = "Cycle detected when moving individuals between populations"; return -1; }
                cur = nxt;
            }
            t.jmap[(size_t)e * P + a] = cur;
        }
    // Tables of the structured walk (pf_mp.h mp_coalesce): the hazard of a lineage over a stretch that spans epochs is
    // a difference of these; accumulated in this order, which the oracle restates.
    t.cum_coal.assign((size_t)E * P, 0.0);
    t.cum_mig.assign((size_t)E * P, 0.0);
    for (int e = 0; e + 1 < E; ++e)
        for (int a = 0; a < P; ++a) {
            const double dt = m->change_times[e + 1] - m->change_times[e];
            t.cum_coal[(size_t)(e + 1) * P + a] = t.cum_coal[(size_t)e * P + a] + dt * t.inv2Np[(size_t)e * P + a];
            t.cum_mig[(size_t)(e + 1) * P + a] = t.cum_mig[(size_t)e * P + a] + dt * t.mtot[(size_t)e * P + a];
        }
    t.next_join.assign(E, INFINITY);
    t.next_join_epoch.assign(E, E);
    const double* tau = model_sample_times(m);
    for (int e = E - 2; e >= 0; --e) {
        bool moves = false;
        for (int a = 0; a < P; ++a) moves |= t.jmap[(size_t)(e + 1) * P + a] != a;
        // ancient samples: the walk ends a stretch where samples enter too (mp_coalesce counts them in there)
        for (int i = 0; i < n && tau; ++i) moves |= tau[i] > 0.0 && tau[i] == m->change_times[e + 1];
        t.next_join[e] = moves ? m->change_times[e + 1] : t.next_join[e + 1];
        t.next_join_epoch[e] = moves ? e + 1 : t.next_join_epoch[e + 1];
    }
    t.spop.assign(n, 0);
    if (m->sample_pops) t.spop.assign(m->sample_pops, m->sample_pops + n);
    for (int v : t.spop) if (v < 0 || v >= P) { g_err = "sample population out of range"; return -1; }
    return 0;
}

// The model's tables on the device, for every entry point that launches a kernel: A.T, A.inv2N (population 0), A.recflags (the model's for a
// handle, 3 -- record everything -- elsewhere), A.Hc, and for a structured model the tables of build_mp_tables.  Copied on `stream`, which is
// synchronised once at the end.  Hc_host: the host copy of A.Hc, for the caller that builds the search table from it.
static int upload_model_tables(const pf_model* m, KArgs& A, DevMem& mem, hipStream_t stream, bool model_recflags = false,
                               std::vector<double>* Hc_host = nullptr) {
    const int E = m->n_epochs, P = m->n_pops;
    std::vector<double> inv2N(E);
    for (int e = 0; e < E; ++e) inv2N[e] = 1.0 / (2.0 * m->pop_sizes[(size_t)e * P]);
    const std::vector<double> Hc = cumulative_intensity(m->change_times, inv2N, E);
    const std::vector<int> rf(E, 3);
    int rc = mem.upload(&A.T, m->change_times, E, stream) || mem.upload(&A.inv2N, inv2N.data(), E, stream) ||
             mem.upload(&A.recflags, model_recflags ? m->record_flags : rf.data(), E, stream) || mem.upload(&A.Hc, Hc.data(), E, stream);
    MpTables t;
    if (!rc && P > 1)
        rc = build_mp_tables(m, t) || mem.upload(&A.next_join_epoch, t.next_join_epoch.data(), t.next_join_epoch.size(), stream) ||
             mem.upload(&A.cum_coal, t.cum_coal.data(), t.cum_coal.size(), stream) || mem.upload(&A.cum_mig, t.cum_mig.data(), t.cum_mig.size(), stream) ||
             mem.upload(&A.next_join, t.next_join.data(), t.next_join.size(), stream) || mem.upload(&A.inv2Np, t.inv2Np.data(), t.inv2Np.size(), stream) ||
             mem.upload(&A.mig_rate, t.mrate.data(), t.mrate.size(), stream) || mem.upload(&A.mig_tot, t.mtot.data(), t.mtot.size(), stream) ||
             mem.upload(&A.join_map, t.jmap.data(), t.jmap.size(), stream) || mem.upload(&A.sample_pop, t.spop.data(), t.spop.size(), stream);
    // ancient samples: [n] times, [E] the length of epoch e times the samples that enter after it (what k_count_anc takes off a tree's length inside e)
    std::vector<double> anc;
    if (!rc && P > 1 && model_sample_times(m)) {
        const double* st = model_sample_times(m);
        anc.assign(st, st + m->nsam);
        for (int e = 0; e < E; ++e) {
            int later = 0;
            for (int i = 0; i < m->nsam; ++i) later += st[i] > m->change_times[e];
            anc.push_back(later && e + 1 < E ? (double)later * (m->change_times[e + 1] - m->change_times[e]) : 0.0);
        }
        rc = mem.upload(&A.anc, anc.data(), anc.size(), stream);
    }
    // (after a failure too: the copies queued so far read this function's vectors)
    const hipError_t synchronised = hipStreamSynchronize(stream);
    if (rc) return -1;
    HIPCHK(synchronised);
    if (Hc_host) *Hc_host = Hc;
    return 0;
}

static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_err = std::string(what) + ": " + hipGetErrorString(e); return -1; }
    return 0;
}

static int harvest_spans(pf_handle* h) {
    for (auto& sp : h->spans) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, sp.a, sp.b));
        h->k_ms[sp.k] += std::max(0.0, (double)ms - h->span_overhead_ms);
        h->k_timed[sp.k] += 1;
        h->ev_pool.push_back(sp.a);
        h->ev_pool.push_back(sp.b);
    }
    h->spans.clear();
    return 0;
}

static hipEvent_t get_event(pf_handle* h) {
    if (!h->ev_pool.empty()) { hipEvent_t e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

struct Timed {
    pf_handle* h; int k; bool on; hipEvent_t a, b; hipStream_t st;
    Timed(pf_handle* h_, int k_, bool on_, hipStream_t st_ = nullptr) : h(h_), k(k_), on(on_), st(st_ ? st_ : h_->stream) {
        h->k_launches[k] += 1;
        if (on) { a = get_event(h); b = get_event(h); hipEventRecord(a, st); }
    }
    ~Timed() {
        if (on) { hipEventRecord(b, st); h->spans.push_back({a, b, k}); }
    }
};

static hipEvent_t next_sync_event(pf_handle* h) {
    hipEvent_t e = h->sync_ev[h->sync_next];
    h->sync_next = (h->sync_next + 1) % h->sync_ev.size();
    return e;
}

int pf_init_prior(pf_handle* h, double initial_position) {
    HIPCHK(hipSetDevice(h->device));
    if (h->P > 1)
        pf_mp_launch_init(h->A, initial_position, h->smem, h->stream);
    else if (h->wide)
        pf_wide_launch_init(h->A, initial_position, h->smem, h->stream);
    else
        hipLaunchKernelGGL(k_init, dim3(h->nblocks), dim3(PF_BS), h->smem, h->stream, h->A, initial_position);
    if (check_launch("k_init")) return -1;
    if (h->A.lmap_opp) {
        HIPCHK(hipMemsetAsync(h->A.lmap_opp, 0, (size_t)h->A.lmap_bins * 8, h->stream));
        HIPCHK(hipMemsetAsync(h->A.lmap_cnt, 0, (size_t)(h->n + 2) * h->A.lmap_bins * 8, h->stream));
    }
    std::fill(h->h_counted_to.begin(), h->h_counted_to.end(), 0.0);
    HIPCHK(hipMemsetAsync(h->A.partial, 0, (size_t)h->E * h->A.nbx * h->A.ncol * 8, h->stream));
    h->fin_pending = false;
    h->ev_dec = nullptr; h->ev_cnt = nullptr;
    h->seg_done = 0;
    h->finished = false;
    return 0;
}

int pf_load_segments(pf_handle* h, const pf_segments* sg) {
    HIPCHK(hipSetDevice(h->device));
    const long long S = sg->n;
    // what the .seg readers refuse, refused here too for callers that bring their own rows: an allele outside -1..2, and an unphased mark on
    // one sample only of a pair (2k, 2k + 1) -- the kernels' forms of the phasing test differ on such a row
    for (long long s = 0; s < S; ++s) {
        const int8_t* a = sg->alleles + (size_t)s * h->n;
        for (int i = 0; i < h->n; ++i)
            if (a[i] < -1 || a[i] > 2) { g_err = "Unknown character found in .seg file; expect one of '.', '/', '0' or '1'."; return -1; }
        for (int i = 0; i + 1 < h->n; i += 2)
            if ((a[i] == 2) != (a[i + 1] == 2)) { g_err = "Found inconsistent unphased heterozygous marks"; return -1; }
    }
    double *ds, *dl; int8_t *dst, *dal; int* dlim;
    int rc = 0;
    rc |= h->alloc(&ds, S); rc |= h->alloc(&dl, S); rc |= h->alloc(&dst, S);
    rc |= h->alloc(&dal, (size_t)S * h->n); rc |= h->alloc(&dlim, S);
    rc |= h->alloc(&h->A.tr_T, S); rc |= h->alloc(&h->A.tr_ess, S); rc |= h->alloc(&h->A.tr_logl, S);
    rc |= h->alloc(&h->A.tr_flag, S);
    if (rc) return -1;
    HIPCHK(hipMemcpyAsync(ds, sg->start, S * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dl, sg->length, S * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dst, sg->state, S, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dal, sg->alleles, (size_t)S * h->n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dlim, sg->max_record_epoch, S * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->A.seg_start = ds; h->A.seg_len = dl; h->A.seg_state = dst; h->A.seg_alleles = dal; h->A.seg_limit = dlim;
    h->h_seg_start.assign(sg->start, sg->start + S);
    h->h_seg_len.assign(sg->length, sg->length + S);
    h->n_segs = S;
    return 0;
}

int pf_load_lookahead(pf_handle* h, const pf_lookahead* la) {
    HIPCHK(hipSetDevice(h->device));
    if (la->level < 0 || la->level > 4) { g_err = "-apf must be in 0..4"; return -1; }
    if (la->n != h->n_segs) { g_err = "pf_load_lookahead: one look-ahead record per segment expected"; return -1; }
    if (la->level == 0) { h->A.apf = 0; h->la_flags = 0; return 0; }
    if (h->A.anc) { g_err = "pf_load_lookahead: -apf (the auxiliary particle filter) is not supported with sample times (-eI, ancient samples)"; return -1; }
    if (h->wide) { g_err = "-apf (the auxiliary particle filter) needs nsam <= 16"; return -1; }
    const long long S = la->n;
    const int n = h->n, D = la->max_doubletons, Q = la->n_quantiles;
    KArgs& A = h->A;
    double *fsd, *rmr, *ddist, *split, *q, *tbl; int8_t *unph, *didx, *sal; int *nd, *sk;
    int rc = 0;
    rc |= h->alloc(&fsd, (size_t)S * n); rc |= h->alloc(&rmr, (size_t)S * n); rc |= h->alloc(&unph, (size_t)S * n);
    rc |= h->alloc(&nd, S); rc |= h->alloc(&didx, (size_t)S * D * 4); rc |= h->alloc(&ddist, (size_t)S * D * 2);
    rc |= h->alloc(&split, S); rc |= h->alloc(&sal, (size_t)S * n); rc |= h->alloc(&sk, S);
    rc |= h->alloc(&q, Q); rc |= h->alloc(&tbl, (size_t)n * Q);
    if (!A.st0.lookahead) rc |= h->alloc(&A.st0.lookahead, (size_t)A.nslots * h->Np);
    if (rc) return -1;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(fsd, la->first_singleton_distance, (size_t)S * n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(rmr, la->relative_mutation_rate, (size_t)S * n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(unph, la->is_singleton_unphased, (size_t)S * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(nd, la->n_doubletons, (size_t)S * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(didx, la->doubleton_idx, (size_t)S * D * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ddist, la->doubleton_dist, (size_t)S * D * 2 * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(split, la->first_split_distance, (size_t)S * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(sal, la->split_alleles, (size_t)S * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(sk, la->split_count, (size_t)S * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(q, la->quantiles, (size_t)Q * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(tbl, la->tbl_lengths, (size_t)n * Q * 8, hipMemcpyHostToDevice));
    std::vector<double> ones((size_t)A.nslots * h->Np, 1.0);
    HIPCHK(hipMemcpy(A.st0.lookahead, ones.data(), ones.size() * 8, hipMemcpyHostToDevice));
    A.apf = la->level; A.la_D = D; A.la_Q = Q;
    A.la_fsd = fsd; A.la_rmr = rmr; A.la_unph = unph; A.la_nd = nd; A.la_didx = didx; A.la_ddist = ddist;
    A.la_split = split; A.la_salleles = sal; A.la_sk = sk; A.la_q = q; A.la_tbl = tbl;
    A.la_mean_tbl = la->mean_total_branch_length;
    h->la_flags = la->flags & (PF_LA_ROW_PIPELINE | PF_LA_ROW_PIPELINE_MP | PF_LA_ROW_PIPELINE_LDS);      // (with the load: a later one without the bits returns the handle to the general kernels)
    h->smem_la = smem_bytes_la(n, h->E);
    // 15 and 16 haplotypes: k_lookahead's scratch columns do not fit beside the tree; k_lookahead_xl keeps them inside the tree's own scratch
    h->la_xl = h->smem_la > 160 * 1024;
    if (h->la_xl) {
        h->smem_la = smem_bytes(n, h->E);
        if (h->smem_la > 64 * 1024) hipFuncSetAttribute((const void*)k_lookahead_xl, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem_la);
    } else if (h->smem_la > 64 * 1024) hipFuncSetAttribute((const void*)k_lookahead, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem_la);
    return 0;
}

