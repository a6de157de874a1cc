// smcsmc_amd/csrc/pf_create.h -- pf_create in four named steps: refuse, plan, allocate, prepare.  Included once, by pf_hip.hip, behind pf_handle.h.
#pragma once
#include <memory>

// ------------------------------------------------------------------ creation: refuse, plan, allocate, prepare
// Step 1.  Every refusal that needs no device, in the order in which they have always been made: pf_create's own, which a caller on a machine
// without a device still gets by name, then (behind the device count and index, create_impl) those of the model.
static int refuse_params(const pf_model* m, const pf_params* p) {
    auto fail = [&](const std::string& msg) { g_err = msg; return -1; };
    // switches of launch arrangements that were removed: a stale caller is told so, it does not silently get the default
    static const struct { int bit; const char* what; } removed[] = {
        {64, "one population as two launches on two streams"}, {512, "count workgroups in ascending epoch order"},
        {1024, "the two streams on disjoint compute units"}, {8192, "hand-off between launches through counters in memory"}};
    for (const auto& r : removed)
        if (p->debug & r.bit) return fail("pf_create: pf_params.debug bit " + std::to_string(r.bit) + " (" + r.what + ") selected a launch arrangement that has been removed");
    if (p->log_cap < 0 || p->gen_cap < 0 || p->piece_cap < 0 || p->log_cap > 0x7fffffffLL || p->piece_cap > 0x7fffffffLL)
        return fail("pf_create: ring capacities out of range");
    if ((p->gen_cap > 0 && p->gen_cap < 4) || (p->log_cap > 0 && p->log_cap < 4)) return fail("pf_create: log_cap and gen_cap must be at least 4");
    if (p->gen_cap > 0 && p->gen_cap < PF_RING + 4 && m->n_pops > 1)
        return fail("pf_create: gen_cap must be at least 20 when the extend role runs ahead of the counts (structured models)");
    return 0;
}
static int refuse_model(const pf_model* m, const pf_params* p) {
    auto fail = [&](const std::string& msg) { g_err = msg; return -1; };
    if (m->n_pops < 1 || m->n_pops > PF_POPS_TAKEN(m))
        return fail((m->flags & PF_MODEL_WIDE_POPS) ? "pf_create: n_pops must be in 1..8" : "pf_create: n_pops must be in 1..4");      // (five to eight: PF_MODEL_WIDE_POPS)
    if (m->nsam < 2 || m->nsam > PF_NMAX_WIDE) return fail("pf_create: nsam must be in 2..64");
    const bool wide = m->n_pops == 1 && (m->nsam > PF_NMAX || (p->debug & PF_DEBUG_FORCE_WIDE));
    if (m->nsam > PF_NMAX && m->n_pops > 1) return fail("pf_create: more than 16 haplotypes need one population (structured models take nsam <= 16)");
    if ((p->debug & PF_DEBUG_FORCE_WIDE) && m->n_pops > 1) return fail("pf_create: PF_DEBUG_FORCE_WIDE applies to one population only");
    if (wide && (p->flags & 2)) return fail("pf_create: tree recording (-arg) needs nsam <= 16 (its descendant masks are 32 bits wide)");
    if (m->n_epochs < 1 || m->n_epochs > PF_EMAX) return fail("pf_create: n_epochs must be in 1..64");
    if (m->n_pops > PF_PMAX && m->n_epochs > PF_EMAX_PWIDE)
        return fail("pf_create: a model of more than four populations takes at most 32 epochs (its migration events keep population and epoch in one byte, three bits and five)");
    if (p->np < 1 || p->np > 262144) return fail("pf_create: np must be in 1..262144");
    if (m->n_bias_heights < 0 || m->n_bias_heights > PF_BIAS_MAX) return fail("pf_create: at most 8 bias heights are supported");
    if (m->n_bias_heights > 0 && (!m->bias_heights || !m->bias_strengths || !m->application_delays))
        return fail("pf_create: bias_heights, bias_strengths and application_delays must all be given");
    if (m->n_rate_segments > 0) {
        if (!m->rate_positions || !m->rate_values || !m->leaf_rel_rates || !m->application_delays)
            return fail("pf_create: rate_positions, rate_values, leaf_rel_rates and application_delays must all be given with a guide");
        if (m->rate_positions[0] != 0.0) return fail("pf_create: the recombination guide must start at position 0");
        for (int k = 0; k < m->n_rate_segments; ++k) {
            if (k && !(m->rate_positions[k] > m->rate_positions[k - 1])) return fail("pf_create: guide segment starts must increase");
            if (!(m->rate_values[k] > 0)) return fail("pf_create: guide recombination rates must be positive");
            for (int i = 0; i < m->nsam; ++i)
                if (!(m->leaf_rel_rates[(size_t)k * m->nsam + i] > 0)) return fail("pf_create: relative leaf rates of the guide must be positive");
        }
    }
    if (p->mig_cap > 4096) return fail("pf_create: mig_cap out of range");
    // ancient samples (PF_MODEL_SAMPLE_TIMES): the times themselves, then what does not run with them
    {
        std::string why;
        if (sample_times_refusal(m, why, "pf_create")) return fail(why);
        if (model_sample_times(m)) {
            if (p->flags & 2) return fail("pf_create: tree recording (-arg) is not supported with sample times (-eI, ancient samples)");
            if (m->n_bias_heights > 0) return fail("pf_create: focused sampling (bias_heights) is not supported with sample times (-eI, ancient samples)");
            if (m->n_rate_segments > 0) return fail("pf_create: a recombination guide is not supported with sample times (-eI, ancient samples)");
        }
    }
    if (m->vb_coal_counts) {
        const size_t nc = (size_t)m->n_epochs * m->n_pops, nm = nc * m->n_pops;
        for (size_t i = 0; i < nc; ++i) if (!(m->vb_coal_counts[i] > 0)) return fail("pf_create: variational-Bayes event counts must be positive");
        for (size_t i = 0; i < nm && m->vb_mig_counts; ++i) if (!(m->vb_mig_counts[i] > 0)) return fail("pf_create: variational-Bayes event counts must be positive");
    }
    return 0;
}

static int create_refusals(const pf_model* m, const pf_params* p) { return refuse_params(m, p) || refuse_model(m, p) ? -1 : 0; }

// the ring capacities pf_create gives create_impl: the caller's, or the defaults
static void create_caps(const pf_model* m, const pf_params* p, long long* log_cap, long long* gen_cap) {
    // with -arg (flags bit 1) nothing may be overwritten: rings sized for a whole chunk by default
    const bool trees = p->flags & 2;
    // (more than 16 haplotypes: a record is 8 (n + 5) bytes, 552 at n = 64; the default ring then holds as many bytes per particle as
    // the 16 384 records of n = 16 do, rounded down to a power of two: 8192 records up to n = 35, 4096 up to n = 64)
    long long log_def = trees ? 131072 : 16384;
    if (!trees && m->nsam > PF_NMAX) {
        const long long fit = 16384LL * (5 + PF_NMAX - 1) / (5 + m->nsam);
        log_def = 1;
        while (log_def * 2 <= fit) log_def *= 2;
    }
    *log_cap = p->log_cap > 0 ? p->log_cap : log_def;
    *gen_cap = p->gen_cap > 0 ? p->gen_cap : (trees ? 131072 : 8192);
}

// Step 2.  What a handle is, decided here and nowhere else, from the model and the parameters alone (pf_test_plan shows it without a device).
struct CreatePlan {
    bool wide = false;
    int nblocks = 0, nc = 0;
    long long gen_cap = 0;        // as given, or clamped with -arg
    Rings rings = Rings::None;    // before the demotions of step 4
    int nslots = 2;               // copies of the particle state (KArgs::st0)
    bool draw_table = false;      // draw table of k_sweep (draw_role)
    size_t smem = 0, smem_pipe = 0;
    int ledger_wgs = 192, ncw = 0, workers = 0, split_batch = 0;
    std::vector<int> cw_off;
    int mcap = 0, dcap = 0;
    unsigned pcap = 0;
    int RS = 0, ncol = 0, max_trace_events = 0;
};
static CreatePlan create_plan(const pf_model* m, const pf_params* p, long long log_cap, long long gen_cap) {
    CreatePlan pl;
    const int E = m->n_epochs, n = m->nsam, P = m->n_pops;
    const long long Np = p->np;
    const bool wide = m->n_pops == 1 && (m->nsam > PF_NMAX || (p->debug & PF_DEBUG_FORCE_WIDE));
    pl.wide = wide;
    pl.nblocks = (int)((Np + PF_BS - 1) / PF_BS);
    pl.mcap = p->mig_cap > 0 ? p->mig_cap : PF_MMAX;
    const bool anc = model_sample_times(m) != nullptr;      // ancient samples (refuse_model: structured, no -arg): the ANC instances' LDS
    pl.smem = P > 1 ? (anc ? pf_mp_smem_bytes_anc(n, E, P, pl.mcap) : pf_mp_smem_bytes(n, E, P, pl.mcap)) : (wide ? pf_wide_smem_bytes(n, E) : smem_bytes(n, E));
    pl.max_trace_events = std::max(0, p->max_trace_events);
    if (p->flags & 2) {
        // -arg: the parent table of every resampling is kept (it is the ancestry the tree dump walks back through).
        // Structured models record trees on either row kernel: the register tree (nsam <= 8) or the LDS tree (any nsam
        // they take, i.e. up to 16 -- the width of the descendant sets in a record -- and PF_DEBUG_FORCE_LDS).
        if (gen_cap > 0x7fffffffLL / 2) gen_cap = 0x7fffffffLL / 2;
        pl.max_trace_events = (int)gen_cap;
    }
    pl.gen_cap = gen_cap;
    pl.split_batch = (p->debug >> 16) & 15;       // (bits 16-19 of debug: tuning experiments; 0 = four)
    // What this handle is allocated for: the rings of a row pipeline (sixteen copies of the state, the second run-list copy, the decision
    // rings, the count columns' table, smem_pipe) and the draw table.
    const size_t nc = (size_t)((Np + 63) / 64);
    pl.nc = (int)nc;
    const bool fits = Np <= 131072 && !wide;      // beyond that the decision tables outgrow the default dynamic LDS
    const bool plain = !(p->flags & 2) && !(p->debug & (PF_DEBUG_FORCE_LDS | PF_DEBUG_NO_FUSE | PF_DEBUG_K_PIPE));     // no -arg, no switch to another path
    if (P == 1 && n <= 8 && fits) pl.rings = Rings::Reg;      // (with a switch or a look-ahead that takes the rows elsewhere the rings are there, unused)
    // structured models with the tree in registers: the same pipeline, the extend role as its own launch (run_sweep_x)
    // (more than PF_PMAX populations: no rings -- the general path on the LDS-tree kernels at every number of haplotypes, the wide walk of pf_mp.h)
    // (sample times: the same -- no rings, the general path on the ANC instances of the LDS-tree kernels at every number of haplotypes)
    else if (P > PF_PMAX || anc) pl.rings = Rings::None;
    else if (P > 1 && n <= 8 && fits && plain) pl.rings = Rings::Xmp;
    // one population on the LDS tree, several chunks in lockstep (pf_run_many): the same rings, the extend role k_sweep_xl.  Not with a
    // generation ring too short for an extend role that runs ahead of the counts (what pf_create refuses for structured models; here the
    // general kernels serve such a handle as before)
    else if (P == 1 && n > 8 && n <= PF_NMAX && fits && plain && gen_cap >= PF_RING + 4 && !(p->debug & PF_DEBUG_TWO_LAUNCH) && lds_pipe_tables_fit(n, (int)nc))
        pl.rings = Rings::Xl;
    // structured models on the LDS tree, only where the caller asked (PF_FLAG_MP_LDS_ROWS): the same rings, the extend role k_sweep_xlmp with 64
    // particles a workgroup.  The decision's tables go into the lanes' migration-time column or behind the state: 0 says that they fit in neither
    else if ((p->flags & PF_FLAG_MP_LDS_ROWS) && P > 1 && n > 8 && n <= PF_NMAX && fits && plain && gen_cap >= PF_RING + 4 && !(p->debug & PF_DEBUG_TWO_LAUNCH) &&
             pf_mp_sweep_xl_smem_bytes(n, E, P, pl.mcap, (int)nc) > 0)
        pl.rings = Rings::Xlmp;
    const bool has_rings = pl.rings != Rings::None;
    pl.nslots = has_rings ? PF_RING : 2;
    pl.draw_table = pl.rings == Rings::Reg && !(p->debug & (PF_DEBUG_K_PIPE | PF_DEBUG_NO_DRAW_TABLE));
    if (has_rings) pl.smem_pipe = ((size_t)(2 * PF_EPAD + E + 2 * PF_BIAS_MAX + 3) + pipe_lds_doubles((int)nc)) * 8;
    // (several chunks per GPU -- the caller set count_wgs -- : on the rows that do not resample, nine in ten, these workgroups find nothing to do and
    // leave after 2 us of a slot each; with 32 instead of 192 eight chunks gain 3 %, one chunk is the same either way: 28.7 us per row)
    pl.ledger_wgs = p->count_wgs > 0 ? 32 : std::max(16, std::min(PF_LEDGER_BLOCKS, 192));
    {
        const int PT = pf_count_pops(P);         // k_count is instantiated for 1, 2, PF_PMAX and PF_PWIDE populations
        pl.ncol = PT == 1 ? 6 : 3 * PT + 3 + PT * PT + 2 * PT;
    }
    pl.dcap = p->delay_cap > 0 ? p->delay_cap : PF_DCAP_DEFAULT;
    pl.RS = 5 + (n - 1) + (wide ? 1 : 0);          // the wide kernels' records: the cut branch's samples in a 64-bit word behind the heights
    // a genealogy update leaves one piece per (epoch, population) stretch of its path: a handful per record
    if (P > 1) pl.pcap = (unsigned)(p->piece_cap > 0 ? p->piece_cap : 4 * log_cap);
    // accumulators of the count workgroups per epoch (measured: four times as many count workgroups per epoch in the row
    // pipeline made a row 15 % slower -- the launch then holds 5 000 workgroups of 30 KB LDS each, four rounds of the chip)
    // the row pipeline spreads an epoch's count tasks (the ancestor runs of the generations in its window: for the old epochs,
    // whose lag is a few rows, nearly one per particle) over this many workgroups; fewer is slower (C3 shape, one chunk: 40
    // workgroups 32.9 us per row, 16: 38.7, 8: 53.7, 4: 91.4, 2: 168 -- profiles/round3/count_wgs.md)
    pl.ncw = p->count_wgs > 0 ? std::min<int>(p->count_wgs, pl.nblocks) : pl.nblocks;
    // (the queue has one kernel instance so far: one population, at most four haplotypes, no focused sampling, no -arg, single launch per step)
    pl.workers = (pl.rings == Rings::Reg && !(p->debug & PF_DEBUG_K_PIPE) && n <= 4 && !(m->n_bias_heights > 0 || m->n_rate_segments > 0) && !(p->flags & 2)) ? std::max(0, std::min(p->count_workers, 4096)) : 0;
    // count workgroups per epoch column of the row pipeline: the tasks of an epoch are the live ancestors of the generations in its
    // window, about Np / (1 + depth), depth = generations between window and front, i.e. in proportion to its lag: a column whose
    // lag is a few rows long gets all ncw workgroups, the young epochs' columns, whose workgroups mostly found nothing to do
    // and left after their prologue, as few as two.  (What a workgroup finds it strides over: any number is correct.)
    pl.cw_off.assign(E + 1, 0);
    for (int j = 0; j < E; ++j) {
        const double lag = m->lags[E - 1 - j];
        int w = (int)std::ceil((double)pl.ncw * std::min(1.0, 2500.0 / std::max(lag, 1.0)));
        // (a higher minimum -- 4, 8, 12, 15 -- changes nothing: the long count workgroups of a step are not those of narrow columns)
        w = std::max(std::min(2, pl.ncw), std::min(w, pl.ncw));
        // (only when the caller set count_wgs, i.e. runs several chunks side by side and wants fewer workgroups: a single chunk
        // leaves most of the chip idle, and there every column is shortest with all the workgroups it can get)
        if (p->count_wgs <= 0) w = pl.ncw;
        pl.cw_off[j + 1] = pl.cw_off[j] + w;
    }
    return pl;
}

// Steps 3 and 4 on a handle whose streams and events exist; whatever fails, the caller lets go of the handle, which frees what there is.
static int create_allocate(pf_handle* h, const pf_model* m, const pf_params* p, const CreatePlan& pl, long long log_cap);
static int create_prepare(pf_handle* h, const pf_params* p);

static pf_handle* create_impl(const pf_model* m, const pf_params* p, int device, long long log_cap, long long gen_cap) {
    auto fail = [&](const std::string& msg) -> pf_handle* { g_err = msg; return nullptr; };
    int ndev = pf_device_count();
    if (ndev <= 0) return fail("pf_create: no HIP device available (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail("pf_create: device index out of range");
    if (refuse_model(m, p)) return nullptr;
    const CreatePlan pl = create_plan(m, p, log_cap, gen_cap);
    // every failure from here on leaves through ~pf_handle
    std::unique_ptr<pf_handle> h(new pf_handle());
    h->device = device;
    if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed");
    // (no stream priorities: a high-priority filter stream per handle gains nothing for one chunk and costs 30 % of the
    // throughput when several chunks share the device -- priority streams share fewer hardware queues)
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
    if (hipStreamCreateWithFlags(&h->cstream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
    h->sync_ev.resize(512);
    for (auto& e : h->sync_ev) if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) return fail("hipEventCreate failed");
    if (create_allocate(h.get(), m, p, pl, log_cap) || create_prepare(h.get(), p)) return nullptr;
    return h.release();
}

// Step 3.  The handle's fields and arrays from the plan: one allocation per array.
static int create_allocate(pf_handle* h, const pf_model* m, const pf_params* p, const CreatePlan& pl, long long log_cap) {
    const int E = m->n_epochs, n = m->nsam, P = m->n_pops;
    const long long Np = p->np;
    const bool wide = pl.wide, has_rings = pl.rings != Rings::None;
    const size_t nc = (size_t)pl.nc;
    h->E = E; h->n = n; h->Np = Np; h->P = P;
    h->wide = wide;
    h->nblocks = pl.nblocks;
    h->smem = pl.smem;
    h->max_trace_events = pl.max_trace_events;
    h->debug = p->debug;
    h->no_count = (p->debug & PF_DEBUG_NO_COUNT) != 0;
    h->no_spec_stage = (p->debug & PF_DEBUG_NO_SPEC_STAGE) != 0;
    h->split_batch = pl.split_batch;
    h->rings = pl.rings;
    h->smem_pipe = pl.smem_pipe;
    h->ledger_wgs = pl.ledger_wgs;
    h->ncw = pl.ncw;
    h->workers = pl.workers;
    h->cw_off = pl.cw_off;
    h->h_lags.assign(m->lags, m->lags + E);
    h->h_counted_to.assign(E, 0.0);
    h->h_L = m->loci_length;
    KArgs& A = h->A;
    memset(&A, 0, sizeof(A));
    A.E = E; A.n = n; A.flags = m->flags | (h->no_spec_stage ? 256 : 0);
    A.flags |= p->debug & (7 << 20);        // profiling probes of the count role (bits 20, 21: the sums are then wrong on purpose)
    A.L = m->loci_length; A.mu = m->mutation_rate; A.rho = m->recombination_rate;
    A.Np = Np;
    A.mcap = pl.mcap;
    A.ess_threshold = (double)Np * p->ess_fraction;
    A.seed = p->seed;
    A.P = P;
    A.ncol = pl.ncol;
    int rc = 0;
    std::vector<double> Hc;
    if (h->mem.upload(&A.lags, m->lags, E, h->stream) || upload_model_tables(m, A, h->mem, h->stream, true, &Hc)) return -1;
    if (m->vb_coal_counts) {
        const size_t nc = (size_t)E * P, nm = (size_t)E * P * P;
        const double* cin; double *cout_, *mout;
        std::vector<double> cnt(nc + nm, 1e10);
        for (size_t i = 0; i < nc; ++i) cnt[i] = m->vb_coal_counts[i];
        if (m->vb_mig_counts) for (size_t i = 0; i < nm; ++i) cnt[nc + i] = m->vb_mig_counts[i];
        const int vrc = h->mem.upload(&cin, cnt.data(), nc + nm, h->stream) || h->alloc(&cout_, nc) || h->alloc(&mout, nm);
        if (!vrc) {
            hipLaunchKernelGGL(k_vb_table, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, h->stream, cin, (long long)nc, cout_);
            hipLaunchKernelGGL(k_vb_table, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, h->stream, cin + nc, (long long)nm, mout);
        }
        const hipError_t synchronised = hipStreamSynchronize(h->stream);      // (cnt is read until here)
        if (vrc) return -1;
        HIPCHK(synchronised);
        A.vb_coal = cout_; A.vb_mig = mout;
    }
    A.lut = nullptr; A.lut_kbT = 0; A.lut_kbH = 0;
    unsigned char lut[2 * PF_LUT_N];
    if (!(p->debug & PF_DEBUG_NO_SEARCH_LUT) && lut_build(m->change_times, E, lut, &A.lut_kbT) && lut_build(Hc.data(), E, lut + PF_LUT_N, &A.lut_kbH))
        rc |= h->mem.upload(&A.lut, lut, sizeof(lut), h->stream);
    A.n_bias = m->n_bias_heights;
    A.delay_type = m->delay_type;
    A.dcap = pl.dcap;
    A.delay_evict = (p->flags & 4) ? 1 : 0;
    for (int k = 0; k < PF_BIAS_MAX + 2; ++k) A.bias_H[k] = HUGE_VAL;
    for (int k = 0; k < PF_BIAS_MAX + 1; ++k) A.bias_S[k] = 1.0;
    A.bias_H[0] = 0.0;
    if (A.n_bias > 0 || m->n_rate_segments > 0) {
        for (int k = 0; k < A.n_bias; ++k) A.bias_H[k + 1] = m->bias_heights[k];
        for (int k = 0; k <= A.n_bias && A.n_bias > 0; ++k) A.bias_S[k] = m->bias_strengths[k];
        rc |= h->mem.upload(&A.app_delays, m->application_delays, E, h->stream);
    }
    // one entry of rg_blkcnt per wavefront where the extend workgroups own fewer than 256 particles: the structured models (64, on either tree), and the handles
    // RunPath::SweepSplit takes (split_shape, pf_handle.h), whose paired form owns 128 -- whichever form of the row kernel then runs
    const bool split = split_shape(h->rings == Rings::Reg, m->n_pops, n, m->n_bias_heights > 0 || m->n_rate_segments > 0, (p->flags & 2) != 0, p->debug);
    A.blk_gran = (h->rings == Rings::Xmp || h->rings == Rings::Xlmp || split) ? 4 : 1;
    {
        const size_t K = (size_t)pl.nslots;
        A.nslots = pl.nslots;
        DState& st = A.st0;
        rc |= h->alloc(&st.S, K * (size_t)(n - 1) * Np);
        rc |= h->alloc(&st.C, K * (size_t)2 * (n - 1) * Np);
        rc |= h->alloc(&st.w_post, K * Np);
        rc |= h->alloc(&st.w_pilot, K * Np);
        rc |= h->alloc(&st.next_base, K * Np);
        rc |= h->alloc(&st.x_mark, K * Np);
        rc |= h->alloc(&st.Ltree, K * Np);
        rc |= h->alloc(&st.mark_limit, K * Np);
        if (P > 1) {
            rc |= h->alloc(&st.Pn, K * (size_t)(n - 1) * Np);
            rc |= h->alloc(&st.nm, K * Np);
            rc |= h->alloc(&st.Mt, K * (size_t)A.mcap * Np);
            rc |= h->alloc(&st.Mb, K * (size_t)A.mcap * Np);
            rc |= h->alloc(&st.Mq, K * (size_t)A.mcap * Np);
        }
        if (m->n_rate_segments > 0) rc |= h->alloc(&st.ridx, K * Np);
        if (m->n_bias_heights > 0 || m->n_rate_segments > 0) {
            rc |= h->alloc(&st.total_delayed, K * Np);
            rc |= h->alloc(&st.dcount, K * Np);
            rc |= h->alloc(&st.dpos, K * (size_t)A.dcap * Np);
            rc |= h->alloc(&st.dfac, K * (size_t)A.dcap * Np);
            rc |= h->alloc(&st.ddelta, K * (size_t)A.dcap * Np);
            rc |= h->alloc(&st.dk, K * (size_t)A.dcap * Np);
        }
    }
    if (p->flags & 1) {
        // 100-bp local recombination map (count.hpp:101-102, 115)
        A.lmap_bins = (long long)(m->loci_length / 100.0) + 4;
        rc |= h->alloc(&A.lmap_opp, (size_t)A.lmap_bins);
        rc |= h->alloc(&A.lmap_cnt, (size_t)(n + 2) * A.lmap_bins);
    }
    if (m->n_rate_segments > 0) {
        // RecombinationBias::set_model_rates (pfparam.hpp:199-211): the segments that start inside the locus
        int K = 0;
        while (K < m->n_rate_segments && m->rate_positions[K] < m->loci_length) ++K;
        rc |= h->mem.upload(&A.g_pos, m->rate_positions, K, h->stream);
        rc |= h->mem.upload(&A.g_rho, m->rate_values, K, h->stream);
        rc |= h->mem.upload(&A.g_leaf, m->leaf_rel_rates, (size_t)K * n, h->stream);
        A.g_K = K;
    }
    rc |= h->alloc(&A.rng_ctr, Np);
    A.dt_tab = nullptr; A.dt_filled = nullptr; A.dt_ctr = nullptr;
    if (pl.draw_table) {
        // 512 bytes per slot
        rc |= h->alloc(&A.dt_tab, (size_t)2 * PF_DRAW_RING * Np);
        rc |= h->alloc(&A.dt_filled, (size_t)2 * Np);
        rc |= h->alloc(&A.dt_ctr, (size_t)2 * Np);
    }
    rc |= h->alloc(&A.ebuf, Np);
    rc |= h->alloc(&A.widx, Np);
    A.cap = (unsigned)log_cap;
    A.rec_trees = (p->flags & 2) ? 1 : 0;
    A.RS = pl.RS;
    A.Gcap = (int)pl.gen_cap;
    rc |= h->alloc(&A.log, (size_t)Np * A.cap * A.RS);
    if (P > 1) {
        A.pcap = pl.pcap;
        rc |= h->alloc(&A.plog, (size_t)Np * A.pcap * 3);
        rc |= h->alloc(&A.pidx, Np);
    }
    rc |= h->alloc(&A.gstart, (size_t)A.Gcap * Np);
    rc |= h->alloc(&A.lo, (size_t)A.Gcap * (Np + 1));
    rc |= h->alloc(&A.gen_x0, A.Gcap);
    rc |= h->alloc(&A.parent, Np);
    rc |= h->alloc(&A.blkcnt2[0], (size_t)h->nblocks); rc |= h->alloc(&A.blkcnt2[1], (size_t)h->nblocks);
    rc |= h->alloc(&A.run_st, (size_t)A.Gcap * Np);
    rc |= h->alloc(&A.run_anc, (size_t)A.Gcap * Np);
    rc |= h->alloc(&A.nruns, A.Gcap);
    A.nc = (int)nc;
    if (has_rings) {
        rc |= h->alloc(&A.run_st2, (size_t)A.Gcap * Np);
        rc |= h->alloc(&A.run_anc2, (size_t)A.Gcap * Np);
        rc |= h->alloc(&A.nruns2, A.Gcap);
        rc |= h->alloc(&A.rg_scan1, PF_RING * (size_t)Np); rc |= h->alloc(&A.rg_scan1m, PF_RING * (size_t)Np);
        rc |= h->alloc(&A.rg_scanp, PF_RING * (size_t)Np); rc |= h->alloc(&A.rg_widx, PF_RING * (size_t)Np);
        rc |= h->alloc(&A.rg_cpost, PF_RING * nc); rc |= h->alloc(&A.rg_csq, PF_RING * nc); rc |= h->alloc(&A.rg_cpil, PF_RING * nc);
        rc |= h->alloc(&A.rg_cpp, PF_RING * nc); rc |= h->alloc(&A.rg_cmx1, PF_RING * nc); rc |= h->alloc(&A.rg_coffp, PF_RING * nc);
        rc |= h->alloc(&A.rg_dpend, PF_RING * nc); rc |= h->alloc(&A.rg_blkcnt, PF_RING * (size_t)h->nblocks * 4);
    }
    rc |= h->alloc(&A.chunk_post, nc); rc |= h->alloc(&A.chunk_sq, nc); rc |= h->alloc(&A.chunk_pil, nc);
    rc |= h->alloc(&A.scan1, Np); rc |= h->alloc(&A.chunk_off, nc); rc |= h->alloc(&A.l2scan, nc);
    rc |= h->alloc(&A.scan1m, Np); rc |= h->alloc(&A.chunk_mx1, nc);
    rc |= h->alloc(&A.chunk_dpend, nc);
    rc |= h->alloc(&A.chunk_pp, nc); rc |= h->alloc(&A.l2scanp, nc);
    for (int b = 0; b < 2; ++b) {
        rc |= h->alloc(&A.scanp2[b], Np); rc |= h->alloc(&A.chunk_offp2[b], nc);
        rc |= h->alloc(&A.snap_w[b], Np); rc |= h->alloc(&A.snap_S[b], (size_t)(n - 1) * Np);
        rc |= h->alloc(&A.snap_xm[b], Np); rc |= h->alloc(&A.snap_ml[b], Np); rc |= h->alloc(&A.snap_widx[b], Np);
    }
    // per-epoch accumulators: one per count workgroup of a column (count_body)
    A.nbx = h->nblocks;
    if (has_rings) {
        const int* dcw = nullptr;
        rc |= h->mem.upload(&dcw, h->cw_off.data(), (size_t)(E + 1), h->stream);
        // (with every column at full width the kernels compute column and workgroup from the index: no table)
        A.cw_off = p->count_wgs <= 0 ? nullptr : dcw;
    }
    rc |= h->alloc(&A.totals, (size_t)A.ncol * E);
    rc |= h->alloc(&A.partial, (size_t)E * A.nbx * A.ncol);
    A.max_trace_events = h->max_trace_events;
    rc |= h->alloc(&A.ev_seg, (size_t)std::max(1, h->max_trace_events));
    rc |= h->alloc(&A.ev_parents, (size_t)std::max(1, h->max_trace_events) * Np);
    rc |= h->alloc(&A.ctrl, 1);
    // the uploads above (search table, delays, guide, count columns) read the caller's arrays and this function's: done with them before it
    // returns, also after a failure
    const hipError_t synchronised = hipStreamSynchronize(h->stream);
    if (rc) return -1;
    HIPCHK(synchronised);
    return 0;
}

// Step 4.  The kernels' LDS limits for this handle, and the two demotions of a row pipeline the device then refuses.
static int create_prepare(pf_handle* h, const pf_params* p) {
    auto fail = [&](const std::string& msg) { g_err = msg; return -1; };
    const int E = h->E, n = h->n, P = h->P;
    const bool wide = h->wide;
    KArgs& A = h->A;
    if (wide && pf_wide_prepare(h->smem)) return fail("pf_create: the local-tree state does not fit the LDS of one workgroup");
    if (P == 1 && !wide && h->smem > 64 * 1024) {
        hipFuncSetAttribute((const void*)k_extend, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem);
        hipFuncSetAttribute((const void*)k_init, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem);
    }
    // structured models: the LDS-tree kernels serve the prior tree and calibration for every n, the row kernel is the
    // register-tree one for n <= 8
    // (and the only one beyond PF_PMAX populations, where they are the row kernel at every n)
    const bool lds_rows = P > 1 && (n > 8 || P > PF_PMAX || A.anc || (p->debug & PF_DEBUG_FORCE_LDS));
    if (h->smem > 160 * 1024 || (P > 1 && pf_mp_prepare(h->smem, A.mcap)) ||
        (P > 1 && !lds_rows && pf_mp_reg_smem_bytes(E, P, A.mcap) > 160 * 1024))
        return fail(P > 1 ? "pf_create: the local-tree state (tree, epoch tables and pf_params.mig_cap migration events per lane) does not fit the LDS of one workgroup"
                          : "pf_create: the local-tree state does not fit the LDS of one workgroup");
    // a row pipeline the device then refuses: the rings stay, the general kernels take the rows (and pf_run_many refuses)
    auto demote = [&] { h->rings = Rings::None; };
    if (h->rings == Rings::Xmp) {
        h->smem_sweep_x = pf_mp_sweep_smem_bytes(E, P, A.mcap, A.nc);
        if (pf_mp_sweep_prepare(h->smem_sweep_x)) demote();                  // the event lists and the decision tables do not fit together: the two-stream path
    }
    if (h->rings == Rings::Xl) {
        // k_sweep_xl: the LDS of k_extend (the decision tables lie in the tree columns)
        h->smem_sweep_x = h->smem;
        // (the attribute belongs to the kernel, not to the handle: the largest any handle of the process has asked for, so that a
        // handle of twelve haplotypes made after one of sixteen does not lower it)
        static std::atomic<int> xl_smem{0};
        int most = xl_smem.load();
        while (most < (int)h->smem && !xl_smem.compare_exchange_weak(most, (int)h->smem)) {}
        most = std::max(most, (int)h->smem);
        if (most > 64 * 1024 &&
            (hipFuncSetAttribute((const void*)k_sweep_xl<false>, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess ||
             hipFuncSetAttribute((const void*)k_sweep_xl<true>, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess ||
             hipFuncSetAttribute((const void*)k_sweep_xl<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess)) {
            (void)hipGetLastError();
            demote();
        }
    }
    if (h->rings == Rings::Xlmp) {
        // k_sweep_xlmp: the LDS of k_extend_mp, and the decision's tables behind it where the migration-time column is too short for them
        h->smem_sweep_x = pf_mp_sweep_xl_smem_bytes(n, E, P, A.mcap, A.nc);
        if (pf_mp_sweep_xl_prepare(h->smem_sweep_x)) demote();
    }
    return 0;
}

pf_handle* pf_create(const pf_model* m, const pf_params* p, int device) {
    if (!m || !p) { g_err = "pf_create: null model or parameters"; return nullptr; }
    if (refuse_params(m, p)) return nullptr;
    long long log_cap, gen_cap;
    create_caps(m, p, &log_cap, &gen_cap);
    return create_impl(m, p, device, log_cap, gen_cap);
}

void pf_destroy(pf_handle* h) { delete h; }

// Steps 1 and 2 without a device: the refusal, or the plan as integers -- rings (0 none, 1 Reg, 2 Xmp, 3 Xl, 4 Xlmp), nslots, draw_table, smem,
// smem_pipe, ledger_wgs, ncw, workers, split_batch, mcap, dcap, pcap, RS, ncol, max_trace_events, E, cw_off[0..E]
int pf_test_plan(const pf_model* m, const pf_params* p, int32_t* out, int32_t n_out) {
    if (!m || !p) { g_err = "pf_create: null model or parameters"; return -1; }
    if (create_refusals(m, p)) return -1;
    long long log_cap, gen_cap;
    create_caps(m, p, &log_cap, &gen_cap);
    const CreatePlan pl = create_plan(m, p, log_cap, gen_cap);
    const int32_t head[] = {(int32_t)pl.rings, pl.nslots, pl.draw_table, (int32_t)pl.smem, (int32_t)pl.smem_pipe, pl.ledger_wgs, pl.ncw, pl.workers,
                            pl.split_batch, pl.mcap, pl.dcap, (int32_t)pl.pcap, pl.RS, pl.ncol, pl.max_trace_events, m->n_epochs};
    const int nh = (int)(sizeof(head) / sizeof(head[0])), nv = nh + m->n_epochs + 1;
    if (!out || n_out < nv) { g_err = "pf_test_plan: room for " + std::to_string(nv) + " values needed"; return -1; }
    std::copy(head, head + nh, out);
    std::copy(pl.cw_off.begin(), pl.cw_off.end(), out + nh);
    return nv;
}
