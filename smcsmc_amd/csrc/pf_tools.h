// smcsmc_amd/csrc/pf_tools.h -- the entry points without a handle: unit tests, the look-ahead table, lag calibration, the simulators.
// Included once, by pf_hip.hip, behind pf_get.h.
#pragma once

// ------------------------------------------------------------------ unit-level test entry points
static int test_setup(int device) {
    if (pf_device_count() <= 0) { g_err = "no HIP device"; return -1; }
    HIPCHK(hipSetDevice(device));
    return 0;
}

int pf_test_math(const double* x, int64_t n, double* oe, double* ol, double* of, int device) {
    if (test_setup(device)) return -1;
    DevMem mem;
    const double* dx; double *de, *dl, *df;
    if (mem.upload(&dx, x, (size_t)n, 0) || mem.reserve(&de, (size_t)n) || mem.reserve(&dl, (size_t)n) || mem.reserve(&df, (size_t)n)) return -1;
    hipLaunchKernelGGL(k_test_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, (long long)n, de, dl, df);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(oe, de, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ol, dl, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(of, df, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

int pf_test_div(const double* a, const double* b, int64_t n, double* out, int device) {
    if (test_setup(device)) return -1;
    DevMem mem;
    const double *da, *db; double* dout;
    if (mem.upload(&da, a, (size_t)n, 0) || mem.upload(&db, b, (size_t)n, 0) || mem.reserve(&dout, (size_t)n)) return -1;
    hipLaunchKernelGGL(k_test_div, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, da, db, (long long)n, dout);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

int pf_test_uniform(uint64_t seed, uint32_t slot, uint32_t stream, uint64_t first_draw, int64_t n, double* out, int device) {
    if (test_setup(device)) return -1;
    DevMem mem;
    double* d;
    if (mem.reserve(&d, (size_t)n)) return -1;
    hipLaunchKernelGGL(k_test_uniform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (unsigned long long)seed, slot, stream,
                       (unsigned long long)first_draw, (long long)n, d);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

// canonical sum / scan / systematic table through the production kernels (k_partials + k_decide)
static int test_reduce_impl(const double* x, int64_t n, double* out_sum, double* out_scan, double u, int32_t* lo, int device) {
    if (test_setup(device)) return -1;
    pf_model m;
    memset(&m, 0, sizeof(m));
    double ct = 0.0, ps = 1e4, lag = 1e30;
    int rf = 3;
    m.n_epochs = 1; m.n_pops = 1; m.nsam = 2; m.loci_length = 1e6; m.mutation_rate = 1e-8; m.recombination_rate = 1e-8;
    m.change_times = &ct; m.pop_sizes = &ps; m.record_flags = &rf; m.lags = &lag;
    pf_params p;
    memset(&p, 0, sizeof(p));
    p.np = n; p.ess_fraction = lo ? 2.0 : 0.0; p.seed = 1; p.max_trace_events = 0;   // ESS < 2N always -> forces the table
    pf_handle* h = create_impl(&m, &p, device, 8, 4);
    if (!h) return -1;
    int rc = 0;
    double s0 = 0.0, l0 = 1.0; int8_t st0 = 1; int8_t al[2] = {-1, -1}; int lim0 = 0;
    pf_segments sg = {1, &s0, &l0, &st0, al, &lim0};
    rc |= pf_load_segments(h, &sg);
    rc |= pf_init_prior(h, 0.0);
    if (!rc) {
        hipMemcpyAsync(h->A.st0.w_post, x, n * 8, hipMemcpyHostToDevice, h->stream);
        hipMemcpyAsync(h->A.st0.w_pilot, x, n * 8, hipMemcpyHostToDevice, h->stream);
        hipLaunchKernelGGL(k_partials, dim3(h->nblocks), dim3(PF_BS), 0, h->stream, h->A);
        // override u by running k_decide in mode 0 and then patching: simpler -- write u after the fact
        hipLaunchKernelGGL(k_decide, dim3(h->nblocks + 1), dim3(PF_BS), 0, h->stream, h->A, (long long)0, lo ? 0 : 1, no_windows(h), h->nblocks);
        hipStreamSynchronize(h->stream);
        Ctrl c;
        rc |= read_ctrl(h, c);
        if (out_sum) *out_sum = c.T;
        if (out_scan) {
            std::vector<double> s1(n), off((n + 63) / 64);
            hipMemcpy(s1.data(), h->A.scan1, n * 8, hipMemcpyDeviceToHost);
            hipMemcpy(off.data(), h->A.chunk_off, off.size() * 8, hipMemcpyDeviceToHost);
            for (int64_t i = 0; i < n; ++i) out_scan[i] = off[i >> 6] + s1[i];
        }
        if (lo) {
            (void)u;
            hipMemcpy(lo, h->A.lo, (n + 1) * 4, hipMemcpyDeviceToHost);
        }
    }
    pf_destroy(h);
    return rc ? -1 : 0;
}

int pf_test_reduce(const double* x, int64_t n, double* out_sum, double* out_incl_scan, int device) {
    return test_reduce_impl(x, n, out_sum, out_incl_scan, 0.0, nullptr, device);
}

int pf_test_systematic(const double* pilot, int64_t n, double u, int32_t* lo, int device) {
    // the production kernel draws u from the resampler stream (seed 1, event 0); the caller
    // obtains the same u through pf_test_uniform(1, 0xFFFFFFFF, 1, 0, ...)
    return test_reduce_impl(pilot, n, nullptr, nullptr, u, lo, device);
}

// bytes of device memory the owners of this process hold now (DevMem, pf_devmem.h): 0 when no handle is open and no call is running
int64_t pf_test_live_bytes(void) { return (int64_t)g_live_bytes.load(); }

int pf_test_search_lut(const double* tab, int32_t n, uint8_t* lut, int32_t* kbase) {
    int kb = 0;
    if (n < 1 || n > PF_EMAX || !lut_build(tab, n, lut, &kb)) return 0;
    *kbase = kb;
    return 1;
}

int pf_terminal_branch_quantiles(const pf_model* m, uint64_t seed, int64_t n_trees, const double* quantiles, int32_t nq,
                                 double* lengths_out, double* mean_total_out, int device) {
    if (model_sample_times(m)) { g_err = "pf_terminal_branch_quantiles: not supported with sample times (-eI, ancient samples)"; return -1; }
    if (test_setup(device)) return -1;
    if (m->n_pops < 1 || m->n_pops > PF_POPS_TAKEN(m) || m->nsam < 2 || m->nsam > PF_NMAX || m->n_epochs < 1 || m->n_epochs > PF_EMAX ||
        (m->n_pops > PF_PMAX && m->n_epochs > PF_EMAX_PWIDE) || n_trees < 1) {
        g_err = "pf_terminal_branch_quantiles: unsupported model (1..4 populations, 1..8 with PF_MODEL_WIDE_POPS; 2..16 haplotypes, 1..64 epochs, at most 32 with more than four populations)";
        return -1;
    }
    const int E = m->n_epochs, n = m->nsam, P = m->n_pops;
    KArgs A;
    memset(&A, 0, sizeof(A));
    A.E = E; A.n = n; A.P = P; A.L = m->loci_length; A.mu = m->mutation_rate; A.rho = m->recombination_rate; A.mcap = PF_MMAX;
    DevMem mem;
    double *dh, *dl; int* derr;
    if (upload_model_tables(m, A, mem, 0) || mem.alloc(&derr, 1, 0) || mem.reserve(&dh, (size_t)n * n_trees) || mem.reserve(&dl, (size_t)n_trees)) return -1;
    int tbl_err = 0;
    if (P > 1) {
        const size_t smem = pf_mp_smem_bytes(n, E, P, PF_MMAX);
        if (pf_mp_prepare(smem, PF_MMAX)) { g_err = "pf_terminal_branch_quantiles: the local-tree state does not fit the LDS"; return -1; }
        pf_mp_launch_tbl(A, (unsigned long long)seed, (long long)n_trees, dh, dl, derr, smem, 0);
    } else {
        const size_t smem = smem_bytes(n, E);
        if (smem > 64 * 1024) hipFuncSetAttribute((const void*)k_tbl, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        hipLaunchKernelGGL(k_tbl, dim3((unsigned)((n_trees + PF_BS - 1) / PF_BS)), dim3(PF_BS), smem, 0, A, (unsigned long long)seed,
                           (long long)0, (long long)n_trees, dh, dl);
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(&tbl_err, derr, 4, hipMemcpyDeviceToHost));
    std::vector<double> hh, ll;
    if (download(hh, dh, (size_t)n * n_trees) || download(ll, dl, (size_t)n_trees)) return -1;
    mem.clear();
    if (tbl_err) {
        g_err = tbl_err == 1 ? "too many migration events on one local tree" : "No final coalescence event was sampled!";
        return -1;
    }
    for (int i = 0; i < n; ++i) {
        double* row = hh.data() + (size_t)i * n_trees;
        std::sort(row, row + n_trees);
        for (int q = 0; q < nq; ++q) lengths_out[i * nq + q] = row[(long long)(quantiles[q] * (double)n_trees)];
    }
    double total = 0.0;
    for (long long r = 0; r < n_trees; ++r) total += ll[r];      // serial, in tree order (smcsmc.cpp:145)
    *mean_total_out = total / (double)n_trees;
    return 0;
}

// ------------------------------------------------------------------ lag calibration (host driver)
// calculate_median_survival_distances (smcsmc.cpp:169-263).  The reference grows its sample one
// tree at a time with a shared RNG; here trees are simulated in fixed batches of PF_CAL_BATCH
// independent Philox streams until every epoch has min_events samples (or max_trees is reached),
// then the same median / fallback rules are applied (smcsmc.cpp:235-262).
#define PF_CAL_BATCH 16384

static int median_survival_impl(const pf_model* m, uint64_t seed, int32_t min_events, int64_t max_trees, double* median_out,
                                int64_t* trees_used, int32_t debug, int device) {
    {
        std::string why;
        if (sample_times_refusal(m, why, "pf_median_survival")) { g_err = why; return -1; }
    }
    if (test_setup(device)) return -1;
    if (m->n_pops < 1 || m->n_pops > PF_POPS_TAKEN(m) || m->nsam < 2 || m->nsam > (m->n_pops == 1 ? PF_NMAX_WIDE : PF_NMAX) || m->n_epochs < 1 ||
        m->n_epochs > PF_EMAX || (m->n_pops > PF_PMAX && m->n_epochs > PF_EMAX_PWIDE)) {
        g_err = "pf_median_survival: unsupported model (nsam 2..64 with one population, 2..16 with several; 1..4 populations, 1..8 with PF_MODEL_WIDE_POPS and then at most 32 epochs with more than four)";
        return -1;
    }
    // one population beyond 16 haplotypes (or PF_DEBUG_FORCE_WIDE): the wide kernel, same trees and walk
    const bool wide = m->n_pops == 1 && (m->nsam > PF_NMAX || (debug & PF_DEBUG_FORCE_WIDE));
    const int E = m->n_epochs, n = m->nsam, P = m->n_pops;
    KArgs A;
    memset(&A, 0, sizeof(A));
    A.E = E; A.n = n; A.P = P; A.L = m->loci_length; A.mu = m->mutation_rate; A.rho = m->recombination_rate; A.mcap = PF_MMAX;
    DevMem mem;
    int *dep, *derr; double* ddist;
    // The stopping rule is evaluated batch by batch (D8), but PF_CAL_GROUP batches are simulated per launch: a batch of
    // 16 384 trees fills a quarter of the SIMDs and takes as long as four.  Batches behind the one at which the rule
    // fires are discarded, so the result is that of one launch per batch.
    constexpr int PF_CAL_GROUP = 4;
    const size_t per_batch = (size_t)PF_CAL_BATCH * (n - 1);
    if (upload_model_tables(m, A, mem, 0) || mem.alloc(&derr, 1, 0) || mem.reserve(&dep, PF_CAL_GROUP * per_batch) ||
        mem.reserve(&ddist, PF_CAL_GROUP * per_batch)) return -1;
    std::vector<std::vector<double>> surv(E);
    std::vector<int> hep(PF_CAL_GROUP * per_batch);
    std::vector<double> hdist(PF_CAL_GROUP * per_batch);
    long long trees = 0;
    const size_t smem = P > 1 ? (model_sample_times(m) ? pf_mp_smem_bytes_anc(n, E, P, PF_MMAX) : pf_mp_smem_bytes(n, E, P, PF_MMAX))
                              : (wide ? pf_wide_smem_bytes(n, E) : smem_bytes(n, E));
    if (P > 1 && pf_mp_prepare(smem, PF_MMAX)) { g_err = "pf_median_survival: the local-tree state does not fit the LDS"; return -1; }
    if (wide && pf_wide_prepare(smem)) { g_err = "pf_median_survival: the local-tree state does not fit the LDS"; return -1; }
    const size_t smem_cal = smem + (size_t)(2 * PF_EPAD + E) * 8;          // + the padded epoch tables of the register path
    if (P == 1 && !wide && smem_cal > 64 * 1024) {
        hipFuncSetAttribute((const void*)k_calibrate<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_cal);
        hipFuncSetAttribute((const void*)k_calibrate<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_cal);
        hipFuncSetAttribute((const void*)k_calibrate<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_cal);
    }
    int cal_err = 0;
    auto finished = [&]() {
        int not_done = 0;
        for (int e = 0; e < E; ++e) not_done += (int)surv[e].size() < min_events;
        return not_done == 0 || trees >= max_trees;
    };
    while (!finished()) {
        const long long nrep = (long long)PF_CAL_GROUP * PF_CAL_BATCH;
        if (P > 1)
            pf_mp_launch_calibrate(A, (unsigned long long)seed, trees, nrep, dep, ddist, derr, smem, 0);
        else if (wide)
            pf_wide_launch_calibrate(A, (unsigned long long)seed, trees, nrep, dep, ddist, smem, 0);
        else
        {
            const dim3 grid((unsigned)(nrep / PF_BS)), blk(PF_BS);
            if (n <= 4) hipLaunchKernelGGL(k_calibrate<4>, grid, blk, smem_cal, 0, A, (unsigned long long)seed, trees, nrep, dep, ddist);
            else if (n <= 8) hipLaunchKernelGGL(k_calibrate<8>, grid, blk, smem_cal, 0, A, (unsigned long long)seed, trees, nrep, dep, ddist);
            else hipLaunchKernelGGL(k_calibrate<0>, grid, blk, smem_cal, 0, A, (unsigned long long)seed, trees, nrep, dep, ddist);
        }
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(&cal_err, derr, 4, hipMemcpyDeviceToHost));
        if (cal_err) break;
        HIPCHK(hipMemcpy(hep.data(), dep, hep.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hdist.data(), ddist, hdist.size() * 8, hipMemcpyDeviceToHost));
        for (int b = 0; b < PF_CAL_GROUP && !finished(); ++b) {
            for (size_t i = b * per_batch; i < (b + 1) * per_batch; ++i)
                if (hdist[i] >= 0) surv[hep[i]].push_back(hdist[i]);
            trees += PF_CAL_BATCH;
        }
    }
    mem.clear();
    if (cal_err) {
        g_err = cal_err == 1 ? "too many migration events on one local tree"
              : cal_err == 3 ? "No final coalescence event was sampled!" : "structured-model genealogy update failed";
        return -1;
    }
    if (trees_used) *trees_used = trees;
    // smcsmc.cpp:235-262
    double earliest = -1;
    for (int e = 0; e < E; ++e) {
        std::sort(surv[e].begin(), surv[e].end());
        int median_idx = ((int)surv[e].size() - 1) / 2;
        if (median_idx < 10) median_out[e] = -1;
        else {
            median_out[e] = surv[e][median_idx];
            if (earliest < 0) earliest = median_out[e];
        }
    }
    for (int e = 0; e < E; ++e)
        if (median_out[e] < 0) median_out[e] = e > 0 ? median_out[e - 1] : earliest;
    return 0;
}

int pf_median_survival(const pf_model* m, uint64_t seed, int32_t min_events, int64_t max_trees, double* median_out,
                       int64_t* trees_used, int device) {
    return median_survival_impl(m, seed, min_events, max_trees, median_out, trees_used, 0, device);
}

int pf_median_survival_opts(const pf_model* m, uint64_t seed, int32_t min_events, int64_t max_trees, double* median_out,
                            int64_t* trees_used, int32_t debug, int device) {
    return median_survival_impl(m, seed, min_events, max_trees, median_out, trees_used, debug, device);
}

// One population, 2..64 haplotypes, 64-bit carrier masks: the wide kernel (k_simulate_wide, the body of k_simulate).
int pf_simulate_sites_wide(const pf_model* m, uint64_t seed, int32_t nchunks, int64_t max_sites, double* pos, uint64_t* masks,
                        int64_t* n_sites, int device) {
    if (test_setup(device)) return -1;
    if (m->n_pops != 1 || m->nsam < 2 || m->nsam > PF_NMAX_WIDE || m->n_epochs < 1 || m->n_epochs > PF_EMAX || nchunks < 1 || max_sites < 1) {
        g_err = "pf_simulate_sites_wide: one population, 2..64 haplotypes, 1..64 epochs";
        return -1;
    }
    const int E = m->n_epochs, n = m->nsam;
    KArgs A;
    memset(&A, 0, sizeof(A));
    A.E = E; A.n = n; A.P = 1; A.L = m->loci_length; A.mu = m->mutation_rate; A.rho = m->recombination_rate; A.mcap = PF_MMAX;
    DevMem mem;
    double* dpos; unsigned long long* dmask; long long* dn;
    if (upload_model_tables(m, A, mem, 0) || mem.reserve(&dpos, (size_t)nchunks * max_sites) || mem.reserve(&dmask, (size_t)nchunks * max_sites) ||
        mem.reserve(&dn, (size_t)nchunks)) return -1;
    const size_t smem = pf_wide_smem_bytes(n, E);
    if (pf_wide_prepare(smem)) { g_err = "pf_simulate_sites_wide: the local-tree state does not fit the LDS"; return -1; }
    pf_wide_launch_simulate(A, (unsigned long long)seed, (int)nchunks, (long long)max_sites, dpos, dmask, dn, smem, 0);
    if (check_launch("k_simulate_wide")) return -1;
    if (hipDeviceSynchronize() != hipSuccess) { g_err = "k_simulate_wide failed"; return -1; }
    std::vector<long long> hn(nchunks);
    HIPCHK(hipMemcpy(hn.data(), dn, (size_t)nchunks * 8, hipMemcpyDeviceToHost));
    for (int c = 0; c < nchunks; ++c) {
        n_sites[c] = hn[c];
        const long long k = std::min<long long>(std::llabs(hn[c]), max_sites);
        HIPCHK(hipMemcpy(pos + (size_t)c * max_sites, dpos + (size_t)c * max_sites, (size_t)k * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(masks + (size_t)c * max_sites, dmask + (size_t)c * max_sites, (size_t)k * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

// Synthetic data for `nchunks` independent chunks of the model's length (one population): site positions and carrier
// masks per chunk (k_simulate).  n_sites[c] < 0: more than max_sites sites (the first max_sites are valid).
int pf_simulate_sites(const pf_model* m, uint64_t seed, int32_t nchunks, int64_t max_sites, double* pos, uint32_t* masks,
                      int64_t* n_sites, int device) {
    if (model_sample_times(m)) { g_err = "pf_simulate_sites: the site simulator is not supported with sample times (-eI, ancient samples)"; return -1; }
    if (test_setup(device)) return -1;
    if (m->n_pops < 1 || m->n_pops > PF_PMAX || m->nsam < 2 || m->nsam > PF_NMAX || m->n_epochs < 1 || m->n_epochs > PF_EMAX || nchunks < 1 || max_sites < 1) {
        g_err = m->n_pops > PF_PMAX && m->n_pops <= PF_PWIDE ? "pf_simulate_sites: the site simulator takes at most four populations (the filter takes up to eight)"
                                                              : "pf_simulate_sites: 1..4 populations, 2..16 haplotypes, 1..64 epochs";
        return -1;
    }
    const int E = m->n_epochs, n = m->nsam, P = m->n_pops;
    KArgs A;
    memset(&A, 0, sizeof(A));
    A.E = E; A.n = n; A.P = P; A.L = m->loci_length; A.mu = m->mutation_rate; A.rho = m->recombination_rate; A.mcap = PF_MMAX;
    DevMem mem;
    double* dpos; unsigned* dmask; long long* dn;
    if (upload_model_tables(m, A, mem, 0) || mem.reserve(&dpos, (size_t)nchunks * max_sites) || mem.reserve(&dmask, (size_t)nchunks * max_sites) ||
        mem.reserve(&dn, (size_t)nchunks)) return -1;
    int* derr = nullptr;
    int rc = 0;
    if (P > 1) {
        // structured model: the LDS-tree walk of pf_mp.h, one lane per chunk
        if (mem.alloc(&derr, 1, 0)) return -1;
        const size_t smem = pf_mp_smem_bytes(n, E, P, PF_MMAX);
        if (pf_mp_prepare(smem, PF_MMAX)) { g_err = "pf_simulate_sites: the local-tree state does not fit the LDS"; return -1; }
        pf_mp_launch_simulate(A, (unsigned long long)seed, (int)nchunks, (long long)max_sites, dpos, dmask, dn, derr, smem, 0);
    } else {
        const size_t smem = smem_bytes(n, E);
        if (smem > 64 * 1024) hipFuncSetAttribute((const void*)k_simulate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        hipLaunchKernelGGL(k_simulate, dim3((unsigned)((nchunks + PF_BS - 1) / PF_BS)), dim3(PF_BS), smem, 0, A, (unsigned long long)seed,
                           (int)nchunks, (long long)max_sites, dpos, dmask, dn);
    }
    rc = check_launch("k_simulate");
    if (!rc && hipDeviceSynchronize() != hipSuccess) { g_err = "k_simulate failed"; rc = -1; }
    if (!rc && derr) {
        int herr = 0;
        HIPCHK(hipMemcpy(&herr, derr, 4, hipMemcpyDeviceToHost));
        if (herr) { g_err = herr == 1 ? "too many migration events on one local tree" : (herr == 3 ? "No final coalescence event was sampled!" : "structured simulation: internal error"); rc = -1; }
    }
    if (!rc) {
        std::vector<long long> hn(nchunks);
        HIPCHK(hipMemcpy(hn.data(), dn, (size_t)nchunks * 8, hipMemcpyDeviceToHost));
        for (int c = 0; c < nchunks; ++c) {
            n_sites[c] = hn[c];
            const long long k = std::min<long long>(std::llabs(hn[c]), max_sites);
            HIPCHK(hipMemcpy(pos + (size_t)c * max_sites, dpos + (size_t)c * max_sites, (size_t)k * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(masks + (size_t)c * max_sites, dmask + (size_t)c * max_sites, (size_t)k * 4, hipMemcpyDeviceToHost));
        }
    }
    return rc;
}
