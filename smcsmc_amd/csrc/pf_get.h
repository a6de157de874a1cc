// smcsmc_amd/csrc/pf_get.h -- what is read back from a handle: pf_sync, pf_finish, the getters, the tree dump (-arg), timing and traces.
// Included once, by pf_hip.hip, behind pf_run.h.
#pragma once

int pf_sync(pf_handle* h) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->cstream));
    if (h->fin_pending) {
        hipLaunchKernelGGL(k_count_fin, dim3(1), dim3(256), 0, h->stream, h->A);
        h->fin_pending = false;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (harvest_spans(h)) return -1;
    Ctrl c;
    if (read_ctrl(h, c)) return -1;
    if (c.err) {
        const char* msg = "unknown device error";
        if (c.err == ERR_LOG_OVERFLOW) msg = "event log ring overflow (raise pf_params.log_cap)";
        if (c.err == ERR_GEN_OVERFLOW) msg = "generation ledger overflow (raise pf_params.gen_cap)";
        if (c.err == ERR_ZERO_PROB) msg = "Zero or negative probabilities";   /* pc.cpp:428-429 */
        if (c.err == ERR_MIG_OVERFLOW) msg = "too many migration events on one local tree";
        if (c.err == ERR_MP_INTERNAL) msg = "structured-model genealogy update: coalescence partners inconsistent";
        if (c.err == ERR_NO_COALESCENCE) msg = "No final coalescence event was sampled!";   /* particle.cpp:1383 */
        if (c.err == ERR_DELAY_OVERFLOW) msg = "delayed-factor store overflow (raise pf_params.delay_cap)";
        if (c.err == ERR_PAIR_STALL) msg = "row kernel, paired form: a wavefront waited 0.1 s for its partner (PF_DEBUG_NO_PAIR runs the other form)";
        g_err = msg;
        return -2;
    }
    return 0;
}

int pf_finish(pf_handle* h) {
    HIPCHK(hipSetDevice(h->device));
    // smcsmc.cpp:371: normalize_probability once more, then the lag-free flush (373)
    h->A.sp = (int)(h->seg_done & 1);
    if (h->ev_cnt) hipStreamWaitEvent(h->stream, h->ev_cnt, 0);     // k_partials rewrites the parity buffers
    hipLaunchKernelGGL(k_partials, dim3(h->nblocks), dim3(PF_BS), 0, h->stream, h->A);
    h->step_windows = host_windows(h, h->h_L, true);
    if (launch_decide(h, 0, 1, h->step_windows)) return -1;
    if (launch_resample(h, 0)) return -1;    // flag == 0 in mode 1: in-place normalisation
    if (launch_count(h, 0, h->step_windows)) return -1;
    if (launch_ledger(h, 0)) return -1;
    h->finished = true;
    return pf_sync(h);
}

int64_t pf_num_segments_done(pf_handle* h) { return h->seg_done; }

double pf_logl(pf_handle* h) {
    if (pf_sync(h)) return NAN;
    Ctrl c;
    if (read_ctrl(h, c)) return NAN;
    return c.logl;
}

int pf_get_counts(pf_handle* h, double* out, int32_t n) {
    if (pf_sync(h)) return -1;
    const int E = h->E, P = h->P;
    if (n < PF_COUNTS_LEN2(E, P)) { g_err = "count buffer too small"; return -1; }
    Ctrl c;
    if (read_ctrl(h, c)) return -1;
    double* tail;
    if (P == 1) {
        HIPCHK(hipMemcpy(out, h->A.totals, (size_t)6 * E * 8, hipMemcpyDeviceToHost));
        tail = out + 6 * E;
    } else {
        // device layout: totals[column][epoch]; columns as AccT<P>.  A kernel compiled for PF_PMAX populations
        // (P == 3) still uses the column numbering of its template parameter, and so does that of PF_PWIDE (P == 5 .. 7).
        const int PT = pf_count_pops(P);
        const int ncol = h->A.ncol;
        std::vector<double> tot;
        if (download(tot, h->A.totals, (size_t)ncol * E)) return -1;
        auto col = [&](int k, int e) { return tot[(size_t)k * E + e]; };
        double* o = out;
        for (int stat = 0; stat < 3; ++stat) {                 // coal count, opp, weight [E][P]
            for (int e = 0; e < E; ++e) for (int a = 0; a < P; ++a) o[e * P + a] = col(stat * PT + a, e);
            o += E * P;
        }
        for (int stat = 0; stat < 3; ++stat) {                 // recomb count, opp, weight [E]
            for (int e = 0; e < E; ++e) o[e] = col(3 * PT + stat, e);
            o += E;
        }
        for (int e = 0; e < E; ++e) for (int a = 0; a < P; ++a) for (int b = 0; b < P; ++b)
            o[(e * P + a) * P + b] = col(3 * PT + 3 + a * PT + b, e);
        o += E * P * P;
        for (int e = 0; e < E; ++e) for (int a = 0; a < P; ++a) o[e * P + a] = col(3 * PT + 3 + PT * PT + a, e);
        o += E * P;
        for (int e = 0; e < E; ++e) for (int a = 0; a < P; ++a) o[e * P + a] = col(3 * PT + 3 + PT * PT + PT + a, e);
        o += E * P;
        tail = o;
    }
    tail[0] = c.delayed_opp;
    tail[1] = c.delayed_count;
    tail[2] = (double)c.n_resample;
    tail[3] = c.logl;
    return 0;
}

int pf_get_local_recomb(pf_handle* h, double* opp_diff, double* counts, int64_t nbins) {
    if (pf_sync(h)) return -1;
    if (!h->A.lmap_opp) { g_err = "pf_get_local_recomb: the map was not recorded (pf_params.flags bit 0)"; return -1; }
    const long long nb = h->A.lmap_bins;
    std::vector<double> o, c;
    if (download(o, h->A.lmap_opp, (size_t)nb) || download(c, h->A.lmap_cnt, (size_t)(h->n + 2) * nb)) return -1;
    for (long long b = 0; b < nbins; ++b) {
        opp_diff[b] = b < nb ? o[b] : 0.0;
        for (int k = 0; k < h->n + 2; ++k) counts[(size_t)k * nbins + b] = b < nb ? c[(size_t)k * nb + b] : 0.0;
    }
    return 0;
}

int pf_get_migrations(pf_handle* h, int32_t* n_events, double* times, int8_t* branch, int8_t* newpop, int8_t* node_pops,
                      int32_t cap) {
    if (pf_sync(h)) return -1;
    if (h->P < 2) { g_err = "pf_get_migrations: the model has one population"; return -1; }
    Ctrl c;
    if (read_ctrl(h, c)) return -1;
    const DState st = state_slot(h->A, c.cur);
    const long long Np = h->Np;
    const int n = h->n;
    const int mcap = h->A.mcap;
    std::vector<int> nm;
    std::vector<double> mt;
    std::vector<int8_t> mb, mq, pn;
    if (download(nm, st.nm, (size_t)Np) || download(mt, st.Mt, (size_t)mcap * Np) || download(mb, st.Mb, (size_t)mcap * Np) ||
        download(mq, st.Mq, (size_t)mcap * Np) || download(pn, st.Pn, (size_t)(n - 1) * Np)) return -1;
    for (long long p = 0; p < Np; ++p) {
        if (n_events) n_events[p] = nm[p];
        for (int k = 0; k < cap; ++k) {
            bool ok = k < nm[p] && k < mcap;
            if (times) times[p * cap + k] = ok ? mt[(size_t)k * Np + p] : 0.0;
            if (branch) branch[p * cap + k] = ok ? mb[(size_t)k * Np + p] : 0;
            if (newpop) newpop[p * cap + k] = ok ? (mq[(size_t)k * Np + p] & (h->P > PF_PMAX ? 7 : 3)) : 0;      // the upper bits hold the event's epoch
        }
        if (node_pops) for (int r = 0; r < n - 1; ++r) node_pops[p * (n - 1) + r] = pn[(size_t)r * Np + p];
    }
    return 0;
}

int pf_get_trace(pf_handle* h, double* T, double* ess, int32_t* resampled, double* logl, int64_t n) {
    if (pf_sync(h)) return -1;
    long long m = std::min<long long>(n, h->seg_done);
    if (m <= 0) return 0;
    if (T) HIPCHK(hipMemcpy(T, h->A.tr_T, m * 8, hipMemcpyDeviceToHost));
    if (ess) HIPCHK(hipMemcpy(ess, h->A.tr_ess, m * 8, hipMemcpyDeviceToHost));
    if (logl) HIPCHK(hipMemcpy(logl, h->A.tr_logl, m * 8, hipMemcpyDeviceToHost));
    if (resampled) HIPCHK(hipMemcpy(resampled, h->A.tr_flag, m * 4, hipMemcpyDeviceToHost));
    return (int)m;
}

int pf_get_resample_events(pf_handle* h, int32_t* seg_idx, int32_t* parents, int32_t max_events) {
    if (pf_sync(h)) return -1;
    Ctrl c;
    if (read_ctrl(h, c)) return -1;
    int nev = (int)std::min<long long>(std::min<long long>(c.n_resample, h->max_trace_events), max_events);
    if (nev <= 0) return 0;
    if (seg_idx) HIPCHK(hipMemcpy(seg_idx, h->A.ev_seg, (size_t)nev * 4, hipMemcpyDeviceToHost));
    if (parents) HIPCHK(hipMemcpy(parents, h->A.ev_parents, (size_t)nev * h->Np * 4, hipMemcpyDeviceToHost));
    return nev;
}

int pf_get_particles(pf_handle* h, double* w_post, double* w_pilot, double* heights, int8_t* children, double* next_base) {
    if (pf_sync(h)) return -1;
    Ctrl c;
    if (read_ctrl(h, c)) return -1;
    const DState st = state_slot(h->A, c.cur);
    const long long Np = h->Np;
    const int n = h->n;
    if (w_post) HIPCHK(hipMemcpy(w_post, st.w_post, Np * 8, hipMemcpyDeviceToHost));
    if (w_pilot) HIPCHK(hipMemcpy(w_pilot, st.w_pilot, Np * 8, hipMemcpyDeviceToHost));
    if (next_base) HIPCHK(hipMemcpy(next_base, st.next_base, Np * 8, hipMemcpyDeviceToHost));
    if (heights) {
        std::vector<double> tmp;
        if (download(tmp, st.S, (size_t)(n - 1) * Np)) return -1;
        for (long long p = 0; p < Np; ++p)
            for (int r = 0; r < n - 1; ++r) heights[p * (n - 1) + r] = tmp[(size_t)r * Np + p];
    }
    if (children) {
        std::vector<int8_t> tmp;
        if (download(tmp, st.C, (size_t)2 * (n - 1) * Np)) return -1;
        for (long long p = 0; p < Np; ++p)
            for (int k = 0; k < 2 * (n - 1); ++k) children[p * 2 * (n - 1) + k] = tmp[(size_t)k * Np + p];
    }
    return 0;
}

// Philox4x32-10 on the host (the same stream definition as philox_uniform in pf_device.h): the final one-particle draw
// needs a single uniform
static double philox_uniform_host(unsigned long long seed, unsigned slot, unsigned stream, unsigned long long draw) {
    unsigned c0 = (unsigned)draw, c1 = (unsigned)(draw >> 32), c2 = slot, c3 = stream;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const unsigned long long bits = (((unsigned long long)c0 << 32) | c1) >> 11;
    return ((double)bits + 0.5) * 1.1102230246251565e-16;
}

// ------------------------------------------------------------------ -arg: the history of one particle
// ParticleContainer::printTrees (pc.cpp:515-555) prints the tree-modifying events of the particle left by the final
// one-particle draw (smcsmc.cpp:395).  Here: walk back through the generations (the parent tables of all resamplings
// are kept with -arg), collect the record ranges of every ancestor, copy them out.
__global__ void k_trace_ancestry(KArgs A, int G, int slot, int* out_slot, unsigned* out_k0, unsigned* out_k1) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long a = slot;
    for (int g = G; g >= 0; --g) {
        out_slot[g] = (int)a;
        out_k0[g] = A.gstart[(size_t)(g % A.Gcap) * A.Np + a];
        out_k1[g] = g == G ? A.widx[a] : A.gstart[(size_t)((g + 1) % A.Gcap) * A.Np + a];
        if (g > 0) a = A.ev_parents[(size_t)(g - 1) * A.Np + a];
    }
}
__global__ void k_gather_records(KArgs A, int ngen, const int* slot, const unsigned* k0, const unsigned* k1, const long long* off,
                                 double* out) {
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= ngen) return;
    double* o = out + (size_t)off[g] * A.RS;
    for (unsigned k = k0[g]; k < k1[g]; ++k) {
        const double* rec = rec_ptr(A, slot[g], k);
        for (int j = 0; j < A.RS; ++j) *o++ = rec[j];
    }
}

// pieces of the records gathered by k_gather_records (structured models): entry i copies np[i] pieces of slot[i] from pstart[i]
__global__ void k_gather_pieces(KArgs A, int nrec, const int* slot, const unsigned* pstart, const unsigned* np, const long long* off,
                                double* out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= nrec) return;
    double* o = out + (size_t)off[i] * 3;
    for (unsigned j = 0; j < np[i]; ++j) {
        const double* q = A.plog + ((size_t)slot[i] * A.pcap + ((pstart[i] + j) % A.pcap)) * 3;
        *o++ = q[0]; *o++ = q[1]; *o++ = q[2];
    }
}

int64_t pf_sample_tree_events(pf_handle* h, int32_t* kind, double* pos, double* height, uint32_t* desc, int64_t max_events,
                              int64_t* particle_out) {
    return pf_sample_tree_events_pops(h, kind, pos, height, desc, nullptr, nullptr, max_events, particle_out);
}

int64_t pf_sample_tree_events_pops(pf_handle* h, int32_t* kind, double* pos, double* height, uint32_t* desc, int32_t* from_pop,
                                   int32_t* to_pop, int64_t max_events, int64_t* particle_out) {
    if (!h->A.rec_trees) { g_err = "pf_sample_tree_events: the handle was not created with tree recording (pf_params.flags bit 1)"; return -1; }
    if (pf_sync(h)) return -1;
    Ctrl c;
    if (read_ctrl(h, c)) return -1;
    const long long Np = h->Np;
    // the one-particle systematic draw of resample(..., NULL, 1): the particle whose cumulative pilot weight
    // (pilotWeight(), pc.cpp:256-262) passes U * total
    std::vector<double> w;
    if (download(w, state_slot(h->A, c.cur).w_pilot, (size_t)Np)) return -1;
    double total = 0.0;
    for (double v : w) total += v;
    const double u = philox_uniform_host((unsigned long long)h->A.seed, 0xFFFFFFFFu, 1, (unsigned long long)c.n_resample);
    long long j = 0;
    double acc = 0.0;
    for (; j < Np - 1; ++j) { acc += w[j]; if (acc > u * total) break; }
    if (particle_out) *particle_out = j;
    const int G = c.gen;
    // (the host vectors the uploads read stand before the owner of the temporaries: when a failure leaves, hipFree waits for the device first)
    std::vector<unsigned> k0, k1, rstart, rnp;
    std::vector<long long> off(G + 1);
    std::vector<long long> poff;
    std::vector<int> rslot;
    DevMem tmp;
    int* dslot; unsigned *dk0, *dk1; const long long* doff;
    if (tmp.reserve(&dslot, (size_t)G + 1) || tmp.reserve(&dk0, (size_t)G + 1) || tmp.reserve(&dk1, (size_t)G + 1)) return -1;
    hipLaunchKernelGGL(k_trace_ancestry, dim3(1), dim3(1), 0, h->stream, h->A, G, (int)j, dslot, dk0, dk1);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (download(k0, dk0, (size_t)G + 1) || download(k1, dk1, (size_t)G + 1)) return -1;
    long long nrec = 0;
    for (int g = 0; g <= G; ++g) { off[g] = nrec; nrec += (long long)(k1[g] - k0[g]); }
    const int RS = h->A.RS;
    double* drec;
    if (tmp.upload(&doff, off.data(), (size_t)G + 1, h->stream) || tmp.reserve(&drec, (size_t)nrec * RS)) return -1;
    hipLaunchKernelGGL(k_gather_records, dim3((unsigned)((G + 1 + 255) / 256)), dim3(256), 0, h->stream, h->A, G + 1, dslot, dk0, dk1, doff, drec);
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<double> rec;
    if (download(rec, drec, (size_t)nrec * RS)) return -1;
    // structured models: the migrations and the coalescence of an update are in its pieces (pf_mp.h PLog)
    std::vector<double> pieces;
    poff.assign((size_t)nrec + 1, 0);
    if (h->P > 1 && nrec) {
        std::vector<int> gslot;
        if (download(gslot, dslot, (size_t)G + 1)) return -1;
        rslot.resize((size_t)nrec); rstart.resize((size_t)nrec); rnp.resize((size_t)nrec);
        for (int g = 0; g <= G; ++g)
            for (long long r = off[g]; r < off[g] + (long long)(k1[g] - k0[g]); ++r) rslot[(size_t)r] = gslot[g];
        for (long long r = 0; r < nrec; ++r) {
            const double* q = &rec[(size_t)r * RS];
            unsigned long long meta, ref;
            memcpy(&meta, &q[4], 8);
            memcpy(&ref, &q[3], 8);
            const int type = (int)(meta & 0xff);
            const bool has = type == 0 || type == 2;
            rstart[(size_t)r] = has ? (unsigned)(ref & 0xffffffffu) : 0u;
            rnp[(size_t)r] = has ? (unsigned)(ref >> 32) : 0u;
            poff[(size_t)r + 1] = poff[(size_t)r] + rnp[(size_t)r];
        }
        const long long npieces = poff[(size_t)nrec];
        const int* d_s; const unsigned *d_p0, *d_np; const long long* d_off; double* d_out;
        if (tmp.upload(&d_s, rslot.data(), (size_t)nrec, h->stream) || tmp.upload(&d_p0, rstart.data(), (size_t)nrec, h->stream) ||
            tmp.upload(&d_np, rnp.data(), (size_t)nrec, h->stream) || tmp.upload(&d_off, poff.data(), (size_t)nrec, h->stream) ||
            tmp.reserve(&d_out, (size_t)npieces * 3)) return -1;
        hipLaunchKernelGGL(k_gather_pieces, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, h->stream, h->A, (int)nrec, d_s, d_p0, d_np, d_off, d_out);
        HIPCHK(hipStreamSynchronize(h->stream));
        if (download(pieces, d_out, (size_t)npieces * 3)) return -1;
    }
    tmp.clear();
    // last position first; within an update the R line precedes the C line, which precedes the M lines of the walk that
    // led to it, latest first (the reference prepends every event to one list and prints from its head, pc.cpp:527-551)
    int64_t nout = 0;
    auto emit = [&](int kd, double x, double t, unsigned d, int from, int to) {
        if (nout < max_events) {
            if (kind) kind[nout] = kd;
            if (pos) pos[nout] = x;
            if (height) height[nout] = t;
            if (desc) desc[nout] = d;
            if (from_pop) from_pop[nout] = from;
            if (to_pop) to_pop[nout] = to;
        }
        ++nout;
    };
    const unsigned full = (1u << h->n) - 1u;
    for (long long r = nrec - 1; r >= 0; --r) {
        const double* q = &rec[(size_t)r * RS];
        unsigned long long meta;
        memcpy(&meta, &q[4], 8);
        const int type = (int)(meta & 0xff);
        if (type != 0 && type != 2) continue;
        const unsigned cut = (unsigned)((meta >> 32) & 0xffff), below = (unsigned)((meta >> 48) & 0xffff);
        if (type == 0) emit(0, q[1], q[2], cut, -1, -1);
        if (h->P == 1) { emit(1, q[1], q[3], below, 0, -1); continue; }
        // the floating lineage is the cut branch (an update) or leaf i on its way into the partial tree (initial tree:
        // n_eff = i); the other active lineage is the root's own, above everything that is not the floating lineage
        const int leaf = (int)((meta >> 24) & 0xff);
        const unsigned fl = type == 0 ? cut : (1u << leaf);
        const unsigned rt = type == 0 ? (full & ~cut) : ((1u << leaf) - 1u);
        for (long long j = poff[(size_t)r + 1] - 1; j >= poff[(size_t)r]; --j) {
            long long tag;
            memcpy(&tag, &pieces[(size_t)j * 3], 8);
            const int pop = (int)(tag & 0xff), kd = (int)((tag >> 8) & 0xff), to = (int)((tag >> 16) & 0xff);
            const double t1 = pieces[(size_t)j * 3 + 2];
            if (kd & 1) emit(1, q[1], t1, below, pop, -1);
            if (kd & 2) emit(2, q[1], t1, (kd & 4) ? rt : fl, pop, to);
        }
    }
    return nout;
}

int pf_set_timing(pf_handle* h, int period) {
    h->timing_period = period;
    if (period > 0 && h->span_overhead_ms == 0) {
        // A span is two event records around one launch; what the pair measures with nothing in between is not kernel
        // time.  Median of 64 empty spans, subtracted from every span, so that the per-launch figure agrees with the
        // kernel durations a profiler reports.
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        std::vector<float> empty;
        for (int i = 0; i < 64; ++i) {
            hipEvent_t a = get_event(h), b = get_event(h);
            hipEventRecord(a, h->stream); hipEventRecord(b, h->stream);
            HIPCHK(hipEventSynchronize(b));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, a, b));
            empty.push_back(ms);
            h->ev_pool.push_back(a); h->ev_pool.push_back(b);
        }
        std::sort(empty.begin(), empty.end());
        h->span_overhead_ms = empty[empty.size() / 2];
    }
    return 0;
}

// profiling builds (-DPF_STAMPS): wall-clock stamps (100 MHz) of the phases of the extend workgroups, one set per row and
// wavefront; a regular build records nothing
int pf_debug_stamps(pf_handle* h, int64_t rows, uint64_t* out) {
    HIPCHK(hipSetDevice(h->device));
    if (rows > 0 && !out) {
        unsigned long long* buf = nullptr;
        if (h->alloc(&buf, (size_t)rows * h->A.nc * PF_STAMP_W)) return -1;
        HIPCHK(hipMemset(buf, 0, (size_t)rows * h->A.nc * PF_STAMP_W * 8));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->A.stamps = buf; h->A.stamp_rows = rows;
        return 0;
    }
    if (!h->A.stamps) { g_err = "pf_debug_stamps: not enabled"; return -1; }
    if (pf_sync(h)) return -1;
    HIPCHK(hipMemcpy(out, h->A.stamps, (size_t)std::min<long long>(rows, h->A.stamp_rows) * h->A.nc * PF_STAMP_W * 8, hipMemcpyDeviceToHost));
    return 0;
}

int pf_get_kernel_time(pf_handle* h, int k, double* ms, int64_t* launches) {
    if (k < 0 || k > 3) return -1;
    if (pf_sync(h)) return -1;
    // mean duration of the timed launches, scaled to all launches of this class
    double mean = h->k_timed[k] ? h->k_ms[k] / (double)h->k_timed[k] : 0.0;
    if (ms) *ms = mean * (double)h->k_launches[k];
    if (launches) *launches = h->k_launches[k];
    return 0;
}

// Measurement aid: steps [first_step, first_step + n_steps) of the next pf_run / pf_run_many calls led by this handle run the traced
// instance of the row kernel (k_sweep4t: at most four haplotypes, no focused sampling; other shapes ignore the request).
int pf_set_wg_trace(pf_handle* h, int64_t first_step, int32_t n_steps) {
    HIPCHK(hipSetDevice(h->device));
    if (pf_sync(h)) return -1;
    h->trace_mem.clear(); h->d_trace = nullptr;
    h->trace_t0 = (int)std::max<int64_t>(0, first_step);
    h->trace_n = std::max(0, n_steps);
    h->trace_stride = 0; h->trace_words = 0;
    return 0;
}

// The trace: four 64-bit words per workgroup slot of every traced step -- start and end (100 MHz clock; 0 0: slot not used by that step's
// grid), HW_ID | XCC_ID << 32, index within the chunk | chunk << 32.  Returns the number of words (0: nothing traced yet); copies at most
// cap_words of them; info = {steps, workgroup slots per step}.
int64_t pf_get_wg_trace(pf_handle* h, uint64_t* out, int64_t cap_words, int32_t* info) {
    if (hipSetDevice(h->device) != hipSuccess || pf_sync(h)) return -1;
    if (info) { info[0] = h->d_trace ? h->trace_n : 0; info[1] = h->trace_stride; }
    if (!h->d_trace) return 0;
    const size_t nw = std::min<size_t>(h->trace_words, (size_t)std::max<int64_t>(0, cap_words));
    if (out && nw && hipMemcpy(out, h->d_trace, nw * 8, hipMemcpyDeviceToHost) != hipSuccess) { g_err = "copy of the workgroup trace failed"; return -1; }
    return (int64_t)h->trace_words;
}

int pf_get_delay_stats(pf_handle* h, int64_t* n_forced, int32_t* peak_pending) {
    if (pf_sync(h)) return -1;
    Ctrl c;
    if (read_ctrl(h, c)) return -1;
    if (n_forced) *n_forced = (int64_t)c.n_delay_evict;
    if (peak_pending) *peak_pending = c.delay_peak;
    return 0;
}

int pf_get_stats(pf_handle* h, int64_t* n_records, int64_t* state_bytes, int64_t* n_resamples) {
    if (pf_sync(h)) return -1;
    if (n_records) {
        std::vector<unsigned> w;
        if (download(w, h->A.widx, (size_t)h->Np)) return -1;
        long long t = 0;
        for (unsigned v : w) t += v;
        *n_records = t;
    }
    if (state_bytes) *state_bytes = (int64_t)(h->n - 1) * 8 + 2 * (h->n - 1) + 5 * 8 + 4 + 8 + 8 + 4;
    if (n_resamples) {
        Ctrl c;
        if (read_ctrl(h, c)) return -1;
        *n_resamples = c.n_resample;
    }
    return 0;
}

