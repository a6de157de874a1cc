"""Structured models of five to eight populations: the wide walk (eight lineage counters, population and epoch of a migration event in
three and five bits of its byte) on the LDS-tree kernels at every number of haplotypes, and the count instance of eight populations
(migration counts collected in LDS).  Same bar as test_gpu_structured.py: trees, node populations, migration lists, weights, ESS,
log-likelihood and resampling indices bit-identical to the CPU oracle; CountModel sums within 1e-9 relative.

Every sweep case has a positive migration count in every ordered pair of populations and every population among the targets of the
stored migration events: an event byte still read with two bits of population would show there."""
import functools
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib
import trees_format

pytestmark = pytest.mark.gpu

COUNT_RTOL = 1e-9
NO_FUSE, FORCE_LDS = 2, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _canon_events(mg):
    """as test_gpu_structured.py: events at the same instant on different branches have no defined order"""
    out = []
    for i in range(len(mg["n_events"])):
        k = mg["n_events"][i]
        out.append(sorted(zip(_bits(mg["times"][i, :k]).tolist(), mg["branch"][i, :k].tolist(), mg["newpop"][i, :k].tolist())))
    return out


def _assert_state_equal(ref, g):
    po, pg = ref["particles"], g.particles()
    assert (po["children"] == pg["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(po[k]) == _bits(pg[k])).all(), k
    mo, mg = ref["migrations"], g.migrations()
    assert (mo["n_events"] == mg["n_events"]).all()
    assert (mo["node_pops"] == mg["node_pops"]).all()
    assert _canon_events(mo) == _canon_events(mg)


def _assert_trace_equal(ref, g):
    to, tg = ref["trace"], g.trace()
    assert g.segments_done() == len(to["T"])
    assert (to["resampled"] == tg["resampled"]).all()
    for k in ("T", "ess", "logl"):
        assert (_bits(to[k]) == _bits(tg[k])).all(), k
    so, po_ = ref["events"]; sg, pg_ = g.resample_events()
    assert (so == sg).all() and (po_ == pg_).all()


def _assert_counts_close(co, cg):
    for k in ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight", "mig_count", "mig_opp", "mig_weight"):
        np.testing.assert_allclose(cg[k], co[k], rtol=COUNT_RTOL, atol=1e-300, err_msg=k)
    assert cg["resample_count"] == co["resample_count"]


def _oracle_result(o):
    """what the comparisons read, taken once (the oracle object is let go)"""
    return dict(trace=o.trace(), events=o.resample_events(), particles=o.particles(), migrations=o.migrations(), counts=o.counts())


# ---------------------------------------------------------------- full sweeps
#        n  E  P  Np  seed mig   (n = 16, P = 8: mig 2.0 overflows the default mig_cap of 96 in the oracle)
SWEEPS = [(5, 8, 5, 300, 2, 2.0), (8, 8, 8, 256, 3, 2.0), (9, 8, 8, 192, 9, 2.0), (12, 8, 5, 200, 5, 2.0), (16, 8, 8, 192, 6, 1.0)]


@functools.lru_cache(maxsize=None)
def _sweep_inputs(n, E, P, seed, mig):
    base = cases.make_model(n=n, E=E, L=1.0e5)
    segs = cases.make_segments(base, seed=seed, max_seg_len=5000)
    return cases.make_structured(base, P=P, split_epoch=E - 3, mig=mig), segs


@functools.lru_cache(maxsize=None)
def _sweep_oracle(n, E, P, Np, seed, mig):
    model, segs = _sweep_inputs(n, E, P, seed, mig)
    o = oracle_lib.Oracle(model, Np, ess_fraction=0.5, seed=seed, max_trace_events=64)
    o.init_prior(segs["start"][0])
    o.run(o.pack_segments(model, segs))
    return _oracle_result(o)


@pytest.mark.parametrize("debug", [0, NO_FUSE], ids=["default", "no-fuse"])
@pytest.mark.parametrize("n,E,P,Np,seed,mig", SWEEPS)
def test_wide_full_sweep_parity(hiplib, n, E, P, Np, seed, mig, debug):
    """k_init_mp<8>, k_extend_mp<false, false, 8> and k_count<8 or 16, 8> against the oracle, below and above the register-tree limit of
    eight haplotypes; with PF_DEBUG_NO_FUSE the same path and the same bits."""
    from smcsmc_amd import ParticleFilter
    model, segs = _sweep_inputs(n, E, P, seed, mig)
    ref = _sweep_oracle(n, E, P, Np, seed, mig)
    g = ParticleFilter(model, Np, ess_fraction=0.5, seed=seed, max_trace_events=64, debug=debug)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    assert g.run_path() == "General"
    g.run(); g.finish()
    assert ref["trace"]["resampled"].sum() > 0, "test case must exercise resampling"
    _assert_trace_equal(ref, g)
    _assert_state_equal(ref, g)
    co, cg = ref["counts"], g.counts()
    off_diagonal = ~np.eye(P, dtype=bool)
    assert (co["mig_count"].sum(0)[off_diagonal] > 0).all(), "a migration count in every ordered pair of populations"
    mg = g.migrations()
    targets = set()
    for i in range(len(mg["n_events"])):
        targets.update(mg["newpop"][i, :mg["n_events"][i]].tolist())
    assert targets == set(range(P)), targets            # (three bits of population in the event byte: two would fold 4..7 onto 0..3)
    _assert_counts_close(co, cg)


def test_wide_focused_sampling_parity(hiplib):
    """-bias_heights / -bias_strengths with six populations: biased cut point, delayed importance weights, resampling with pending factors"""
    from smcsmc_amd import ParticleFilter
    n, E, P, Np, seed = 6, 6, 6, 300, 4
    base = cases.make_model(n=n, E=E, L=1.0e5)
    segs = cases.make_segments(base, seed=seed, max_seg_len=5000)
    model = dict(cases.make_structured(base, P=P, split_epoch=E - 3, mig=1.0), bias_heights=[400.0], bias_strengths=[5.0, 1.0],
                 application_delays=np.full(E, 3000.0))
    o = oracle_lib.Oracle(model, Np, seed=seed, max_trace_events=64); o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
    ref = _oracle_result(o)
    g = ParticleFilter(model, Np, seed=seed, max_trace_events=64)
    g.init_prior(segs["start"][0]); g.load_segments(segs); g.run(); g.finish()
    assert g.run_path() == "General"
    assert ref["trace"]["resampled"].sum() > 0
    _assert_trace_equal(ref, g)
    _assert_state_equal(ref, g)
    co, cg = ref["counts"], g.counts()
    for k in ("coal_count", "coal_opp", "rec_count", "rec_opp", "mig_count", "mig_opp"):       # sums in another order
        np.testing.assert_allclose(cg[k], co[k], rtol=COUNT_RTOL, atol=COUNT_RTOL * np.abs(co[k]).max(), err_msg=k)
    np.testing.assert_allclose(cg["delayed_opp"], co["delayed_opp"], rtol=1e-12)


@pytest.mark.parametrize("n,P,Np,seed", [(7, 7, 200, 7), (10, 6, 160, 8)])
def test_wide_tree_dump(hiplib, n, P, Np, seed):
    """-arg: the R, C and M lines of the drawn particle's history equal the oracle's event for event, populations up to P - 1 among them"""
    from smcsmc_amd import ParticleFilter, outfile
    E = 8
    base = cases.make_model(n=n, E=E, L=1.0e5)
    segs = cases.make_segments(base, seed=seed, max_seg_len=5000)
    model = cases.make_structured(base, P=P, split_epoch=E - 3, mig=2.0)
    g = ParticleFilter(model, Np, seed=seed, max_trace_events=0, record_trees=True, log_cap=8192, gen_cap=4096)
    g.init_prior(segs["start"][0]); g.load_segments(segs); g.run(); g.finish()
    assert g.trace()["resampled"].sum() > 3
    part, kind, pos, hgt, desc, fr, to = g.sample_tree_events(pops=True)
    o = oracle_lib.Oracle(model, Np, seed=seed, max_trace_events=0)
    o.enable_tree_recording()
    o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
    opart, okind, opos, ohgt, odesc, ofr, oto = o.sample_tree_events(pops=True)
    assert opart == part and len(okind) == len(kind)
    assert (okind == kind).all() and (odesc == desc).all() and (ofr == fr).all() and (oto == to).all()
    assert (_bits(opos) == _bits(pos)).all() and (_bits(ohgt) == _bits(hgt)).all()
    assert set(to[kind == 2].tolist()) == set(range(P)), "every population is the target of an M line"
    assert (np.diff(pos) <= 0).all()
    full = (1 << n) - 1
    i = 0
    while i < len(kind):
        if kind[i] == 0:                       # an update: R, C, M...
            cut = int(desc[i]); x = pos[i]; i += 1
            assert kind[i] == 1 and pos[i] == x and hgt[i] >= hgt[i - 1] and (int(desc[i]) & cut) == cut
        else:                                  # a leaf of the first tree: C, M...
            assert kind[i] == 1 and pos[i] == 0.0
            cut = None
        tc = hgt[i]; i += 1
        while i < len(kind) and kind[i] == 2:
            assert hgt[i] <= tc and fr[i] != to[i] and 0 <= to[i] < P
            if cut is not None:
                assert int(desc[i]) in (cut, full & ~cut)
            i += 1
    text = outfile.trees_text(kind, pos, hgt, desc, start_position=1.0, from_pop=fr, to_pop=to)
    assert len(text.splitlines()) == len(kind)
    trees_format.check_lines(text.splitlines(), nsam=n, npop=P)


@pytest.mark.parametrize("n,P", [(6, 5), (8, 8)])
def test_wide_auxiliary_particle_filter_parity(hiplib, n, P):
    """-apf 2 on the general kernels; the quantile table from prior trees of the structured model (k_tbl_mp<8>)"""
    from smcsmc_amd import ParticleFilter, pf, segments as segmod
    E = 6
    base = cases.make_model(n=n, E=E, L=1.2e5)
    model = cases.make_structured(base, P=P)
    segs = cases.make_segments(base, seed=30 + n, max_seg_len=5000)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    la = segmod.pack_lookahead(rows, n)
    tbl = pf.terminal_branch_quantiles(model, seed=1, n_trees=20000)
    o = oracle_lib.Oracle(model, 320, seed=9, max_trace_events=64); o.init_prior(segs["start"][0]); si = o.pack_segments(model, segs)
    g = ParticleFilter(model, 320, seed=9, max_trace_events=64); g.init_prior(segs["start"][0]); g.load_segments(segs)
    o.load_lookahead(la, 2, tbl); g.load_lookahead(la, 2, tbl)
    o.run(si); g.run(); g.finish()
    assert g.run_path() == "General"
    ref = _oracle_result(o)
    assert ref["trace"]["resampled"].sum() > 0
    _assert_trace_equal(ref, g)
    _assert_state_equal(ref, g)
    pg = g.particles()
    # the look-ahead sits in the pilot weight only (compared exactly: at the last row of the eight-population case the factors are within 1e-5 of one)
    assert (pg["w_post"] != pg["w_pilot"]).any()


def test_wide_recombination_guide_parity(hiplib):
    """-guide with six populations: position-dependent sampling rate, per-sample relative rates, importance weights"""
    from smcsmc_amd import ParticleFilter
    n, P, E = 6, 6, 6
    base = cases.make_model(n=n, E=E, L=1.2e5)
    model = dict(cases.make_structured(base, P=P), guide=cases.guide(base, 9, 2.5, n), application_delays=np.full(E, 3000.0))
    segs = cases.make_segments(base, seed=60 + n, max_seg_len=5000)
    o = oracle_lib.Oracle(model, 320, seed=6, max_trace_events=64); o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
    ref = _oracle_result(o)
    g = ParticleFilter(model, 320, seed=6, max_trace_events=64)
    g.init_prior(segs["start"][0]); g.load_segments(segs); g.run(); g.finish()
    assert ref["trace"]["resampled"].sum() > 0
    _assert_trace_equal(ref, g)
    _assert_state_equal(ref, g)
    co, cg = ref["counts"], g.counts()
    for k in ("coal_count", "coal_opp", "rec_count", "rec_opp", "mig_count", "mig_opp"):
        np.testing.assert_allclose(cg[k], co[k], rtol=COUNT_RTOL, atol=COUNT_RTOL * np.abs(co[k]).max(), err_msg=k)


def test_wide_tools_parity(hiplib):
    """lag calibration (k_calibrate_mp<8>) and terminal-branch quantiles (k_tbl_mp<8>) at six populations: device == oracle bit for bit"""
    from smcsmc_amd import pf
    model = cases.make_structured(cases.make_model(n=6, E=8, L=1e7), P=6, split_epoch=5)
    dm, dt = pf.median_survival(model, seed=1, min_events=50, max_trees=32768)
    om, ot = oracle_lib.median_survival(model, seed=1, min_events=50, max_trees=32768)
    assert dt == ot
    assert (_bits(dm) == _bits(om)).all()
    model = cases.make_structured(cases.make_model(n=6, E=8, L=1e6), P=6)
    dl, dmean = pf.terminal_branch_quantiles(model, seed=1, n_trees=30000)
    ol_, omean = oracle_lib.terminal_branch_quantiles(model, seed=1, n_trees=30000)
    assert (_bits(dl) == _bits(ol_)).all() and _bits([dmean])[0] == _bits([omean])[0]
    assert (np.diff(dl, axis=1) > 0).all()


def test_wide_site_simulator_says_where_it_stops(hiplib):
    from smcsmc_amd import pf
    model = cases.make_structured(cases.make_model(n=6, E=4, L=1e5), P=6)
    with pytest.raises(pf.PfError, match="site simulator takes at most four populations"):
        pf.simulate_sites(model, seed=1, nchunks=1)


@pytest.mark.parametrize("kw", [dict(), dict(mp_rows=True), dict(debug=FORCE_LDS), dict(record_trees=True, gen_cap=64, log_cap=64)],
                         ids=["plain", "mp-rows", "force-lds", "arg"])
@pytest.mark.parametrize("n,P", [(4, 5), (8, 8), (12, 6)])
def test_wide_handles_run_on_the_general_path(hiplib, n, P, kw):
    """no rings, the general kernels whatever the flags ask for, and pf_run_many refuses such handles by name"""
    from smcsmc_amd import ParticleFilter, PfError
    E = 4
    base = cases.make_model(n=n, E=E, L=2e5)
    segs = cases.make_segments(base, seed=40 + n, max_seg_len=2000)
    model = cases.make_structured(base, P=P, split_epoch=E - 1, mig=0.5)       # (a late join: faster migration overflows the event list, in the oracle too)
    fs = [ParticleFilter(model, 256, seed=5 + k, **kw) for k in range(2)]
    try:
        for f in fs:
            f.init_prior(0.0); f.load_segments(segs)
            assert f.run_path() == "General" and f.run_path(many=True) is None
        assert not ParticleFilter.can_run_many(fs) and not ParticleFilter.can_run_many(fs[:1])
        with pytest.raises(PfError, match="more than four populations"):
            ParticleFilter.run_many(fs)
    finally:
        for f in fs:
            f.close()


def test_wide_look_ahead_flags_leave_the_general_path(hiplib):
    """the PF_LA_ROW_PIPELINE* bits on a handle that does not qualify: general path, no error"""
    from smcsmc_amd import ParticleFilter, pf, segments as segmod
    n, P, E = 9, 5, 4
    base = cases.make_model(n=n, E=E, L=2e5)
    segs = cases.make_segments(base, seed=49, max_seg_len=2000)
    model = cases.make_structured(base, P=P, split_epoch=E - 1, mig=0.5)       # (a late join: faster migration overflows the event list, in the oracle too)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    la, tbl = segmod.pack_lookahead(rows, n), pf.terminal_branch_quantiles(model, seed=1, n_trees=2000)
    for flag in (dict(pipeline=True), dict(structured=True), dict(lds=True)):
        f = ParticleFilter(model, 256, seed=5, mp_rows=True)
        try:
            f.init_prior(0.0); f.load_segments(segs); f.load_lookahead(la, 2, tbl, **flag)
            assert f.run_path() == "General" and f.run_path(many=True) is None
        finally:
            f.close()


def test_wide_prior_recovers_model(hiplib):
    """No-data run: the posterior is the prior, so the counts must reproduce the model's rates -- per population, and per ordered pair
    of populations (assertions and margins of test_structured_prior_recovers_model; the oracle itself lands within 1 % here)."""
    from smcsmc_amd import ParticleFilter
    N0, P = 1e4, 6
    model = cases.make_structured(cases.make_model(n=6, E=8, L=2e6), P=P, split_epoch=5, mig=1.0)
    segs = cases.nodata_segments(model, 4000.0)
    g = ParticleFilter(model, 2048, seed=3); g.init_prior(0.0); g.load_segments(segs); g.run(); g.finish()
    c = g.counts()
    coal = c["coal_count"] / np.maximum(c["coal_opp"], 1e-300) * 2 * N0
    mig = c["mig_count"].sum(2) / np.maximum(c["mig_opp"], 1e-300) * 4 * N0
    ok = c["coal_count"] > 20
    assert ok.sum() >= 6
    assert np.abs(coal[ok] - 1).max() < 0.05
    okm = c["mig_count"].sum(2) > 5
    assert okm.sum() >= 4
    assert np.abs(mig[okm] / (P - 1) - 1).max() < 0.05                 # total emigration rate: mig to each of the P - 1 others
    pair = c["mig_count"] / np.maximum(c["mig_opp"], 1e-300)[:, :, None] * 4 * N0
    okp = c["mig_count"] > 20
    assert set(zip(*np.nonzero(okp.any(0)))) == {(a, b) for a in range(P) for b in range(P) if a != b}, "all 30 ordered pairs qualify"
    assert np.abs(pair[okp] - 1).max() < 0.05
    assert c["coal_count"][5:, 1:].sum() == 0 and c["mig_count"][5:].sum() == 0      # after the join
    assert abs(c["rec_count"].sum() / c["rec_opp"].sum() / 1e-8 - 1) < 0.02


def test_wide_binary_end_to_end(hiplib, tmp_path):
    """The drop-in binary with six populations on data of the project's own simulator: its .out equals, character for character, the table
    written from the same run through the python binding, carries Coal rows for every population and Migr rows for every ordered pair;
    -arg writes M lines with populations up to 5; calibrated default lags and -apf run."""
    from smcsmc_amd import ParticleFilter, outfile, segments as segmod, simulate
    binary = os.path.join(ROOT, "bin", "smcsmc")
    if not os.path.exists(binary):
        from smcsmc_amd import build
        build.build_all()
    L, n, P = 200000, 6, 6
    base = cases.make_model(n=n, E=3, L=L)
    seg = str(tmp_path / "six.seg")
    simulate.write_seg(seg, simulate.simulate_seg(n, L, 2.5e-8, 1e-8, base["change_times"], base["pop_sizes"], seed=11))
    core = ("-N0 10000 -t %g -r %g %d -I 6 1 1 1 1 1 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    for t in ("0.0", "0.1"):
        core += ["-eN", t, "1.0", "-eM", t, "5.0"]
    core += ["-eN", "0.5", "1.0", "-eM", "0.5", "0"]
    for k in range(2, P + 1):
        core += ["-ej", "0.5", str(k), "1"]
    common = ["-nsam", str(n), "-EM", "0", "-tmax", "4", "-seg", seg]
    r = subprocess.run([binary] + core + common + ["-Np", "300", "-lag", "50000", "-seed", "5", "-o", str(tmp_path / "run")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(tmp_path / "run.out").read()
    m = json.loads(subprocess.run([binary] + core + ["-nsam", str(n), "-tmax", "4", "-dumpmodel"], capture_output=True, text=True).stdout)
    E = len(m["change_times"])
    assert m["npop"] == P and m["sample_pops"] == list(range(P)) and E == 3
    mig = np.array(m["mig_rates"]).reshape(E, P, P); smig = np.array(m["single_mig"]).reshape(E, P, P)
    assert mig[0, 5, 0] == pytest.approx(1.0 / 4e4) and mig[2].sum() == 0 and (smig[2, 1:, 0] == 1.0).all() and smig[:2].sum() == 0
    model = dict(change_times=np.array(m["change_times"]), pop_sizes=np.array(m["pop_sizes"]), lags=np.full(E, 50000.0),
                 nsam=n, loci_length=float(L), mutation_rate=m["mutation_rate"], recombination_rate=m["recombination_rate"],
                 n_pops=P, mig_rates=mig, single_mig=smig, sample_pops=m["sample_pops"])
    S = segmod.Segments(seg, n, L, max_segment_length=int(2.0 / (m["recombination_rate"] * 4 * m["N0"])))
    segs = S.pack(model["lags"])
    g = ParticleFilter(model, 300, seed=5, max_trace_events=0)
    g.init_prior(segs["start"][0]); g.load_segments(segs); g.run(); g.finish()
    assert outfile.outfile_text(model, g.counts(), 300) == text
    data = outfile.parse_outfile(text, is_text=True)
    for a in range(P):
        assert (("Coal", 0, a, -1, -1), "Opp") in data
        for b in range(P):
            if a != b:
                assert (("Migr", 0, a, b, -1), "Count") in data and (("Migr", 1, a, b, -1), "Opp") in data
    assert data[(("Migr", 0, 5, 0, -1), "Count")] > 0
    assert data[(("Migr", 2, 5, 0, -1), "Count")] == 0                      # after the join
    # default (calibrated) lags and the look-ahead: the tools' kernels take the six populations too
    r = subprocess.run([binary] + core + common + ["-Np", "200", "-seed", "3", "-apf", "2", "-o", str(tmp_path / "cal")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Migr" in open(tmp_path / "cal.out").read() and "Terminal branch length quantiles" in r.stdout
    # -arg: R, C and M lines with their populations
    r = subprocess.run([binary] + core + common + ["-Np", "200", "-seed", "6", "-lag", "50000", "-arg", "-o", str(tmp_path / "arg")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw_lines = gzip.open(tmp_path / "arg.trees.gz", "rt").read().splitlines()
    trees_format.check_lines(raw_lines, nsam=n, npop=P)
    ms = [ln.split("\t") for ln in raw_lines if ln.startswith("M\t")]
    assert ms and max(int(f[4]) for f in ms) == P - 1
