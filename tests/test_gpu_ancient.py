"""Ancient samples (model key sample_times, pf_model.sample_times, -eI) on the device: structured models on the general path, the instances
of k_init_mp / k_extend_mp / k_calibrate_mp for sample times (PW + PF_ANC, pf_mp.hip) and k_count_anc.

  * target: the filter against tests/golden/mc_model_ancient.json, the brute-force Monte Carlo statement of the model in
    tests/mc_model_ancient.py, under the rules of tests/mc_model_check.py (combine / verdict, unchanged);
  * all times zero: the oracle's run of the model without times, bit for bit;
  * no internal node at or below an ancient leaf under it; the prior's rates from a run without data; the binary with -eI.

With a time above zero the device is held to the oracle bit for bit in tests/test_gpu_ancient_parity.py (the oracle takes sample times
since then; tests/test_oracle_ancient_cpu.py holds it to the same fixture and to the checks of this file, on the CPU).  The tests here
judge the device on its own, against the model and not against the oracle, and stay as they are.
"""
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import mc_model_check as mc
import oracle_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests/golden/mc_model_ancient.json")))["cases"]


@pytest.fixture
def ancient_gold():
    """the cases of this fixture under the rules of mc_model_check (device_check, combine and verdict read mc.GOLD), for one test: what was
    added is taken out again"""
    added = [k for k in GOLD if k not in mc.GOLD]
    mc.GOLD.update({k: GOLD[k] for k in added})
    try:
        yield GOLD
    finally:
        for k in added:
            mc.GOLD.pop(k, None)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- the target
@pytest.mark.parametrize("mode", ["is", "rs"])
@pytest.mark.parametrize("case", ["a3", "a4"])
def test_filter_targets_the_model_with_ancient_samples(hiplib, ancient_gold, case, mode):
    """log mean exp(logl) over the 32 seeds, and with resampling the exp(logl)-weighted counts, against the fixture: 4 combined standard
    errors, "no power" above 3 % (log p) or 6 % (a cell)"""
    assert max(GOLD[case]["model"]["sample_times"]) > 0
    res, logl = mc.device_check(case, mode)
    assert len(logl) == len(mc.SEEDS)


# ---------------------------------------------------------------- all times zero
ZERO = [(4, 2), (9, 2), (6, 6)]


@functools.lru_cache(maxsize=None)
def _zero_inputs(n, P):
    E = 6
    base = cases.make_model(n=n, E=E, L=6e4)
    segs = cases.make_segments(base, seed=10 + n, max_seg_len=5000)
    return cases.make_structured(base, P=P, split_epoch=E - 2, mig=1.0), segs


@functools.lru_cache(maxsize=None)
def _zero_oracle(n, P, Np, seed):
    model, segs = _zero_inputs(n, P)
    o = oracle_lib.Oracle(model, Np, ess_fraction=0.5, seed=seed, max_trace_events=64)
    o.init_prior(segs["start"][0])
    o.run(o.pack_segments(model, segs))
    return dict(trace=o.trace(), events=o.resample_events(), particles=o.particles(), migrations=o.migrations(), counts=o.counts(), logl=o.logl())


@pytest.mark.parametrize("n,P", ZERO)
def test_zero_times_are_the_model_without_times(hiplib, n, P):
    from smcsmc_amd import ParticleFilter
    Np, seed = 256, 4
    model, segs = _zero_inputs(n, P)
    ref = _zero_oracle(n, P, Np, seed)
    g = ParticleFilter(dict(model, sample_times=[0.0] * n), Np, ess_fraction=0.5, seed=seed, max_trace_events=64)
    try:
        g.init_prior(segs["start"][0]); g.load_segments(segs)
        assert g.run_path() == "General" and g.run_path(many=True) is None
        g.run(); g.finish()
        assert ref["trace"]["resampled"].sum() > 0, "the case must exercise resampling"
        assert _bits([g.logl()])[0] == _bits([ref["logl"]])[0]
        to, tg = ref["trace"], g.trace()
        assert (to["resampled"] == tg["resampled"]).all()
        for k in ("T", "ess", "logl"):
            assert (_bits(to[k]) == _bits(tg[k])).all(), k
        so, po = ref["events"]; sg, pg = g.resample_events()
        assert (so == sg).all() and (po == pg).all()
        qo, qg = ref["particles"], g.particles()
        assert (qo["children"] == qg["children"]).all()
        for k in ("heights", "w_post", "w_pilot", "next_base"):
            assert (_bits(qo[k]) == _bits(qg[k])).all(), k
        mo, mg = ref["migrations"], g.migrations()
        assert (mo["n_events"] == mg["n_events"]).all() and (mo["node_pops"] == mg["node_pops"]).all()
        co, cg = ref["counts"], g.counts()
        for k in ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight", "mig_count", "mig_opp", "mig_weight"):
            np.testing.assert_allclose(cg[k], co[k], rtol=1e-9, atol=1e-300, err_msg=k)
    finally:
        g.close()


def test_zero_times_calibrate_the_same_lags(hiplib):
    from smcsmc_amd import pf
    model = cases.make_structured(cases.make_model(n=6, E=8, L=1e7), P=2, split_epoch=5)
    a, ta = pf.median_survival(model, seed=1, min_events=50, max_trees=32768)
    b, tb = pf.median_survival(dict(model, sample_times=[0.0] * 6), seed=1, min_events=50, max_trees=32768)
    assert ta == tb and (_bits(a) == _bits(b)).all()


# ---------------------------------------------------------------- what a handle with sample times refuses
def test_handle_refuses_look_ahead_and_lockstep(hiplib):
    from smcsmc_amd import ParticleFilter, PfError, pf, segments as segmod
    n, P = 4, 2
    model, segs = _zero_inputs(n, P)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a))) for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    la, tbl = segmod.pack_lookahead(rows, n), pf.terminal_branch_quantiles(model, seed=1, n_trees=2000)
    fs = [ParticleFilter(dict(model, sample_times=[0.0, 0.0, 0.0, float(model["change_times"][2])]), 256, seed=5 + k) for k in range(2)]
    try:
        for f in fs:
            f.init_prior(0.0); f.load_segments(segs)
            assert f.run_path() == "General" and f.run_path(many=True) is None
        assert not ParticleFilter.can_run_many(fs) and not ParticleFilter.can_run_many(fs[:1])
        with pytest.raises(PfError, match=r"pf_run_many: a model with sample times \(-eI, ancient samples\) runs on the general kernels"):
            ParticleFilter.run_many(fs)
        with pytest.raises(PfError, match="pf_load_lookahead: .* is not supported with sample times"):
            fs[0].load_lookahead(la, 2, tbl)
    finally:
        for f in fs:
            f.close()


# ---------------------------------------------------------------- no node at or below an ancient leaf
def _ancient_model(n, L, times_epoch=2):
    """N = 10 000 throughout; epochs at 0, 2 000, 20 000, 60 000 generations; two populations that join at the last epoch start; the later half
    of the samples enters at change_times[times_epoch]"""
    m = cases.make_model(n=n, E=4, L=L, lag=1e9)
    m["change_times"] = np.array([0.0, 2000.0, 20000.0, 60000.0])
    m = cases.make_structured(m, P=2, split_epoch=3, mig=1.0, sample_pops=[i % 2 for i in range(n)])
    m["sample_times"] = [0.0] * (n - n // 2) + [float(m["change_times"][times_epoch])] * (n // 2)
    return m


def test_no_node_at_or_below_an_ancient_leaf(hiplib):
    """three of six samples enter at 20 000 generations, where the prior of present-day samples would often have coalesced them already"""
    from smcsmc_amd import ParticleFilter
    n, S = 6, 12
    model = _ancient_model(n, 12000.0)
    rng = np.random.default_rng(3)
    al = rng.integers(0, 2, size=(S, n)).astype(np.int8)
    al[::3] = np.array([0, 0, 1, 0, 1, 1], np.int8)          # (some sites that split old from new)
    segs = dict(start=np.arange(S) * 1000.0, length=np.full(S, 1000.0), state=np.zeros(S, np.int8), alleles=al,
                max_record_epoch=np.full(S, 3, np.int32))
    g = ParticleFilter(model, 512, ess_fraction=0.5, seed=2, max_trace_events=0)
    try:
        g.init_prior(0.0); g.load_segments(segs); g.run(); g.finish()       # (an error code of any particle stops the run with its message)
        p = g.particles()
        assert g.trace()["resampled"].sum() > 0
        H, Ch = p["heights"], p["children"].astype(int)
        tau = np.array(model["sample_times"])
        assert (np.diff(H, axis=1) >= 0).all()
        oldest = np.zeros((len(H), 2 * n - 1))                  # the largest sample time below every node
        oldest[:, :n] = tau[None, :]
        for r in range(n - 1):
            c0, c1 = Ch[:, r, 0], Ch[:, r, 1]
            assert ((c0 < n + r) & (c1 < n + r)).all()
            idx = np.arange(len(H))
            oldest[:, n + r] = np.maximum(oldest[idx, c0], oldest[idx, c1])
        assert (H > oldest[:, n:]).all(), "an internal node at or below an ancient leaf under it"
        assert (H[:, -1] > tau.max()).all() and (H.min(axis=1) < tau.max()).any()      # (and nodes among the present-day samples below that time do exist)
        assert np.isfinite(g.logl())
    finally:
        g.close()


# ---------------------------------------------------------------- the prior
def test_prior_recovers_the_model_with_ancient_samples(hiplib):
    """No-data run: the posterior is the prior, so the counts must reproduce the model's rates (margins and count floors of
    test_wide_prior_recovers_model) -- coalescence and emigration per qualifying epoch and population, and recombinations per unit of
    opportunity per epoch: an opportunity that counted the length of samples that have not entered yet would put the young epochs off"""
    from smcsmc_amd import ParticleFilter
    N0, P, n, rho = 1e4, 2, 6, 1e-8
    model = _ancient_model(n, 2e6, times_epoch=1)
    model["lags"] = 4.0 / (rho * np.array([2000.0, 20000.0, 60000.0, 60000.0]))      # (the default lags of cases.make_model for these epochs)
    segs = cases.nodata_segments(model, 4000.0)
    g = ParticleFilter(model, 2048, seed=3)
    try:
        g.init_prior(0.0); g.load_segments(segs); g.run(); g.finish()
        c = g.counts()
    finally:
        g.close()
    coal = c["coal_count"] / np.maximum(c["coal_opp"], 1e-300) * 2 * N0
    mig = c["mig_count"].sum(2) / np.maximum(c["mig_opp"], 1e-300) * 4 * N0
    rec = c["rec_count"] / np.maximum(c["rec_opp"], 1e-300) / rho
    print("coal", coal, c["coal_count"]); print("mig", mig, c["mig_count"].sum(2)); print("rec", rec, c["rec_count"])
    ok = c["coal_count"] > 20
    assert ok.sum() >= 5
    assert np.abs(coal[ok] - 1).max() < 0.05
    okm = c["mig_count"].sum(2) > 20
    assert okm[1:3].all()                                                      # both populations in the two long epochs before the join
    assert np.abs(mig[okm] / (P - 1) - 1).max() < 0.05
    assert c["coal_count"][3, 1] == 0 and c["mig_count"][3].sum() == 0       # after the join
    okr = c["rec_count"] > 20
    assert okr.all()
    assert np.abs(rec[okr] - 1).max() < 0.05
    assert abs(c["rec_count"].sum() / c["rec_opp"].sum() / rho - 1) < 0.02


# ---------------------------------------------------------------- the binary
def test_binary_end_to_end_with_ancient_samples(hiplib, tmp_path):
    """bin/smcsmc -I 2 2 1 -eI t 0 1 on the rows of a fixture case: its .out equals, character for character, the table written from the same
    run through the binding; calibrated default lags run and are finite"""
    from smcsmc_amd import ParticleFilter, outfile, segments as segmod, simulate
    binary = os.path.join(ROOT, "bin", "smcsmc")
    if not os.path.exists(binary):
        from smcsmc_amd import build
        build.build_all()
    import make_mc_model_ancient as mka
    import mc_model_ancient as mca
    g4 = GOLD["a4"]
    L, n, P, N0 = int(g4["model"]["loci_length"]), 4, 2, 10000.0
    # the sites of the fixture's case (its data seed) as a .seg file; the columns are in the order -I, then -eI, as the fixture has them
    pos, pat = mca.simulate_sites(mka.case_model(mka.CASES["a4"]), mka.CASES["a4"]["data_seed"])
    seg = str(tmp_path / "a4.seg")
    simulate.write_seg(seg, simulate.sites_to_seg(pos, pat, n, L))
    t_anc = 2000.0 / (4 * N0)
    core = ("-N0 10000 -t %.17g -r %.17g %d -I 2 1 1 -eI %.17g 1 1" % (4 * N0 * g4["model"]["mutation_rate"] * L,
            4 * N0 * g4["model"]["recombination_rate"] * (L - 1), L, t_anc)).split()
    core += ["-eN", "0", "1.0", "-en", "0", "2", "0.5", "-em", "0", "1", "2", "4.0",
             "-eN", "%.17g" % t_anc, "0.4", "-en", "%.17g" % t_anc, "2", "0.2",
             "-eN", "0.5", "2.5", "-ej", "0.5", "2", "1"]
    common = ["-nsam", str(n), "-EM", "0", "-tmax", "4", "-seg", seg]
    m = json.loads(subprocess.run([binary] + core + ["-nsam", str(n), "-tmax", "4", "-dumpmodel"], capture_output=True, text=True).stdout)
    E = len(m["change_times"])
    assert E == 3 and m["change_times"] == [0, 2000, 20000] and m["sample_pops"] == [0, 1, 0, 1] and m["sample_times"] == [0, 0, 2000, 2000]
    r = subprocess.run([binary] + core + common + ["-Np", "300", "-lag", "50000", "-seed", "5", "-o", str(tmp_path / "run")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(tmp_path / "run.out").read()
    mig = np.array(m["mig_rates"]).reshape(E, P, P); smig = np.array(m["single_mig"]).reshape(E, P, P)
    assert mig[0, 0, 1] == pytest.approx(1e-4) and mig[0, 1, 0] == 0 and mig[2].sum() == 0 and smig[2, 1, 0] == 1.0
    model = dict(change_times=np.array(m["change_times"], float), pop_sizes=np.array(m["pop_sizes"]), lags=np.full(E, 50000.0),
                 nsam=n, loci_length=float(L), mutation_rate=m["mutation_rate"], recombination_rate=m["recombination_rate"],
                 n_pops=P, mig_rates=mig, single_mig=smig, sample_pops=m["sample_pops"], sample_times=m["sample_times"])
    S = segmod.Segments(seg, n, L, max_segment_length=int(2.0 / (m["recombination_rate"] * 4 * m["N0"])))
    segs = S.pack(model["lags"])
    f = ParticleFilter(model, 300, seed=5, max_trace_events=0)
    try:
        f.init_prior(segs["start"][0]); f.load_segments(segs); f.run(); f.finish()
        assert outfile.outfile_text(model, f.counts(), 300) == text
    finally:
        f.close()
    # default (calibrated) lags: k_calibrate_mp<PF_PMAX + PF_ANC>
    r = subprocess.run([binary] + core + common + ["-Np", "200", "-seed", "3", "-o", str(tmp_path / "cal")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = outfile.parse_outfile(open(tmp_path / "cal.out").read(), is_text=True)
    assert all(np.isfinite(v) for v in data.values()) and (("Coal", 1, 1, -1, -1), "Opp") in data
    # -chunks: the chunks of a structured model are filtered one after the other, and with -eI the note says that lockstep is not to be had
    r = subprocess.run([binary] + core + common + ["-Np", "200", "-lag", "50000", "-seed", "3", "-chunks", "2", "-ranks", "1", "-o", str(tmp_path / "ch")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("1 chunk(s) ran one after the other (chunks in lockstep are not supported with ancient samples, -eI)") == 2, r.stderr
    data = outfile.parse_outfile(open(tmp_path / "ch.out").read(), is_text=True)
    assert all(np.isfinite(v) for v in data.values()) and (("Coal", 1, 1, -1, -1), "Opp") in data
    # what the binary refuses with -eI, by name
    for extra, what in ((["-arg"], "-arg with ancient samples"), (["-apf", "2"], "-apf with ancient samples"), (["-mp_rows"], "-mp_rows .* with ancient samples"),
                        (["-bias_heights", "400", "-bias_strengths", "5", "1"], "-bias_heights with ancient samples")):
        r = subprocess.run([binary] + core + common + extra + ["-Np", "100", "-o", str(tmp_path / "no")], capture_output=True, text=True)
        assert r.returncode != 0 and re.search(what, r.stderr + r.stdout), (extra, r.stderr)
