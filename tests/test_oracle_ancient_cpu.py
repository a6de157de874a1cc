"""Sample times (ancient samples, model key sample_times) in the CPU oracle, judged without any device code.

The device with a time above zero is held to this oracle bit for bit (tests/test_gpu_ancient_parity.py), so the oracle has to earn that
first:
  (1) all-zero times are the model without times, bit for bit -- and the recorded fingerprints (tests/test_oracle_wide_cpu.py) pass unchanged;
  (2) the oracle meets tests/golden/mc_model_ancient.json, made by the independent Monte Carlo statement of the model
      (tests/mc_model_ancient.py), under the unchanged rules of tests/mc_model_check.py: this, not the device, licenses it as a reference;
  (3) no internal node at or below an ancient leaf under it; a run without data recovers the model's rates;
  (4) every parity case of tests/ancient_cases.py is not degenerate: it resamples, the times move log-likelihood and recombination
      opportunity, and the edge it is there for occurs in a positive number of first trees;
  (5) what the device path refuses with sample times, the oracle refuses."""
import json
import multiprocessing as mp
import os

import numpy as np
import pytest

import ancient_cases as ac
import cases
import mc_model_check as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests/golden/mc_model_ancient.json")))["cases"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- 1. all times zero
def _sweep(oracle, model, segs, Np, seed):
    o = oracle.Oracle(model, Np, ess_fraction=0.5, seed=seed, max_trace_events=64)
    o.init_prior(segs["start"][0])
    o.run(o.pack_segments(model, segs))
    r = dict(trace=o.trace(), events=o.resample_events(), particles=o.particles(), migrations=o.migrations(), counts=o.counts(), logl=o.logl())
    o.close()
    return r


@pytest.mark.parametrize("n,P", [(4, 2), (9, 2), (6, 6)])
def test_zero_times_are_the_model_without_times(oracle, n, P):
    """trace, particles, migration lists, counts and the calibrated lags, every bit"""
    E = 6
    base = cases.make_model(n=n, E=E, L=6e4)
    segs = cases.make_segments(base, seed=10 + n, max_seg_len=5000)
    model = cases.make_structured(base, P=P, split_epoch=E - 2, mig=1.0)
    a, b = _sweep(oracle, model, segs, 256, 4), _sweep(oracle, dict(model, sample_times=[0.0] * n), segs, 256, 4)
    assert a["trace"]["resampled"].sum() > 0
    assert _bits([a["logl"]])[0] == _bits([b["logl"]])[0]
    assert (a["trace"]["resampled"] == b["trace"]["resampled"]).all()
    for k in ("T", "ess", "logl"):
        assert (_bits(a["trace"][k]) == _bits(b["trace"][k])).all(), k
    assert (a["events"][0] == b["events"][0]).all() and (a["events"][1] == b["events"][1]).all()
    assert (a["particles"]["children"] == b["particles"]["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(a["particles"][k]) == _bits(b["particles"][k])).all(), k
    for k in ("n_events", "branch", "newpop", "node_pops"):
        assert (a["migrations"][k] == b["migrations"][k]).all(), k
    assert (_bits(a["migrations"]["times"]) == _bits(b["migrations"]["times"])).all()
    for k in a["counts"]:
        assert (_bits(a["counts"][k]) == _bits(b["counts"][k])).all(), k
    cal = dict(model, loci_length=1e6)
    ma, ta = oracle.median_survival(cal, seed=1, min_events=30, max_trees=16384)
    mb, tb = oracle.median_survival(dict(cal, sample_times=[0.0] * n), seed=1, min_events=30, max_trees=16384)
    assert ta == tb and (_bits(ma) == _bits(mb)).all()


# ---------------------------------------------------------------- 2. the target
@pytest.fixture(scope="module")
def ancient_pool(oracle):
    """the cases of the fixture under the rules of mc_model_check, in this process and in the workers (forked after the cases are in);
    what was added is taken out again"""
    added = [k for k in GOLD if k not in mc.GOLD]
    mc.GOLD.update({k: GOLD[k] for k in added})
    try:
        with mp.Pool(4) as p:
            yield p
    finally:
        for k in added:
            mc.GOLD.pop(k, None)
        mc.inputs.cache_clear()


@pytest.mark.parametrize("mode", ["is", "rs"])
@pytest.mark.parametrize("case", ["a3", "a4"])
def test_the_oracle_targets_the_model_with_ancient_samples(ancient_pool, case, mode):
    """32 seeds: log mean exp(logl), and with resampling the exp(logl)-weighted counts, against the fixture: 4 combined standard errors,
    "no power" above 3 % (log p) or 6 % (a cell)"""
    assert max(GOLD[case]["model"]["sample_times"]) > 0
    assert mc.inputs(case)[0]["sample_times"] == GOLD[case]["model"]["sample_times"]
    mc.oracle_check(ancient_pool, case, mode)


# ---------------------------------------------------------------- 3. the trees and the prior
def _ancient_model(n, L, times_epoch=2):
    """the model of test_gpu_ancient.py: N = 10 000 throughout; epochs at 0, 2 000, 20 000, 60 000 generations; two populations that join at
    the last epoch start; the later half of the samples enters at change_times[times_epoch]"""
    m = cases.make_model(n=n, E=4, L=L, lag=1e9)
    m["change_times"] = np.array([0.0, 2000.0, 20000.0, 60000.0])
    m = cases.make_structured(m, P=2, split_epoch=3, mig=1.0, sample_pops=[i % 2 for i in range(n)])
    m["sample_times"] = [0.0] * (n - n // 2) + [float(m["change_times"][times_epoch])] * (n // 2)
    return m


def test_no_node_at_or_below_an_ancient_leaf(oracle):
    """three of six samples enter at 20 000 generations, where the prior of present-day samples would often have coalesced them already"""
    n, S = 6, 12
    model = _ancient_model(n, 12000.0)
    rng = np.random.default_rng(3)
    al = rng.integers(0, 2, size=(S, n)).astype(np.int8)
    al[::3] = np.array([0, 0, 1, 0, 1, 1], np.int8)
    segs = dict(start=np.arange(S) * 1000.0, length=np.full(S, 1000.0), state=np.zeros(S, np.int8), alleles=al,
                max_record_epoch=np.full(S, 3, np.int32))
    r = _sweep(oracle, model, segs, 512, 2)
    assert r["trace"]["resampled"].sum() > 0
    H, Ch = r["particles"]["heights"], r["particles"]["children"].astype(int)
    tau = np.array(model["sample_times"])
    assert (np.diff(H, axis=1) >= 0).all()
    oldest = np.zeros((len(H), 2 * n - 1))                  # the largest sample time below every node
    oldest[:, :n] = tau[None, :]
    idx = np.arange(len(H))
    for k in range(n - 1):
        c0, c1 = Ch[:, k, 0], Ch[:, k, 1]
        assert ((c0 < n + k) & (c1 < n + k)).all()
        oldest[:, n + k] = np.maximum(oldest[idx, c0], oldest[idx, c1])
    assert (H > oldest[:, n:]).all(), "an internal node at or below an ancient leaf under it"
    assert (H[:, -1] > tau.max()).all() and (H.min(axis=1) < tau.max()).any()
    assert np.isfinite(r["logl"])


def test_prior_recovers_the_model_with_ancient_samples(oracle):
    """No-data run: the posterior is the prior, so the counts must reproduce the model's rates (margins and count floors of
    test_gpu_ancient.py::test_prior_recovers_the_model_with_ancient_samples).  L = 1e6 and 256 particles hold the floors here in six
    seconds (smallest qualifying counts: 235 coalescences, 58 migrations, 59 recombinations); the oracle's rectangles carry the lineages
    present, so a miscounted interval puts the young epochs' rate off."""
    N0, P, n, rho = 1e4, 2, 6, 1e-8
    model = _ancient_model(n, 1e6, times_epoch=1)
    model["lags"] = 4.0 / (rho * np.array([2000.0, 20000.0, 60000.0, 60000.0]))
    segs = cases.nodata_segments(model, 4000.0)
    o = oracle.Oracle(model, 256, seed=3, max_trace_events=0)
    o.init_prior(0.0); o.run(o.pack_segments(model, segs))
    c = o.counts(); o.close()
    coal = c["coal_count"] / np.maximum(c["coal_opp"], 1e-300) * 2 * N0
    mig = c["mig_count"].sum(2) / np.maximum(c["mig_opp"], 1e-300) * 4 * N0
    rec = c["rec_count"] / np.maximum(c["rec_opp"], 1e-300) / rho
    print("coal", coal, c["coal_count"]); print("mig", mig, c["mig_count"].sum(2)); print("rec", rec, c["rec_count"])
    ok = c["coal_count"] > 20
    assert ok.sum() >= 5
    assert np.abs(coal[ok] - 1).max() < 0.05
    okm = c["mig_count"].sum(2) > 20
    assert okm[1:3].all()
    assert np.abs(mig[okm] / (P - 1) - 1).max() < 0.05
    assert c["coal_count"][3, 1] == 0 and c["mig_count"][3].sum() == 0       # after the join
    okr = c["rec_count"] > 20
    assert okr.all()
    assert np.abs(rec[okr] - 1).max() < 0.05
    assert abs(c["rec_count"].sum() / c["rec_opp"].sum() / rho - 1) < 0.02


# ---------------------------------------------------------------- 4. the parity cases are not degenerate
@pytest.mark.parametrize("case_id", ac.IDS)
def test_parity_case_is_not_degenerate(oracle, case_id):
    c = ac.by_id(case_id)
    model, segs = ac.inputs(case_id)
    assert max(model["sample_times"]) > 0 and 6e4 <= c["L"] <= 1e5 and 192 <= c["Np"] <= 300
    r, z = ac.oracle_run(case_id), ac.oracle_run(case_id, zero=True)
    assert r["trace"]["resampled"].sum() >= 1
    assert _bits([r["logl"]])[0] != _bits([z["logl"]])[0]
    assert not np.array_equal(r["counts"]["rec_opp"], z["counts"]["rec_opp"])
    what, cnt, Np = ac.edge_measure(case_id)
    print("%s: %d resamplings in %d rows; %s: %d of %d" % (case_id, r["trace"]["resampled"].sum(), len(segs["start"]), what, cnt, Np))
    assert cnt > 0, what


@pytest.mark.parametrize("case_id", ac.VARIANT_CASES)
@pytest.mark.parametrize("variant", ["missing-unphased", "vb", "local_map"])
def test_variant_does_what_it_is_for(oracle, case_id, variant):
    model, segs = ac.inputs(case_id, variant)
    r, plain = ac.oracle_run(case_id, variant), ac.oracle_run(case_id)
    assert r["trace"]["resampled"].sum() >= 1
    if variant == "missing-unphased":
        al = np.asarray(segs["alleles"]).reshape(len(segs["start"]), -1)
        data = (al[:, 0] != -1)                    # (rows that are missing altogether aside)
        assert (al == 2).any() and (al[data][:, -2:] == -1).any() and not (al[data][:, :-2] == -1).any()
        assert _bits([r["logl"]])[0] != _bits([plain["logl"]])[0]
    if variant == "vb":
        assert _bits([r["logl"]])[0] != _bits([plain["logl"]])[0]
    if variant == "local_map":
        lm = r["local_recomb"]
        assert lm["counts"][:model["nsam"]].sum() > 0 and np.abs(lm["opp_diff"]).sum() > 0
        assert _bits([r["logl"]])[0] == _bits([plain["logl"]])[0]


@pytest.mark.parametrize("P", ac.CALIBRATION_POPS)
def test_calibration_case_is_moved_by_its_times(oracle, P):
    """the lag calibration that test_calibration_parity compares: one batch of trees, and not the medians of the model without times"""
    model = ac.calibration_model(P)
    om, ot = oracle.median_survival(model, seed=1, min_events=50, max_trees=16384)
    zm, zt = oracle.median_survival(ac.without_times(model), seed=1, min_events=50, max_trees=16384)
    assert ot == zt == 16384 and (om > 0).all()
    assert (_bits(om) != _bits(zm)).all()


# ---------------------------------------------------------------- 5. refusals
def _times_model(n=4, P=2, **kw):
    m = cases.make_structured(cases.make_model(n=n, E=6, L=6e4), P=P, split_epoch=4) if P > 1 else cases.make_model(n=n, E=6, L=6e4)
    ct = m["change_times"]
    m["sample_times"] = [0.0] * (n - 1) + [float(ct[2])]
    m.update(kw)
    return m


def _refused(oracle, model, match, **kw):
    with pytest.raises(RuntimeError, match=match):
        oracle.Oracle(model, 64, **kw)


def test_oracle_refuses_what_the_device_refuses(oracle):
    ct = _times_model()["change_times"]
    _refused(oracle, _times_model(P=1), "need a structured model")
    _refused(oracle, _times_model(sample_times=[0.0, 0.0, 0.0, 0.5 * (ct[1] + ct[2])]), "sample time .* of sample 3 is not an entry of change_times")
    _refused(oracle, _times_model(sample_times=[0.0, float(ct[2]), float(ct[1]), float(ct[2])]), "must ascend with the sample index")
    _refused(oracle, _times_model(sample_times=[float(ct[1])] * 4), "smallest sample time must be 0")
    _refused(oracle, _times_model(bias_heights=[400.0], bias_strengths=[5.0, 1.0], application_delays=np.full(6, 1000.0)),
             "focused sampling .* is not supported with sample times")
    m = _times_model()
    _refused(oracle, dict(m, guide=cases.guide(m, 3, 2.0, 7), application_delays=np.full(6, 1000.0)), "recombination guide is not supported with sample times")
    o = oracle.Oracle(m, 64)
    with pytest.raises(RuntimeError, match=r"tree recording \(-arg\) is not supported with sample times"):
        o.enable_tree_recording()
    from smcsmc_amd import segments as segmod
    plain = {k: v for k, v in m.items() if k != "sample_times"}
    segs = cases.make_segments(cases.make_model(n=4, E=6, L=6e4), seed=3, max_seg_len=5000)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a))) for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    with pytest.raises(RuntimeError, match=r"look-ahead \(-apf\) is not supported with sample times"):
        o.load_lookahead(segmod.pack_lookahead(rows, 4), 2, oracle.terminal_branch_quantiles(plain, seed=1, n_trees=2000))
    o.close()
    with pytest.raises(RuntimeError, match="terminal branch quantiles are not supported with sample times"):
        oracle.terminal_branch_quantiles(m, seed=1, n_trees=100)
    for bad, match in ((dict(m, n_pops=1, pop_sizes=np.asarray(m["pop_sizes"])[:, 0], mig_rates=None, single_mig=None, sample_pops=None), "need a structured model"),
                       (dict(m, sample_times=[0.0, 0.0, 0.0, 1.0]), "is not an entry of change_times"),
                       (dict(m, sample_times=[float(ct[1])] * 4), "smallest sample time must be 0")):
        with pytest.raises(RuntimeError, match=match):
            oracle.median_survival(bad, seed=1, min_events=5, max_trees=16384)
