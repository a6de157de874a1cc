"""More than 16 haplotypes with one population: the wide kernels (pf_wide.hip: one wavefront per workgroup, 64-bit masks, the
records' extra descendant word, k_count<64, 1>), held to the CPU oracle bit for bit where they are wide.

(1) PF_DEBUG_FORCE_WIDE runs the wide kernels at n = 9, 12, 16 against the oracle and against the 256-lane kernels.
(1b) Without the switch, at n = 17, 24, 32, 33, 48, 63, 64 (tests/wide_cases.py: plain, biased with delays, local map, unphased
    with a missing block, recombination guide, odd n, the unphased pair (62, 63), 32 epochs with a partly filled last wavefront):
    log-likelihood, trace, resampling slots and parents, final particles bit for bit, the six count arrays within 1e-9, the local
    map's per-sample rows at n = 32, 33 and 64.  Lag calibration, the step API, rows without data and rows past the end at
    n = 40, a re-initialised handle at n = 32: against the oracle as well.  The oracle itself is judged at these sizes, without
    a device, in tests/test_oracle_wide_cpu.py.
(2..6) What the model implies, independent of the oracle: Kingman's coalescent for the prior, the site likelihood restated in
    numpy, the frequency spectrum of the simulator; and the binary runs.

Sizes (Np, sequence length): forced-wide parity 300 / 256 / 200 particles over 120 kb; wide parity 100..300 particles over
12..100 kb and 1000 particles over 40 kb at 32 epochs (tests/wide_cases.py); calibration one batch of 16384 trees over 300 kb at
n = 40; prior 4096 particles over 100 kb at n = 32 and 64; local map 1024 particles over 60 kb at n = 64; emission 512 particles,
one site; simulator 4 chunks of 3 Mb at n = 32; binary 300 particles over 200 kb at n = 32; two sweeps 256 particles over 100 kb
at n = 12 and 32."""
import gzip
import os
import subprocess
import time

import numpy as np
import pytest

import cases
import wide_cases
from smcsmc_amd import ParticleFilter, pf, simulate

pytestmark = pytest.mark.gpu
FORCE_WIDE = pf.DEBUG_FORCE_WIDE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_KEYS = ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _sweep(model, segs, Np, seed, **kw):
    g = ParticleFilter(model, Np, seed=seed, max_trace_events=64, **kw)
    g.init_prior(segs["start"][0]); g.load_segments(segs); g.run(); g.finish()
    return g


def _same_run(a, b, counts_rtol=None, counts_a=None):
    """log-likelihood, traces, resampling and particles bit for bit; the counts bit for bit or within counts_rtol (counts_a:
    what to take for a's counts instead of a.counts())"""
    assert _bits([a.logl()])[0] == _bits([b.logl()])[0]
    ta, tb = a.trace(), b.trace()
    assert len(ta["T"]) == len(tb["T"])
    for k in ("T", "ess", "logl"):
        assert (_bits(ta[k]) == _bits(tb[k])).all(), k
    assert (ta["resampled"] == tb["resampled"]).all()
    sa, pa = a.resample_events(); sb, pb = b.resample_events()
    assert (sa == sb).all() and (pa == pb).all()
    wa, wb = a.particles(), b.particles()
    assert (wa["children"] == wb["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(wa[k]) == _bits(wb[k])).all(), k
    ca, cb = (a.counts() if counts_a is None else counts_a), b.counts()
    for k in COUNT_KEYS:
        if counts_rtol is None:
            assert (_bits(ca[k]) == _bits(cb[k])).all(), k
        else:
            np.testing.assert_allclose(ca[k], cb[k], rtol=counts_rtol, atol=1e-300, err_msg=k)
    assert ca["resample_count"] == cb["resample_count"]


def _device_equals_oracle(o, g, model, local_map=False, min_resampling=1):
    """log-likelihood, trace, resampled flags, resampling slots and parents, final particles bit for bit; the six count arrays at
    rtol 1e-9 (the project's bound for the lagged sums); with local_map the 100-bp map, every per-sample row compared"""
    n = model["nsam"]
    assert _bits([o.logl()])[0] == _bits([g.logl()])[0]
    to, tg = o.trace(), g.trace()
    assert len(to["T"]) == len(tg["T"])
    for k in ("T", "ess", "logl"):
        assert (_bits(to[k]) == _bits(tg[k])).all(), k
    assert (to["resampled"] == tg["resampled"]).all() and to["resampled"].sum() >= min_resampling
    so, po = o.resample_events(); sg, pg = g.resample_events()
    assert (so == sg).all() and (po == pg).all()
    wo, wg = o.particles(), g.particles()
    assert (wo["children"] == wg["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(wo[k]) == _bits(wg[k])).all(), k
    co, cg = o.counts(), g.counts()
    for k in COUNT_KEYS:
        np.testing.assert_allclose(cg[k], co[k], rtol=1e-9, atol=1e-300, err_msg=k)
    assert cg["resample_count"] == co["resample_count"]
    if local_map:
        lo, lg = o.local_recomb(model["loci_length"]), g.local_recomb()
        cum_o, cum_g = np.cumsum(lo["opp_diff"]), np.cumsum(lg["opp_diff"])
        np.testing.assert_allclose(cum_g, cum_o, rtol=1e-7, atol=1e-7 * cum_o.max())
        assert lo["counts"][:n].sum() > 0
        assert lg["counts"].shape == lo["counts"].shape == (n + 2, len(lo["opp_diff"]))
        np.testing.assert_allclose(lg["counts"], lo["counts"], rtol=1e-9, atol=1e-12 * max(1.0, lo["counts"].max()))
        assert lg["counts"][:n].sum() == pytest.approx(cg["rec_count"].sum(), rel=1e-9)


# ---------------------------------------------------------------- 1. the wide path against the oracle at n <= 16
@pytest.mark.parametrize("n,Np,kind", [(9, 300, "local_recomb"), (12, 256, "biased"), (16, 200, "plain")])
def test_force_wide_equals_oracle(oracle, hiplib, n, Np, kind):
    model = cases.make_model(n=n, E=8, L=1.2e5)
    if kind == "biased":
        model.update(bias_heights=[400.0], bias_strengths=[3.0, 1.0], delay_type=0, application_delays=np.full(8, 3000.0))
    segs = cases.make_segments(model, seed=50 + n, max_seg_len=5000)
    o = oracle.Oracle(model, Np, seed=n, max_trace_events=64)
    if kind == "local_recomb":
        o.enable_local_recomb()
    o.init_prior(segs["start"][0])
    o.run(o.pack_segments(model, segs))
    g = _sweep(model, segs, Np, n, debug=FORCE_WIDE, local_recomb=kind == "local_recomb")
    _device_equals_oracle(o, g, model, local_map=kind == "local_recomb")


def test_force_wide_equals_default_path_at_12(hiplib):
    """the wide kernels and the 256-lane LDS-tree kernel (k_extend, k_count<16>) compute the same run at n = 12"""
    model = cases.make_model(n=12, E=8, L=1.2e5)
    segs = cases.make_segments(model, seed=7, max_seg_len=5000)
    _same_run(_sweep(model, segs, 256, 3, debug=FORCE_WIDE), _sweep(model, segs, 256, 3), counts_rtol=1e-12)


def test_wide_calibration_equals_oracle(oracle, hiplib):
    """lag calibration (calculate_median_survival_distances) on the wide kernel at n = 12: the oracle's medians, bit for bit"""
    model = cases.make_model(n=12, E=8, L=5e6)
    dm, dt = pf.median_survival(model, seed=1, min_events=50, max_trees=32768, debug=FORCE_WIDE)
    om, ot = oracle.median_survival(model, seed=1, min_events=50, max_trees=32768)
    assert dt == ot
    assert (_bits(dm) == _bits(om)).all()


# ---------------------------------------------------------------- 1b. the wide path against the oracle where it is wide
@pytest.mark.parametrize("case_id", [c["id"] for c in wide_cases.PARITY])
def test_wide_equals_oracle(oracle, hiplib, case_id):
    """No debug switch: n > 16 takes the wide kernels by itself, with mask bits, child ids, LDS strides and record words at
    their real size.  The oracle's and the device's seconds are printed for the budget of the suite."""
    case = wide_cases.by_id(case_id)
    model, segs = wide_cases.inputs(case)
    n, lmap = case["n"], bool(case.get("local_map"))
    al = segs["alleles"].reshape(len(segs["start"]), n)
    if case["kind"] == "unphased" and n >= 63:
        last = n - 2 if n % 2 == 0 else n - 3                                  # n = 64: pair (62, 63); n = 63: (60, 61), 62 alone
        assert (al[:, last] == 2).any() and (al[:, last + 1] == 2).any() and (n % 2 == 0 or not (al[:, n - 1] == 2).any())
    if case.get("missing"):
        assert ((al[:, 20:33] == -1).all(axis=1) & (al[:, :20] >= 0).all(axis=1)).sum() >= 3
    t0 = time.time()
    o = wide_cases.run_oracle(oracle, case, model, segs)
    t1 = time.time()
    g = _sweep(model, segs, case["Np"], n, local_recomb=lmap)
    t2 = time.time()
    print("%s: %d rows, %d resamplings, oracle %.2f s, device %.2f s" % (case_id, len(segs["start"]), o.trace()["resampled"].sum(),
                                                                        t1 - t0, t2 - t1))
    _device_equals_oracle(o, g, model, local_map=lmap, min_resampling=3)
    if case["E"] == 32:
        assert case["Np"] % 64 != 0 and (o.counts()["coal_count"] > 0).all()  # every epoch column of k_count carries events
    g.close(); o.close()


def test_wide_calibration_equals_oracle_at_40(oracle, hiplib):
    """lag calibration (calculate_median_survival_distances) at n = 40: the oracle's medians, bit for bit"""
    model = cases.make_model(n=40, E=8, L=3e5)
    dm, dt = pf.median_survival(model, seed=1, min_events=50, max_trees=16384)
    om, ot = oracle.median_survival(model, seed=1, min_events=50, max_trees=16384)
    assert dt == ot == 16384
    assert (_bits(dm) == _bits(om)).all()
    assert (om > 0).all() and len(np.unique(om)) == len(om)                  # every epoch has a median of its own


def test_stepwise_api_matches_run_at_40(oracle, hiplib):
    """update_segment / count / resample row by row equal run(), and both equal the oracle, at n = 40"""
    n, Np = 40, 130
    model = cases.make_model(n=n, E=8, L=5e4)
    segs = cases.make_segments(model, seed=90, max_seg_len=5000)
    a = _sweep(model, segs, Np, 5)
    b = ParticleFilter(model, Np, seed=5, max_trace_events=64); b.init_prior(segs["start"][0]); b.load_segments(segs)
    for s in range(len(segs["start"])):
        b.update_segment(s); b.count(s); b.resample(s)
    b.finish()
    assert _bits([a.logl()])[0] == _bits([b.logl()])[0]
    ca, cb = a.counts(), b.counts()
    for k in ("coal_count", "coal_opp", "rec_count", "rec_opp"):
        assert (_bits(ca[k]) == _bits(cb[k])).all()
    o = oracle.Oracle(model, Np, seed=5, max_trace_events=64)
    o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
    _device_equals_oracle(o, a, model, min_resampling=3)
    _device_equals_oracle(o, b, model, min_resampling=3)


def test_rows_without_data_and_rows_past_the_end_at_40(oracle, hiplib):
    """the rows of tests/test_gpu_row_chain.py at n = 40: a block in which every sample is missing (no update of the weights,
    no site), a block in which one is, and a last row without data that ends past the sequence"""
    n, Np, L = 40, 130, 6e4
    model = cases.make_model(n=n, E=8, L=L)
    segs = cases.make_segments(model, seed=91, max_seg_len=3000, missing_block=(1.5e4, 2.5e4, list(range(n))))
    al = segs["alleles"]
    part = (segs["start"] >= 3.5e4) & (segs["start"] < 4.0e4)
    al[part, 39] = -1
    assert int((al == -1).all(axis=1).sum()) >= 3 and part.sum() >= 3
    segs["length"][-1] += 7000.0
    al[-1, :] = -1
    assert segs["start"][-1] + segs["length"][-1] > L
    o = oracle.Oracle(model, Np, seed=4, max_trace_events=64)
    o.enable_local_recomb()
    o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
    g = _sweep(model, segs, Np, 4, local_recomb=True)
    assert g.segments_done() == len(segs["start"]) == len(o.trace()["T"])
    _device_equals_oracle(o, g, model, local_map=True, min_resampling=3)


# ---------------------------------------------------------------- 2. the prior beyond 16 haplotypes: Kingman's coalescent
@pytest.mark.parametrize("n", [32, 64])
def test_prior_is_kingman(hiplib, n):
    """Without data the weights stay equal and every particle is an independent SMC' chain, whose trees are draws from Kingman's
    coalescent: the mean height of the coalescence that takes k lineages to k - 1 is sum_{j=k..n} 1 / (lambda j (j - 1) / 2)
    with lambda the per-pair rate 1 / 2N, for every k (a lineage lost above bit 15 or 31 would break the sums of the deep ones)."""
    Np = 4096
    model = cases.make_model(n=n, E=1, L=1e5)
    segs = cases.nodata_segments(model, seglen=1000.0)
    g = _sweep(model, segs, Np, 5)
    assert g.counts()["resample_count"] == 0
    heights = np.sort(g.particles()["heights"].reshape(Np, n - 1), axis=1)
    lam = 1.0 / (2.0 * model["pop_sizes"][0])
    k = np.arange(n, 1, -1)                          # lineages before the r-th coalescence, r = 0 .. n - 2
    rates = lam * k * (k - 1) / 2.0
    expect = np.cumsum(1.0 / rates)
    se = np.sqrt(np.cumsum(1.0 / rates ** 2) / Np)
    z = (heights.mean(axis=0) - expect) / se
    assert np.abs(z).max() < 5.0, z


# ---------------------------------------------------------------- 3. the local recombination map at n = 64
def test_local_map_at_64(hiplib):
    n, Np = 64, 1024
    model = cases.make_model(n=n, E=4, L=6e4)
    segs = cases.make_segments(model, seed=9, max_seg_len=5000)
    g = _sweep(model, segs, Np, 2, local_recomb=True)
    lg = g.local_recomb()
    per_sample = lg["counts"][:n].sum(axis=1)
    assert lg["counts"][:n].sum() == pytest.approx(g.counts()["rec_count"].sum(), rel=1e-9)
    assert (per_sample > 0).all(), np.nonzero(per_sample == 0)[0]


# ---------------------------------------------------------------- 4. the site likelihood at high sample indices
_site_lik = cases.site_lik


def test_emission_at_high_sample_indices(hiplib):
    n, Np = 64, 512
    model = cases.make_model(n=n, E=4, L=1e4, rho=1e-30)
    E = len(model["lags"])
    alleles = np.zeros((3, n), np.int8)
    alleles[0, [33, 40, 47, 55, 63]] = 1              # derived only in samples >= 32
    alleles[1, 32:] = 1; alleles[1, 50] = -1           # ... and a missing sample >= 48
    alleles[2, [62, 63]] = 1; alleles[2, [49, 60]] = -1
    segs = dict(start=np.array([0.0, 0.0, 0.0]), length=np.zeros(3), state=np.zeros(3, np.int8), alleles=alleles,
                max_record_epoch=np.full(3, E - 1, np.int32))
    g = ParticleFilter(model, Np, seed=4, ess_fraction=0.0)
    g.init_prior(0.0); g.load_segments(segs)
    before = g.stats()["records"]
    p0 = g.particles()
    w = p0["w_post"].copy()
    for s in range(3):
        g.update_segment(s)
        p = g.particles()
        assert g.stats()["records"] == before           # no recombination: the trees of p0 are those the sites were scored on
        assert (p["children"] == p0["children"]).all() and (_bits(p["heights"]) == _bits(p0["heights"])).all()
        H = p["heights"].reshape(Np, n - 1); Cc = p["children"].reshape(Np, 2 * (n - 1))
        lik = np.array([_site_lik(H[i], Cc[i], alleles[s], model["mutation_rate"], n) for i in range(Np)])
        w = w * lik
        np.testing.assert_allclose(p["w_post"], w, rtol=1e-12, atol=0)
        if s < 2:
            g.resample(s)                                 # normalises in place (no resampling at ess_fraction 0)
            w = g.particles()["w_post"].copy()


# ---------------------------------------------------------------- 5. the simulator at n = 32
def test_simulator_at_32(hiplib):
    n = 32
    model = dict(change_times=np.array([0.0]), pop_sizes=np.array([1e4]), lags=np.ones(1), nsam=n, loci_length=3e6,
                 mutation_rate=2.5e-8, recombination_rate=1e-8)
    chunks = pf.simulate_sites(model, seed=3, nchunks=4)
    masks = np.concatenate([m for _, m in chunks])
    assert masks.dtype == np.uint64 and len(masks) > 20000
    carriers = ((masks[:, None] >> np.arange(n, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)
    assert (carriers.sum(axis=1) >= 1).all() and (carriers.sum(axis=1) <= n - 1).all()
    a_n = sum(1.0 / i for i in range(1, n))
    assert (carriers.sum(axis=1) == 1).mean() == pytest.approx(1.0 / a_n, rel=0.05)
    lo, hi = carriers[:, :16].sum(), carriers[:, 16:].sum()
    assert hi / lo == pytest.approx(1.0, abs=0.03)
    seg = simulate.simulate_seg_device(n, 2e5, 2.5e-8, 1e-8, [0.0], [1e4], seed=2)[0]
    assert seg["alleles"].shape[1] == n and (seg["alleles"][:, 16:] == 1).any()


# ---------------------------------------------------------------- 6. the binary at n = 32
def test_binary_at_32(hiplib, tmp_path):
    n, L = 32, 200000
    seg = simulate.simulate_seg(n, L, 2.5e-8, 1e-8, np.array([0.0, 1330.0, 13300.0]), np.full(3, 1e4), seed=4)
    path = str(tmp_path / "d.seg")
    simulate.write_seg(path, seg)
    binary = os.path.join(ROOT, "bin", "smcsmc")
    core = ("-N0 10000 -t %g -r %g %d -eN 0 1 -eN 0.0333 1 -eN 0.333 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    r = subprocess.run([binary] + core + ["-nsam", str(n), "-Np", "300", "-EM", "1", "-tmax", "4", "-seed", "2", "-seg", path,
                                          "-o", str(tmp_path / "m")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in open(str(tmp_path / "m.out")) if l.strip()]
    assert rows[0][0] == "Iter" and rows[-1][4] == "LogL" and np.isfinite(float(rows[-1][5]))
    with gzip.open(str(tmp_path / "m.recomb.gz"), "rt") as f:
        header = f.readline().split()
    assert header[4:4 + n] == [str(k + 1) for k in range(n)] and header[4 + n:] == ["time", "log_time"]


# ---------------------------------------------------------------- 7. a re-initialised handle equals a fresh one
@pytest.mark.parametrize("n", [12, 32])
def test_second_sweep_equals_fresh_handle(oracle, hiplib, n):
    """The sweep after pf_init_prior on a used handle is that of a fresh handle, bit for bit.  The count totals are the one thing
    a handle keeps across pf_init_prior (they add up over its sweeps, as before): what the second sweep added to them is the
    fresh handle's counts, up to the rounding of the running sums."""
    model = cases.make_model(n=n, E=6, L=1e5)
    segs = cases.make_segments(model, seed=n, max_seg_len=5000)
    a = _sweep(model, segs, 256, 8)
    first = a.counts()
    a.init_prior(segs["start"][0]); a.run(); a.finish()
    both = a.counts()
    b = _sweep(model, segs, 256, 8)
    assert b.counts()["resample_count"] > 0
    added = dict(both)
    for k in COUNT_KEYS:
        added[k] = both[k] - first[k]
    _same_run(a, b, counts_rtol=1e-9, counts_a=added)
    if n == 32:
        # ... and the fresh handle's sweep, hence the second sweep of the used one, is the oracle's
        o = oracle.Oracle(model, 256, seed=8, max_trace_events=64)
        o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
        _device_equals_oracle(o, b, model, min_resampling=3)
        assert _bits([a.logl()])[0] == _bits([o.logl()])[0]
