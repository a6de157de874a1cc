"""The CPU oracle at up to 64 haplotypes, judged without any device code.

(0) Widening it from 16 to 64 moved nothing at n <= 16: the fingerprints of tests/golden/oracle_fingerprints.json, recorded with
    the oracle before it was widened, are recomputed and compared for equality.
(1..5) Beyond 16 the oracle is in effect new code, and "device equals oracle" is worth what the oracle is worth.  These tests
    hold it to closed forms and to numpy: Kingman's coalescent for the prior (moments of every height, total length, the split
    at the root, cherries per sample), stationarity of the SMC' chain and the model's rates from its counts, the site likelihood
    at high sample indices, and the per-sample rows of the local recombination map.

Every statistical assertion names its statistic, its distribution under "the oracle is right" and the threshold: |z| < 5 for a
statistic that is standard normal there (two-sided p = 5.7e-7), p > 1e-6 for a chi-square.  Seeds are fixed; the margins the
oracle passes with are in the comments next to the assertions (largest |z| / smallest p seen on the CPU)."""
import json
import os

import numpy as np
import pytest
from scipy import stats

import cases
import oracle_fingerprints

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_fingerprints.json")


# ---------------------------------------------------------------- 0. n <= 16 unchanged, bit for bit
@pytest.mark.parametrize("name", [c[0] for c in oracle_fingerprints.CONFIGS])
def test_oracle_at_16_or_fewer_is_unchanged(oracle, name):
    recorded = json.load(open(GOLDEN))["configurations"][name]
    now = oracle_fingerprints.fingerprint(oracle, name)
    assert sorted(now) == sorted(recorded)
    for k in recorded:
        assert now[k] == recorded[k], (name, k)
    if recorded["kind"] != "calibration":
        assert recorded["resamplings"] >= 3 and len(recorded["trace"]["T"]) == recorded["rows"]


# ---------------------------------------------------------------- helpers
def _kingman_rates(n, N):
    """rate of the coalescence that takes k lineages to k - 1, for k = n .. 2 (the r-th coalescence, r = 0 .. n - 2)"""
    k = np.arange(n, 1, -1)
    return k, k * (k - 1) / 2.0 / (2.0 * N)


def _height_z(heights, n, N):
    """z of the sample mean and of the sample variance of every sorted height.  The r-th height is a sum of independent
    exponentials with the rates above: mean sum 1/rate, variance sum 1/rate^2, fourth cumulant sum 6/rate^4.  The sample mean of
    M draws has variance var/M, the unbiased sample variance has variance (mu4 - var^2 (M - 3)/(M - 1))/M with
    mu4 = kappa4 + 3 var^2; both are normal to well within the threshold at the M used here."""
    M = heights.shape[0]
    _, rates = _kingman_rates(n, N)
    mean = np.cumsum(1.0 / rates); var = np.cumsum(1.0 / rates ** 2); k4 = np.cumsum(6.0 / rates ** 4)
    z_mean = (heights.mean(axis=0) - mean) / np.sqrt(var / M)
    mu4 = k4 + 3 * var ** 2
    z_var = (heights.var(axis=0, ddof=1) - var) / np.sqrt((mu4 - var ** 2 * (M - 3) / (M - 1)) / M)
    return z_mean, z_var


def _clade_sizes(children, n):
    """number of samples below every node id (leaves first), for all particles at once: [Np, 2n - 1]"""
    Np = children.shape[0]
    size = np.zeros((Np, 2 * n - 1), np.int64)
    size[:, :n] = 1
    rows = np.arange(Np)
    for r in range(n - 1):
        size[:, n + r] = size[rows, children[:, r, 0]] + size[rows, children[:, r, 1]]
    return size


def _prior(oracle, n, Np, seed, E=1):
    model = cases.make_model(n=n, E=E, L=1e5)
    o = oracle.Oracle(model, Np, seed=seed)
    o.init_prior(0.0)
    p = o.particles()
    o.close()
    return model, p


# ---------------------------------------------------------------- 1. the prior: Kingman's coalescent
@pytest.mark.parametrize("n", [24, 40, 64])
def test_prior_heights_and_length_are_kingman(oracle, n):
    Np, N = 8000, 1e4
    model, p = _prior(oracle, n, Np, seed=100 + n)
    H = p["heights"]
    assert (np.diff(H, axis=1) >= 0).all() and (H[:, 0] > 0).all()          # rank-sorted, as the tree is kept
    z_mean, z_var = _height_z(H, n, N)
    print("n", n, "max |z| mean", np.abs(z_mean).max(), "variance", np.abs(z_var).max())
    assert np.abs(z_mean).max() < 5.0, z_mean           # seen: 1.7 / 1.7 / 2.5 at n = 24 / 40 / 64
    assert np.abs(z_var).max() < 5.0, z_var             # seen: 2.0 / 2.2 / 2.0
    # total branch length sum_k k T_k, T_k the time with k lineages: mean sum k / rate_k = 4 N H(n - 1), variance sum k^2 / rate_k^2
    k, rates = _kingman_rates(n, N)
    length = (np.diff(np.concatenate([np.zeros((Np, 1)), H], axis=1), axis=1) * k[None, :]).sum(axis=1)
    assert (k / rates).sum() == pytest.approx(4 * N * (1.0 / np.arange(1, n)).sum(), rel=1e-12)
    z_len = (length.mean() - (k / rates).sum()) / np.sqrt((k ** 2 / rates ** 2).sum() / Np)
    print("z total length", z_len)
    assert abs(z_len) < 5.0, z_len                      # seen: -1.0 / 0.0 / 0.6


@pytest.mark.parametrize("n", [24, 40, 64])
def test_prior_topology_is_exchangeable(oracle, n):
    """The split at the root and the cherries of Kingman's coalescent.  A child id that went through a narrow field, or a
    renumbering that is off for ids above 31 or 63, shows as samples with high indices behaving differently."""
    Np = 200 * n
    model, p = _prior(oracle, n, Np, seed=200 + n)
    Ch = p["children"].astype(np.int64)
    # every node id 0 .. 2n - 3 is the child of exactly one node, the root (2n - 2) of none
    ids = np.sort(Ch.reshape(Np, -1), axis=1)
    assert (ids == np.arange(2 * n - 2)[None, :]).all()
    assert (Ch < n + np.arange(n - 1)[None, :, None]).all()                  # children lie below their parent's rank
    size = _clade_sizes(Ch, n)
    assert (size[:, 2 * n - 2] == n).all()
    # (a) the smaller clade at the root has k samples with probability 2 / (n - 1) for k < n / 2 and 1 / (n - 1) for k = n / 2
    #     (one root clade is uniform on 1 .. n - 1).  Chi-square with n // 2 - 1 degrees of freedom, p > 1e-6.
    small = np.minimum(size[np.arange(Np), Ch[:, n - 2, 0]], size[np.arange(Np), Ch[:, n - 2, 1]])
    ks = np.arange(1, n // 2 + 1)
    prob = np.where(2 * ks == n, 1.0, 2.0) / (n - 1)
    assert prob.sum() == pytest.approx(1.0)
    obs = np.bincount(small, minlength=n // 2 + 1)[1:]
    print("n", n, "root split p", stats.chisquare(obs, prob * Np).pvalue)
    assert stats.chisquare(obs, prob * Np).pvalue > 1e-6                     # seen: 0.38 / 0.16 / 0.54
    # (b) a sample sits in a cherry (its sibling is a sample) with probability 2 / 3 for n >= 3 (n / 3 cherries are expected),
    #     the same for every sample.  Per sample over all particles the count is Binomial(Np, 2/3): |z| < 5 each.
    both = (Ch < n).all(axis=2)                                               # nodes whose two children are samples
    in_cherry = np.zeros((Np, n), bool)
    pi, ri = np.nonzero(both)
    in_cherry[pi, Ch[pi, ri, 0]] = True
    in_cherry[pi, Ch[pi, ri, 1]] = True
    z = (in_cherry.sum(axis=0) - Np * 2 / 3) / np.sqrt(Np * 2 / 9)
    print("cherry per sample max |z|", np.abs(z).max())
    assert np.abs(z).max() < 5.0, z                                          # seen: 2.2 / 2.5 / 3.3
    #     Indicators of two samples of one tree are dependent, so for a chi-square over the samples particle j contributes
    #     sample j mod n alone: n independent Binomial(Np / n, 2/3) counts, chi-square with n degrees of freedom, p > 1e-6.
    own = in_cherry[np.arange(Np), np.arange(Np) % n]
    cnt = np.bincount(np.arange(Np) % n, weights=own, minlength=n)
    m = Np // n
    chi2 = ((cnt - m * 2 / 3) ** 2 / (m * 2 / 9)).sum()
    print("cherry chi-square p", stats.chi2.sf(chi2, n))
    assert stats.chi2.sf(chi2, n) > 1e-6                                     # seen: 0.54 / 0.29 / 0.72
    #     ... and the lower and the upper half of the samples hold the same number of cherry leaves: the difference of two
    #     such sums over disjoint sets of these independent counts is normal with variance n (Np / n) 2 / 9
    half = n // 2
    zh = (cnt[:half].sum() - cnt[n - half:].sum()) / np.sqrt(2 * half * m * 2 / 9)
    print("cherry halves z", zh)
    assert abs(zh) < 5.0, zh                                                 # seen: -0.1 / 1.0 / -1.9


# ---------------------------------------------------------------- 2. SMC' stationarity and the model's rates
@pytest.mark.parametrize("n", [33, 64])
def test_no_data_chain_keeps_kingman_and_returns_the_rates(oracle, n):
    """Without data the weights stay equal and every particle is an SMC' chain that starts from Kingman's coalescent, which is
    its stationary law: after many genealogy updates the heights still have Kingman's means.  Its events, counted with the
    weights 1 / Np, return the model: in epoch e the number of coalescences is Poisson-like with mean (opportunity / 2N) --
    count minus compensator is a martingale whose variance is the expected count -- so
    z = (count - opp / 2N) Np / sqrt(Np opp / 2N) is standard normal; likewise for recombinations with rate rho."""
    Np, N, rho, E = 1500, 1e4, 1e-8, 8
    model = cases.make_model(n=n, E=E, L=1.5e5, N0=N, rho=rho)
    segs = cases.nodata_segments(model, seglen=1000.0)
    o = oracle.Oracle(model, Np, seed=300 + n)
    o.init_prior(0.0)
    o.run(o.pack_segments(model, segs))
    c = o.counts()
    assert o.logl() == 0.0 and c["resample_count"] == 0
    assert o.stats()["recombinations"] > 150 * Np                           # about 280 (n = 33) / 330 (n = 64) updates per particle
    z_mean, _ = _height_z(o.particles()["heights"], n, N)
    print("n", n, "heights after the run max |z|", np.abs(z_mean).max())
    assert np.abs(z_mean).max() < 5.0, z_mean                               # seen: 2.1 / 3.1 at n = 33 / 64
    with_events = 0
    for e in range(E):
        if c["coal_count"][e] > 0:
            zc = (c["coal_count"][e] - c["coal_opp"][e] / (2 * N)) * Np / np.sqrt(Np * c["coal_opp"][e] / (2 * N))
            print("epoch", e, "coalescence z", zc)
            assert abs(zc) < 5.0, (e, zc)                                   # seen: 1.7 / 2.3 at most
            with_events += 1
        if c["rec_count"][e] > 0:
            zr = (c["rec_count"][e] - c["rec_opp"][e] * rho) * Np / np.sqrt(Np * c["rec_opp"][e] * rho)
            print("epoch", e, "recombination z", zr)
            assert abs(zr) < 5.0, (e, zr)                                   # seen: 2.0 / 1.9 at most
            with_events += 1
    assert with_events >= 2 * (E - 1)
    # opportunity bookkeeping: the recombination opportunity is the integral of the tree length along the sequence
    assert c["rec_opp"].sum() == pytest.approx(model["loci_length"] * 4 * N * (1.0 / np.arange(1, n)).sum(), rel=0.03)
    o.close()


# ---------------------------------------------------------------- 3. the site likelihood at high sample indices
def test_emission_at_high_sample_indices(oracle):
    """update_weight_at_site against the numpy restatement (cases.site_lik), one site at a time on trees that do not change:
    derived alleles only in samples >= 32, missing samples >= 48, and unphased pairs.  The oracle's rule for an unphased pair
    (calculate_initial_haplotype_configuration / next_haplotype, pc.cpp:138-181): samples 2j and 2j + 1 both carry code 2, the
    site's likelihood is the mean over the two phasings (0, 1) and (1, 0) of every such pair, all combinations."""
    n, Np = 64, 256
    model = cases.make_model(n=n, E=4, L=1e4, rho=1e-30)
    E = len(model["lags"])
    alleles = np.zeros((5, n), np.int8)
    alleles[0, [33, 40, 47, 55, 63]] = 1              # derived only in samples >= 32
    alleles[1, 32:] = 1; alleles[1, 50] = -1           # ... and a missing sample >= 48
    alleles[2, [62, 63]] = 1; alleles[2, [49, 60]] = -1
    alleles[3, [62, 63]] = 2; alleles[3, 35] = 1       # the last pair unphased
    alleles[4, [62, 63]] = 2; alleles[4, [30, 31]] = 2; alleles[4, [32, 33]] = 2; alleles[4, 61] = 1; alleles[4, 48] = -1
    S = len(alleles)
    segs = dict(start=np.zeros(S), length=np.zeros(S), state=np.zeros(S, np.int8), alleles=alleles,
                max_record_epoch=np.full(S, E - 1, np.int32))
    o = oracle.Oracle(model, Np, seed=4, ess_fraction=0.0)
    o.init_prior(0.0)
    si = o.pack_segments(model, segs)
    p0 = o.particles()
    H = p0["heights"]; Cc = p0["children"].reshape(Np, 2 * (n - 1)).astype(np.int64)
    w = p0["w_post"].copy()
    logl = 0.0
    for s in range(S):
        o.update_segment(si, s)
        p = o.particles()
        assert o.stats()["recombinations"] == 0 and (p["children"] == p0["children"]).all()
        pairs = [i for i in range(0, n - 1, 2) if alleles[s, i] == 2]
        assert all(alleles[s, i + 1] == 2 for i in pairs) and len(pairs) == [0, 0, 0, 1, 3][s]
        lik = np.zeros(Np)
        for phase in range(1 << len(pairs)):
            hap = alleles[s].copy()
            for j, i in enumerate(pairs):
                hap[i], hap[i + 1] = ((phase >> j) & 1), 1 - ((phase >> j) & 1)
            lik += np.array([cases.site_lik(H[i], Cc[i], hap, model["mutation_rate"], n) for i in range(Np)])
        lik /= 1 << len(pairs)
        assert (lik > 0).all() and lik.std() > 0
        w = w * lik
        logl += np.log(w.sum())
        w = w / w.sum()                                  # update_segment ends with normalize_probability
        np.testing.assert_allclose(p["w_post"], w, rtol=1e-11, atol=0)
        np.testing.assert_allclose(p["w_pilot"], w, rtol=1e-11, atol=0)
        assert o.logl() == pytest.approx(logl, rel=1e-10)
        o.resample(float(s))                             # ess_fraction 0: never resamples; closes the step as the run does
    o.close()


# ---------------------------------------------------------------- 4. the local recombination map at n = 64
def test_local_map_rows_at_64(oracle):
    """With data at n = 64: a recombination event gives weight / #descendants to the row of every sample below the cut branch
    (count.cpp:559-613), so the sample rows add up to the recombination count; every sample is below some cut branch; and,
    sample labels being arbitrary, the 64 row sums are exchangeable: given their values, the sum over samples 0..31 is that of a
    random half, mean n/2 mean(r), variance (n/4) var(r) (sampling 32 of 64 without replacement, var with ddof = 1): |z| < 5."""
    n, Np = 64, 300
    model = cases.make_model(n=n, E=4, L=5e4)
    segs = cases.make_segments(model, seed=9, max_seg_len=5000)
    o = oracle.Oracle(model, Np, seed=2)
    o.enable_local_recomb()
    o.init_prior(0.0)
    o.run(o.pack_segments(model, segs))
    lm, c = o.local_recomb(model["loci_length"]), o.counts()
    assert c["resample_count"] >= 3
    rows = lm["counts"][:n].sum(axis=1)
    assert rows.sum() == pytest.approx(c["rec_count"].sum(), rel=1e-9) and c["rec_count"].sum() > 10
    assert (rows > 0).all(), np.nonzero(rows == 0)[0]
    z = (rows[:32].sum() - 32 * rows.mean()) / np.sqrt(16 * rows.var(ddof=1))
    print("local map halves z", z)
    assert abs(z) < 5.0, z                                                   # seen: 1.2
    assert lm["counts"][n].sum() > 0 and lm["counts"][n + 1].sum() > 0       # the time and log-time rows
    o.close()


# ---------------------------------------------------------------- 5. what the data cases of the GPU parity tests rely on
def test_wide_parity_cases_resample(oracle):
    """tests/test_gpu_many_samples.py compares the device with this oracle at 17..64 haplotypes and asserts, case by case, that
    the run resamples at least three times.  That is a property of the inputs and of the oracle alone; it is checked here, where
    no device is needed, so that a change of the simulator or of the cases cannot empty those tests unnoticed."""
    import wide_cases
    for case in wide_cases.PARITY:
        model, segs = wide_cases.inputs(case)
        o = wide_cases.run_oracle(oracle, case, model, segs)
        assert o.trace()["resampled"].sum() >= 3, case
        assert wide_cases.max_unphased_pairs(segs) <= 12, case             # 2^pairs phasings per particle and site
        o.close()
