"""An independent Monte Carlo statement of the model (tests/mc_model.py) as a pin of the CPU oracle beyond two samples.

"HIP == oracle" shows self-consistency, and tests/exact_hmm2.py pins two samples in one population.  Here the model is
written down once more for any number of samples and populations -- a prior sampler of SMC' graphs in the structured
coalescent, the emission the filter weights by -- and p(data | model) and the posterior expectation of every count are
estimated by brute force on data sets of a dozen sites (tests/golden/mc_model.json, made by tests/golden/make_mc_model.py).
A particle filter's normalising-constant estimate is unbiased at any Np, so the oracle's mean of exp(logl) over seeds must
equal that number, with resampling off and on, with focused sampling, a guide and the look-ahead
(tests/mc_model_check.py states the comparison; tests/test_gpu_mc_model.py applies it to the device).

First the new sampler is checked against things that are neither the oracle nor the filter: the exact forward-backward
answer for two samples, Kingman's node heights, the two-island closed forms, a join, the absence of data, and the
stationarity of the SMC' transition.
"""
import math
import multiprocessing as mp
import random

import numpy as np
import pytest

import cases
import mc_model
import mc_model_check as chk

CT = np.array([0.0, 2000.0, 20000.0])
SIZES = [1.0, 0.4, 2.5]


def _one_pop(n, L=8000.0):
    m = cases.make_model(n=n, E=3, L=L, lag=1e9, sizes=SIZES)
    m["change_times"] = CT
    return m


def _two_pops(n, sample_pops, mig=2.0, one_way=False):
    m = cases.make_structured(_one_pop(n), P=2, split_epoch=2, mig=mig, sample_pops=sample_pops, sizes=[1.0, 0.5])
    if one_way:
        m["mig_rates"][:, 1, 0] = 0.0
    return m


def _intensity(m, t):
    """Lam(t) = int_0^t ds / 2N(s) of a one-population model"""
    T = list(m["change_times"]) + [math.inf]
    return sum(max(0.0, min(t, T[e + 1]) - T[e]) / (2 * m["pop_sizes"][e]) for e in range(len(T) - 1))


def _z(values, expected):
    v = np.asarray(values, float)
    return (v.mean() - expected) / (v.std(ddof=1) / math.sqrt(len(v)))


def test_fastexp_is_the_one_of_cases():
    x = np.concatenate([-np.logspace(-9, 1, 200), [0.0, 0.5, -0.7184, -0.7185]])
    mine = np.array([mc_model.fastexp(float(v)) for v in x])
    pade = x * x < 0.516167859
    assert pade.sum() > 150 and (~pade).sum() > 10
    np.testing.assert_array_equal(mine[pade], cases.fastexp(x)[pade])                  # the same operations in the same order
    np.testing.assert_allclose(mine[~pade], cases.fastexp(x)[~pade], rtol=4e-16)      # (two libraries' exp: an ulp)


def test_the_statement_imports_nothing_of_the_project():
    import ast
    tree = ast.parse(open(mc_model.__file__).read())
    mods = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    mods |= {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert mods == {"bisect", "math", "random", "numpy"}


# ---------------------------------------------------------------------------------------------------------------
# the sampler against exact answers

def test_two_samples_equal_the_exact_forward_backward_answer():
    """case n2 of the fixture (two samples, three epochs, seven rows) against tests/exact_hmm2.py on the same rows, which
    the fixture stores at K = 600 and K = 300 cells: log p and the four count vectors within 4 combined standard errors,
    the discretisation error taken as the change under halving the grid.  The only place where the sampler meets an exact
    answer, so the fixture's log p carries at most 0.5 % here."""
    g = chk.GOLD["n2"]
    ex, half = g["exact"], g["exact_half_resolution"]
    assert g["logp_rse"] <= 0.005
    err = math.hypot(g["logp_rse"], abs(ex["logl"] - half["logl"]))
    print("log p: Monte Carlo %.5f +- %.5f, exact %.5f (K/2: %.5f)" % (g["logp"], g["logp_rse"], ex["logl"], half["logl"]))
    assert abs(g["logp"] - ex["logl"]) <= 4 * err
    for k in ("rec_count", "rec_opp", "coal_count", "coal_opp"):
        mc = np.array(g["stats"][k]).ravel(); se = np.array(g["se"][k]).ravel()
        e1, e2 = np.array(ex[k]), np.array(half[k])
        z = (mc - e1) / np.hypot(se, np.abs(e1 - e2))
        print(k, "Monte Carlo", mc, "exact", e1, "rel. s.e.", se / mc, "z", z)
        assert np.abs(z).max() <= 4, (k, z)
        assert (se / mc).max() <= 0.03, (k, se / mc)            # (and the agreement means something)


def test_kingman_node_heights_with_varying_sizes():
    """n = 4, sizes N0 x (1, 0.4, 2.5): in units of the coalescence intensity Lam(t) = int dt / 2N the k-th node from the
    top of Kingman's coalescent has the expected height sum_{j = k + 1}^{n} 1 / C(j, 2): 1/6, 1/6 + 1/3, 1/6 + 1/3 + 1"""
    m = _one_pop(4)
    mm = mc_model.Model(m)
    rng = random.Random(5)
    hs = np.array([sorted(_intensity(m, h) for h in mc_model.ARG(mm, rng).height[4:]) for _ in range(6000)])
    for k, want in enumerate((1 / 6, 1 / 6 + 1 / 3, 1 / 6 + 1 / 3 + 1)):
        assert abs(_z(hs[:, k], want)) <= 4, (k, hs[:, k].mean(), want)
    # and the second moment of the root: the variance of a sum of independent exponentials, 1/36 + 1/9 + 1
    assert abs(_z((hs[:, 2] - 1.5) ** 2, 1 / 36 + 1 / 9 + 1)) <= 4


def test_symmetric_two_island_pairwise_times():
    """Two demes of N diploids, every lineage moves to the other deme at rate m.  With c = 1 / 2N, Tw and Tb the expected
    coalescence times of two lineages in the same and in different demes:  Tw = 1/(c + 2m) + 2m/(c + 2m) Tb,  Tb = 1/(2m) + Tw,
    hence  Tw = 4N  whatever m (Strobeck 1987, Genetics 117:149; Notohara 1990, J. Math. Biol. 29:59, the case of two demes)
    and  Tb = 4N + 1/(2m)."""
    N, mig = 1e4, 2.0
    m = cases.make_structured(cases.make_model(n=2, E=1, L=1000.0, lag=1e9), P=2, split_epoch=1, mig=mig)
    rate = mig / (4 * N)
    assert m["mig_rates"][0, 0, 1] == rate and not m["single_mig"].any()
    for pops, want in (([0, 0], 4 * N), ([0, 1], 4 * N + 1 / (2 * rate))):
        mm = mc_model.Model(dict(m, sample_pops=pops))
        rng = random.Random(6)
        t = [mc_model.ARG(mm, rng).height[2] for _ in range(8000)]
        assert abs(_z(t, want)) <= 4, (pops, np.mean(t), want)


def test_after_a_join_no_lineage_is_left_in_the_joined_population():
    """population 1 joins population 0 at 20 000 generations: along 40 graphs with a dozen recombinations each, no branch of
    any local tree is in population 1 from then on, and below it lineages do get there (the check is not empty)"""
    m = _two_pops(4, [0, 0, 1, 1])
    mm = mc_model.Model(m)
    rng = random.Random(7)
    seen_one = 0
    for _ in range(40):
        g = mc_model.ARG(mm, rng)
        for _ in range(12):
            g.recombine()
            for v in range(7):
                top = g.height[g.parent[v]] if v != g.root else g.height[v]
                times = [tm for tm, _ in g.path[v]]
                assert times == sorted(times) and all(g.height[v] <= tm <= top for tm in times)   # a path lies on its branch
                for t in [g.height[v]] + [tm for tm, _ in g.path[v]] + [top - 1e-9]:
                    if t >= 20000.0:
                        assert g.pop_at(v, t) == 0
                    else:
                        seen_one += g.pop_at(v, t) == 1
            assert g.path[g.root] == []
    assert seen_one > 100


@pytest.mark.parametrize("kind", ["one", "two"])
def test_without_data_the_weight_is_one_and_the_counts_return_the_model(kind):
    """all samples missing: every weight is 1, log p = 0 with no error, and the ratios of the expected counts are the
    parameters themselves (sizes, recombination rate, migration rates) within 4 standard errors of the ratio"""
    m = _one_pop(3) if kind == "one" else _two_pops(4, [0, 0, 1, 1], one_way=True)
    r = mc_model.run(m, mc_model.no_rows(m, 8000.0), 3000, 8)
    assert r["logp"] == 0.0 and r["logp_rse"] == 0.0 and r["cv"] == 0.0
    st, se = r["stats"], r["se"]
    rel = lambda a, b: math.hypot(se[a].sum() / st[a].sum(), se[b].sum() / st[b].sum())
    rho = st["rec_count"].sum() / st["rec_opp"].sum()
    assert abs(rho / m["recombination_rate"] - 1) <= 4 * rel("rec_count", "rec_opp")
    ne = st["coal_opp"] / (2 * np.maximum(st["coal_count"], 1e-300))
    size = np.asarray(m["pop_sizes"], float).reshape(ne.shape)
    for idx in np.ndindex(ne.shape):
        if st["coal_count"][idx] > 0.3:
            tol = 4 * math.hypot(se["coal_count"][idx] / st["coal_count"][idx], se["coal_opp"][idx] / st["coal_opp"][idx])
            assert abs(ne[idx] / size[idx] - 1) <= tol, (idx, ne[idx], size[idx], tol)
    if kind == "two":
        assert st["coal_count"][2, 1] == 0 and st["mig_opp"][2, 1] == 0          # nobody is there after the join
        assert (st["mig_count"][:, 1, 0] == 0).all() and st["mig_opp"][1, 1] > 0  # one way; time is spent there all the same
        for e in (0, 1):
            mhat = st["mig_count"][e, 0, 1] / st["mig_opp"][e, 0]
            tol = 4 * math.hypot(se["mig_count"][e, 0, 1] / st["mig_count"][e, 0, 1], se["mig_opp"][e, 0] / st["mig_opp"][e, 0])
            assert abs(mhat / m["mig_rates"][e, 0, 1] - 1) <= tol, (e, mhat)


@pytest.mark.parametrize("kind", ["one", "two"])
def test_the_smc_prime_transition_leaves_the_prior_stationary(kind):
    """Fifty kilobases into a sequence without data -- thirty recombinations on average -- the local tree is still a draw of
    the prior: root height and tree length (one population: also in intensity units, against Kingman's 4/3 and its variance
    10/9 for three samples; both: against the trees at position 0), means and second moments within 4 standard errors.  The
    comparison is at a fixed position, not after a fixed number of recombinations (trees seen after k events are biased
    towards long ones).  A floating lineage that meets the wrong number of partners, or a regraft that loses a branch,
    moves these; what it cannot see is SMC against SMC', which have the same marginal tree -- that difference shows in the
    likelihood of data (the sensitivity table of profiles/round18/mc_model.md)."""
    m = _one_pop(3) if kind == "one" else _two_pops(4, [0, 0, 1, 1], one_way=True)
    mm = mc_model.Model(m)
    rng = random.Random(9)
    first, last = [], []
    for _ in range(2500):
        g, f = mc_model.tree_at(mm, rng, 50000.0)
        first.append(f)
        last.append((g.height[g.root], g.ltree))
    first, last = np.array(first), np.array(last)
    if kind == "one":
        lam = np.array([_intensity(m, h) for h in last[:, 0]])
        assert abs(_z(lam, 4 / 3)) <= 4 and abs(_z((lam - 4 / 3) ** 2, 1 + 1 / 9)) <= 4
    for col in (0, 1):
        for power in (1, 2):
            a, b = first[:, col] ** power, last[:, col] ** power
            z = (a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
            assert abs(z) <= 4, (kind, col, power, a.mean(), b.mean(), z)


# ---------------------------------------------------------------------------------------------------------------
# the fixture, and the oracle against it

@pytest.mark.parametrize("case", chk.CASES)
def test_the_fixture_has_the_precision_and_the_cells_the_comparison_needs(case):
    chk.golden_is_usable(case)


def test_the_fixture_is_what_its_generator_would_draw():
    """model and rows of every case are the ones make_mc_model.py builds, and a sixty-fourth of the first chunk's draws
    reproduces from the recorded seed (the whole file takes ten minutes; python tests/golden/make_mc_model.py)"""
    mk = chk.mk
    for case in chk.CASES:
        c, g = mk.CASES[case], chk.GOLD[case]
        m = mk.case_model(c)
        rows = mk.case_rows(c, m)
        assert (g["M"], g["seed"], g["chunks"]) == (c["M"], c["seed"], mk.CHUNKS)
        for k in ("start", "length", "state", "alleles"):
            np.testing.assert_array_equal(np.asarray(g["rows"][k]), rows[k])
        for k in ("change_times", "pop_sizes", "mig_rates", "single_mig"):
            if k in m:
                np.testing.assert_array_equal(np.asarray(g["model"][k], float), np.asarray(m[k], float))
    # the draws: deterministic in (seed, chunk)
    m, rows = chk.inputs("n3")
    a = mc_model.accumulate(m, rows, 200, 12 * 10007)
    b = mc_model.accumulate(m, rows, 200, 12 * 10007)
    assert a[1][0] == b[1][0] and a[1][0] > 0


@pytest.fixture(scope="module")
def pool(oracle):
    with mp.Pool(4) as p:
        yield p


@pytest.mark.parametrize("mode", list(chk.MODES))
@pytest.mark.parametrize("case", chk.CASES)
def test_the_oracle_targets_the_model(pool, case, mode):
    """32 seeds: log(mean exp(logl)) and the exp(logl)-weighted counts equal the fixture within 4 combined standard errors,
    at a combined relative standard error of at most 3 % (log p) and 6 % (a compared cell)"""
    chk.oracle_check(pool, case, mode)
