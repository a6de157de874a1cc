"""tests/mc_model_ancient.py, the independent statement of the model with ancient samples (-eI), checked on the CPU: it is
mc_model.py where no sample is ancient, its first tree has the closed-form height, its graphs stay trees, and the fixture it
made (tests/golden/mc_model_ancient.json) is precise enough to hold the device to (tests/test_gpu_ancient.py)."""
import json
import math
import os
import random

import numpy as np
import pytest

import cases
import mc_model
import mc_model_ancient as mca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CT = [0.0, 2000.0, 20000.0]
SIZES = [1.0, 0.4, 2.5]


def _structured(n, pops, times, L=4000.0, mig=4.0):
    m = cases.make_model(n=n, E=3, L=L, lag=1e9, sizes=SIZES)
    m["change_times"] = np.array(CT)
    m = cases.make_structured(m, P=2, split_epoch=2, mig=mig, sample_pops=pops)
    if times is not None:
        m["sample_times"] = list(times)
    return m


@pytest.mark.parametrize("n,pops", [(3, [0, 1, 1]), (4, [0, 1, 0, 1])])
def test_zero_times_are_the_model_without_times(n, pops):
    """same random.Random seed, same draws: heights, parents, weights and every statistic"""
    plain = _structured(n, pops, None)
    zero = _structured(n, pops, [0.0] * n)
    rows = dict(start=[0.0, 1500.0], length=[1500.0, 2500.0], state=[0, 0], alleles=[[0, 1] + [0] * (n - 2), [1] * (n - 1) + [0]])
    m0, m1 = mc_model.Model(plain), mca.Model(zero)
    first, prow = mc_model.prepare_rows(m0, rows)
    r0, r1 = random.Random(5), random.Random(5)
    for _ in range(200):
        w0, s0 = mc_model.draw(m0, first, prow, r0)
        w1, s1 = mca.draw(m1, first, prow, r1)
        assert w0 == w1 and s0 == s1
    g0, g1 = mc_model.ARG(m0, random.Random(9)), mca.ARG(m1, random.Random(9))
    for _ in range(50):
        assert g0.height == g1.height and g0.parent == g1.parent and g0.ltree == g1.ltree and g0.path == g1.path
        g0.recombine(); g1.recombine()
    assert mc_model.run(plain, rows, 300, 3)["logp"] == mca.run(zero, rows, 300, 3)["logp"]


def test_root_height_of_two_serial_samples():
    """one population, the second sample enters at change_times[1]: the first lineage waits alone, then the pair coalesces at
    rate 1 / (2 N(t)) from there -- E[height] = t1 + sum_e P(no coalescence before e) (1 - exp(-d_e / 2N_e)) 2N_e"""
    m = cases.make_model(n=2, E=3, L=1000.0, lag=1e9, sizes=SIZES)
    m["change_times"] = np.array(CT)
    m["sample_times"] = [0.0, CT[1]]
    N = np.asarray(m["pop_sizes"], float)
    exact, surv = CT[1], 1.0
    for e in (1, 2):
        rate = 1.0 / (2.0 * N[e])
        d = CT[e + 1] - CT[e] if e + 1 < 3 else math.inf
        exact += surv * (1.0 - math.exp(-rate * d)) / rate
        surv *= math.exp(-rate * d)
    model = mca.Model(m)
    rng = random.Random(1)
    M = 20000
    h = np.array([(lambda g: g.height[g.root])(mca.ARG(model, rng)) for _ in range(M)])
    se = h.std(ddof=1) / math.sqrt(M)
    print("mean root height %.1f +- %.1f, closed form %.1f" % (h.mean(), se, exact))
    assert h.min() > CT[1]
    assert abs(h.mean() - exact) <= 4 * se


def test_graphs_stay_trees_above_their_leaves():
    """n = 4 along 300 sequences of recombinations: every parent is higher than its child -- an ancient leaf's time included --
    and the tree's length is the sum of its branches"""
    m = _structured(4, [0, 1, 1, 0], [0.0, 0.0, 2000.0, 20000.0])      # (the last one enters after the join, where everybody is: in population 0)
    model = mca.Model(m)
    rng = random.Random(2)
    for _ in range(300):
        g = mca.ARG(model, rng)
        for _ in range(12):
            assert g.height[:4] == model.stime
            total = 0.0
            for v in range(7):
                if v == g.root:
                    assert g.parent[v] < 0
                    continue
                assert g.height[g.parent[v]] > g.height[v], (v, g.height)
                total += g.height[g.parent[v]] - g.height[v]
            assert abs(total - g.ltree) <= 1e-9 * total and abs(sum(g.lepoch) - g.ltree) <= 1e-9 * total
            g.recombine()


def test_refuses_times_the_front_end_does_not_write():
    for bad in ([0.0, 1000.0, 2000.0], [0.0, 2000.0, 0.0], [2000.0, 2000.0, 20000.0]):
        with pytest.raises(AssertionError):
            mca.Model(_structured(3, [0, 1, 1], bad))


def test_fixture_is_usable():
    """what mc_model_check.golden_is_usable demands of a fixture, on this one"""
    import mc_model_check as mc
    gold = json.load(open(os.path.join(ROOT, "tests/golden/mc_model_ancient.json")))["cases"]
    assert sorted(gold) == ["a3", "a4"]
    added = [k for k in gold if k not in mc.GOLD]
    mc.GOLD.update({k: gold[k] for k in added})
    try:
        for case in gold:
            g = gold[case]
            assert max(g["model"]["sample_times"]) > 0 and len(g["rows"]["start"]) <= 15
            mc.golden_is_usable(case)
    finally:
        for k in added:
            mc.GOLD.pop(k, None)
