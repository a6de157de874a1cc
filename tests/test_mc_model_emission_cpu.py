"""The weight of a site under unphased marks, dephase and ancestral_aware, stated in tests/mc_model.py and held on the CPU: the statement
against a plain enumeration written here, the statement without marks and flags against the numbers it gave before it knew them, the
fixture tests/golden/mc_model_emission.json against the conditions of its generator, and the oracle against the fixture under the
rules of tests/mc_model_check.py (combine and verdict unchanged; tests/test_gpu_mc_model_emission.py applies them to the device).

Every case of the fixture takes the rows of a case of tests/golden/mc_model.json, its twin, and differs from it by one flag or by marks;
its log p lies at least 0.3 from the twin's -- ten times POWER_LOGP, the largest combined standard error the check admits -- so a filter
that ignored the flag would sit at |z| >= 10 however noisy it is within the cap."""
import itertools
import json
import multiprocessing as mp
import os
import random
import sys

import numpy as np
import pytest

import mc_model
import mc_model_check as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_mc_model_emission as mke  # noqa: E402

GOLD = json.load(open(os.path.join(ROOT, "tests/golden/mc_model_emission.json")))["cases"]
CASES = list(mke.CASES)
# modes: plain importance sampling and resampling for every case; the look-ahead, which changes the proposal and not the target, under dephase
CHECKS = [(c, m) for c in CASES for m in ("is", "rs")] + [("n4b-dephase", "apf2")]


@pytest.fixture(scope="module")
def gold():
    """the cases of this fixture under the rules of mc_model_check, which reads chk.GOLD; what was added is taken out again"""
    added = [k for k in GOLD if k not in chk.GOLD]
    chk.GOLD.update({k: GOLD[k] for k in added})
    try:
        yield GOLD
    finally:
        for k in added:
            chk.GOLD.pop(k, None)
        chk.inputs.cache_clear()


# ---------------------------------------------------------------------------------------------------------------
# the statement

def _tree(n, seed):
    m = chk.mk.model_from_json(chk.GOLD["n4b" if n == 4 else "n3"]["model"])
    return m, mc_model.ARG(mc_model.Model(m), random.Random(seed))


def test_without_marks_and_flags_the_statement_gives_the_numbers_it_gave():
    """sum w, sum w^2 and sum w s of 200 draws of the first chunk of three stored cases, as tests/mc_model.py returned them before it
    knew marks and flags (recorded then; the fixture tests/golden/mc_model.json was drawn with that code and stays as it is)"""
    was = {"n3": (12, "0x1.890739c6556fap-109", "0x1.9f9494b73dffbp-220", "0x1.873326c109cdep-81"),
           "n4b": (14, "0x1.e58dda683eefcp-134", "0x1.87c94c2130995p-269", "0x1.aeba4559f52b8p-106"),
           "s4": (16, "0x1.dc4157e477c4cp-153", "0x1.2d2021caed67cp-307", "0x1.f8d798ad56035p-124")}
    for case, (seed, w, w2, ws) in was.items():
        m, rows = chk.inputs(case)
        assert not m.get("dephase") and not m.get("ancestral_aware") and not (rows["alleles"] == 2).any()
        a = mc_model.accumulate(m, rows, 200, seed * 10007)
        got = (a[1][0], a[1][1], a[2].sum())
        np.testing.assert_allclose(got, [float.fromhex(x) for x in (w, w2, ws)], rtol=1e-13, err_msg=case)      # (an ulp of a library's exp)


def test_a_marked_site_weighs_the_mean_over_its_phasings():
    """site_likelihood against an enumeration with itertools: marks at one and at both pairs, dephase on pairs in either order beside a
    mark, and a homozygous pair left alone"""
    for seed in range(5):
        m, g = _tree(4, seed)
        pl = g.pruning_likelihood
        assert g.site_likelihood([2, 2, 0, 1]) == (pl([0, 1, 0, 1]) + pl([1, 0, 0, 1])) / 2
        both = [pl(list(a) + list(b)) for b, a in itertools.product(((0, 1), (1, 0)), repeat=2)]
        assert g.site_likelihood([2, 2, 2, 2]) == sum(both) / 4
        assert g.site_likelihood([1, 0, 0, 0]) == pl([1, 0, 0, 0]) and g.site_likelihood([1, 0, 0, 1]) == pl([1, 0, 0, 1])
        d = mc_model.ARG(mc_model.Model(dict(m, dephase=True)), random.Random(seed))
        assert d.height == g.height
        assert d.site_likelihood([1, 0, 0, 0]) == d.site_likelihood([0, 1, 0, 0]) == (pl([0, 1, 0, 0]) + pl([1, 0, 0, 0])) / 2
        assert d.site_likelihood([1, 0, 2, 2]) == d.site_likelihood([2, 2, 0, 1]) == sum(both) / 4
        assert d.site_likelihood([1, 1, 0, 0]) == pl([1, 1, 0, 0])
    m, g = _tree(3, 1)                                            # odd n: the last sample has no partner
    d = mc_model.ARG(mc_model.Model(dict(m, dephase=True)), random.Random(1))
    assert d.site_likelihood([0, 1, 1]) == (g.pruning_likelihood([0, 1, 1]) + g.pruning_likelihood([1, 0, 1])) / 2
    assert d.site_likelihood([0, 0, 1]) == g.pruning_likelihood([0, 0, 1])


def test_ancestral_aware_is_the_root_prior_one_zero():
    """the two root priors on one tree: 1/2 (a) + 1/2 (a with the alleles exchanged) is the likelihood under 1/2, 1/2; a site without
    a derived allele weighs more when 0 is known to be ancestral, a site with only derived alleles less"""
    for seed in range(5):
        m, g = _tree(4, seed)
        aa = mc_model.ARG(mc_model.Model(dict(m, ancestral_aware=True)), random.Random(seed))
        for al in ([1, 0, 0, 0], [0, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0]):
            flip = [1 - a for a in al]
            assert g.site_likelihood(al) == pytest.approx(0.5 * aa.site_likelihood(al) + 0.5 * aa.site_likelihood(flip), rel=1e-14)
        assert aa.site_likelihood([0, 0, 0, 0]) > g.site_likelihood([0, 0, 0, 0]) > aa.site_likelihood([1, 1, 1, 1])
        assert aa.site_likelihood([2, 2, 0, 0]) == (aa.pruning_likelihood([0, 1, 0, 0]) + aa.pruning_likelihood([1, 0, 0, 0])) / 2


def test_rows_that_are_not_stated_stay_refused():
    m = chk.mk.model_from_json(chk.GOLD["n4b"]["model"])
    model = mc_model.Model(m)
    row = lambda al: dict(start=[0.0], length=[100.0], state=[0], alleles=[al])     # noqa: E731
    mc_model.prepare_rows(model, row([2, 2, 0, 1]))
    for al in ([-1, 2, 0, 0], [2, 0, 0, 0], [1, 2, 0, 0], [0, 2, 2, 0]):
        with pytest.raises(ValueError):
            mc_model.prepare_rows(model, row(al))
    for al in ([-1, -1, 0, 1], [0, 1, 0, -1]):
        with pytest.raises(ValueError, match="some samples missing"):
            mc_model.prepare_rows(model, row(al))
    odd = mc_model.Model(chk.mk.model_from_json(chk.GOLD["n3"]["model"]))
    with pytest.raises(ValueError):
        mc_model.prepare_rows(odd, dict(start=[0.0], length=[100.0], state=[0], alleles=[[0, 1, 2]]))


# ---------------------------------------------------------------------------------------------------------------
# the fixture

@pytest.mark.parametrize("case", CASES)
def test_the_fixture_meets_its_generators_conditions(gold, case):
    g, c = gold[case], mke.CASES[case]
    print("%s: log p %.4f +- %.4f, twin %s %.4f +- %.4f, separation %+.4f, weight cv %.1f, M %d" %
          (case, g["logp"], g["logp_rse"], g["twin"], g["twin_logp"], g["twin_logp_rse"], g["separation"], g["weight_cv"], g["M"]))
    chk.golden_is_usable(case)
    twin = chk.GOLD[c["twin"]]
    assert g["twin"] == c["twin"] and g["twin_logp"] == twin["logp"]
    assert abs(g["logp"] - twin["logp"]) >= mke.SEPARATION == 10 * chk.POWER_LOGP
    assert (g["M"], g["seed"], g["chunks"]) == (c["M"], c["seed"], mke.CHUNKS)
    m, rows = mke.case_model(c), mke.case_rows(c)
    for k in ("start", "length", "state", "alleles", "max_record_epoch"):
        np.testing.assert_array_equal(np.asarray(g["rows"][k]), rows[k])
    assert bool(g["model"].get("dephase", False)) == bool(c["flags"].get("dephase", False))
    assert bool(g["model"].get("ancestral_aware", False)) == bool(c["flags"].get("ancestral_aware", False))
    for k in ("change_times", "pop_sizes", "mig_rates", "single_mig"):
        if k in m:
            np.testing.assert_array_equal(np.asarray(g["model"][k], float), np.asarray(m[k], float))
    al, tal = np.asarray(g["rows"]["alleles"]), np.asarray(twin["rows"]["alleles"])
    if c["mark_every"]:
        assert (al == 2).any() and ((al == 2) | (al == tal)).all()
        assert g["pairs_enumerated"] == mke.pairs_enumerated(m, rows) and sum(1 for x in g["pairs_enumerated"] if x) >= 2
    else:
        assert (al == tal).all()


# ---------------------------------------------------------------------------------------------------------------
# the oracle against the fixture

@pytest.fixture(scope="module")
def pool(oracle, gold):
    with mp.Pool(4) as p:
        yield p


@pytest.mark.parametrize("case,mode", CHECKS)
def test_the_oracle_targets_the_model_under_marks_and_flags(pool, case, mode):
    """32 seeds: log(mean exp(logl)) and (with resampling) the exp(logl)-weighted counts equal the fixture within 4 combined standard
    errors, at a combined relative standard error of at most 3 % (log p) and 6 % (a compared cell)"""
    chk.oracle_check(pool, case, mode)
