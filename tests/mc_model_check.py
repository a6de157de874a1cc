"""The body shared by tests/test_mc_model_cpu.py (oracle) and tests/test_gpu_mc_model.py (device): the filter against
tests/golden/mc_model.json, the brute-force Monte Carlo statement of the model in tests/mc_model.py.

A particle filter's estimate of the normalising constant is unbiased at any number of particles, so over a fixed list of
seeds  log(mean_seeds exp(logl))  must equal the golden log p(data | model) within the two Monte Carlo errors -- with
resampling on or off, with focused sampling, a guide or the look-ahead, which change the proposal and not the target.
The counts of a run are a self-normalised mean over its particles; weighted with the run's exp(logl) they form the
ratio of two unbiased estimates (of Z E[s | data] and of Z), free of the O(1 / Np) bias a plain mean over seeds carries,
so  sum_seeds exp(logl) counts / sum_seeds exp(logl)  must equal the golden posterior expectation.

Tolerance: 4 combined standard errors (golden and filter in quadrature; the filter's from the spread over seeds, for the
ratio by the delta method).  Power: the combined relative standard error must not exceed 3 % for log p and 6 % for a
compared cell, or the check fails as "no power".  A cell is compared when its golden expectation is at least FLOOR events
(an opportunity cell: when the count it belongs to is).
"""
import functools
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import cases  # noqa: E402
import make_mc_model as mk  # noqa: E402

GOLD = json.load(open(os.path.join(ROOT, "tests/golden/mc_model.json")))["cases"]
CASES = list(mk.CASES)
FLOOR = 0.2
Z_MAX = 4.0
POWER_LOGP, POWER_CELL = 0.03, 0.06
SEEDS = list(range(101, 133))                    # 32 runs per case and mode
BIT_SEEDS = SEEDS[:2]
# mode: (ess_fraction, particles, statistics compared).  Without resampling a run is plain importance sampling from the
# prior: its weights have a coefficient of variation of 2 to 19 here, so log p needs more particles and the counts of such
# a run say nothing at this size.
MODES = {
    "is":     (0.0, 32000, False),
    "rs":     (0.9, 8000, True),
    "focus0": (0.9, 8000, True),
    "focus1": (0.9, 8000, True),
    "guide":  (0.9, 8000, True),
    "apf2":   (0.9, 8000, True),
}
COUNT_OF = {"rec_opp": "rec_count", "coal_opp": "coal_count"}


@functools.lru_cache(maxsize=None)
def inputs(case):
    g = GOLD[case]
    return mk.model_from_json(g["model"]), mk.rows_from_json(g["rows"])


def mode_model(case, mode):
    model, _ = inputs(case)
    E = len(model["change_times"])
    if mode.startswith("focus"):
        return dict(model, bias_heights=[400.0], bias_strengths=[5.0, 1.0], delay_type=int(mode[-1]),
                    application_delays=np.full(E, 1000.0))
    if mode == "guide":
        return dict(model, guide=cases.guide(model, 3, 2.0, 7), application_delays=np.full(E, 1000.0))
    return model


def lookahead_rows(case):
    from smcsmc_amd import segments as segmod
    model, segs = inputs(case)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    return segmod.pack_lookahead(rows, model["nsam"])


def flat_counts(c, P):
    keys = ["rec_count", "rec_opp", "coal_count", "coal_opp"] + (["mig_count", "mig_opp"] if P > 1 else [])
    return np.concatenate([np.asarray(c[k], float).ravel() for k in keys])


def golden_flat(case):
    g = GOLD[case]
    P = int(g["model"].get("n_pops", 1))
    E = len(g["model"]["change_times"])
    keys = ["rec_count", "rec_opp", "coal_count", "coal_opp"] + (["mig_count", "mig_opp"] if P > 1 else [])
    val = np.concatenate([np.asarray(g["stats"][k], float).ravel() for k in keys])
    se = np.concatenate([np.asarray(g["se"][k], float).ravel() for k in keys])
    names, use = [], []
    st = {k: np.asarray(g["stats"][k], float).reshape((E,) if k.startswith("rec") else (E, P, P) if k == "mig_count" else (E, P))
          for k in keys}
    for k in keys:
        for idx in np.ndindex(st[k].shape):
            names.append("%s%s" % (k, list(idx)))
            if k == "mig_opp":
                ev = max(st["coal_count"][idx], st["mig_count"][idx].sum())      # the lineage floats there at all
            else:
                ev = st[COUNT_OF.get(k, k)][idx]
            use.append(ev >= FLOOR)
    return names, val, se, np.array(use)


def golden_is_usable(case):
    """what the fixture alone must satisfy: its own precision, two compared cells per statistic, and in a structured case
    a compared migration count in every direction that has a rate"""
    g = GOLD[case]
    assert g["logp_rse"] <= 0.01, "log p of the fixture: relative s.e. %.4f" % g["logp_rse"]
    names, val, se, use = golden_flat(case)
    for k in ("rec_count", "rec_opp", "coal_count", "coal_opp") + (("mig_count", "mig_opp") if "mig_opp[0, 0]" in names else ()):
        cells = [i for i, nm in enumerate(names) if nm.startswith(k + "[") and use[i]]
        assert len(cells) >= 2, "%s: %d cells above the floor" % (k, len(cells))
    if "mig_rates" in g["model"]:
        mr = np.array(g["model"]["mig_rates"]); mc = np.array(g["stats"]["mig_count"])
        P = mr.shape[1]
        for a in range(P):
            for b in range(P):
                if mr[:, a, b].max() > 0:
                    assert (mc[:, a, b] >= FLOOR).any(), "no compared migration count %d -> %d" % (a, b)
    assert (se[use] / val[use]).max() <= POWER_CELL / 2, "a compared cell of the fixture is too noisy"
    assert (np.array(g["rows"]["max_record_epoch"]) == len(g["model"]["change_times"]) - 1).all()


def combine(case, logl, counts, with_stats):
    """logl [S], counts [S, K] of the runs -> dict(logz, rse, z, cells=[(name, golden, filter, rel. s.e., z)])"""
    g = GOLD[case]
    logl = np.asarray(logl, float)
    S = len(logl)
    w = np.exp(logl - logl.max())
    logz = logl.max() + math.log(w.mean())
    rse_f = float(w.std(ddof=1) / w.mean() / math.sqrt(S))
    rse = math.hypot(rse_f, g["logp_rse"])
    out = dict(logz=logz, golden=g["logp"], rse_filter=rse_f, rse=rse, z=(logz - g["logp"]) / rse, cells=[])
    if with_stats:
        names, val, se, use = golden_flat(case)
        c = np.asarray(counts, float)
        est = (w[:, None] * c).sum(0) / w.sum()
        var = ((w[:, None] * (c - est[None, :])) ** 2).sum(0) / w.sum() ** 2 * S / (S - 1)
        for i in np.nonzero(use)[0]:
            s_all = math.hypot(math.sqrt(var[i]), se[i])
            out["cells"].append((names[i], val[i], est[i], s_all / val[i], (est[i] - val[i]) / s_all))
    return out


def verdict(res, label):
    """the assertions of one case and mode, every figure printed first"""
    print("%s: log mean Z %.4f  golden %.4f  rel. s.e. %.4f (filter %.4f)  z %+.2f" %
          (label, res["logz"], res["golden"], res["rse"], res["rse_filter"], res["z"]))
    for nm, gv, fv, rs, z in res["cells"]:
        print("    %-20s golden %.6g  filter %.6g  rel. s.e. %.4f  z %+.2f" % (nm, gv, fv, rs, z))
    assert res["rse"] <= POWER_LOGP, "%s: no power, log p has a combined relative s.e. of %.4f" % (label, res["rse"])
    assert abs(res["z"]) <= Z_MAX, "%s: log mean Z %.4f against %.4f, z = %.2f" % (label, res["logz"], res["golden"], res["z"])
    weak = [(nm, rs) for nm, _, _, rs, _ in res["cells"] if rs > POWER_CELL]
    assert not weak, "%s: no power in %s" % (label, weak)
    off = [(nm, gv, fv, z) for nm, gv, fv, _, z in res["cells"] if abs(z) > Z_MAX]
    assert not off, "%s: %s" % (label, off)


# ---- the oracle, one run per task of a process pool
@functools.lru_cache(maxsize=None)
def _oracle_table(case):
    import oracle_lib
    return oracle_lib.terminal_branch_quantiles(inputs(case)[0], seed=1, n_trees=20000)


def oracle_run(args):
    case, mode, seed = args
    import oracle_lib
    model, rows = inputs(case)
    ess, Np, _ = MODES[mode]
    m = mode_model(case, mode)
    o = oracle_lib.Oracle(m, Np, ess_fraction=ess, seed=seed, max_trace_events=0)
    o.init_prior(rows["start"][0])
    sp = o.pack_segments(m, rows)
    if mode == "apf2":
        o.load_lookahead(lookahead_rows(case), 2, _oracle_table(case))
    o.run(sp)                                   # (finishes the sweep itself)
    out = (o.logl(), flat_counts(o.counts(), int(model.get("n_pops", 1))))
    o.close()
    return out


def oracle_check(pool, case, mode, seeds=SEEDS):
    r = pool.map(oracle_run, [(case, mode, s) for s in seeds])
    res = combine(case, [x[0] for x in r], [x[1] for x in r], MODES[mode][2])
    verdict(res, "%s %s oracle" % (case, mode))
    return res


# ---- the device: the seeds as chunks of run_many calls where the shape allows
@functools.lru_cache(maxsize=None)
def _device_table(case):
    from smcsmc_amd import pf
    return pf.terminal_branch_quantiles(inputs(case)[0], seed=1, n_trees=20000)


def device_runs(case, mode, seeds=SEEDS, group=8):
    from smcsmc_amd import ParticleFilter
    model, rows = inputs(case)
    P = int(model.get("n_pops", 1))
    ess, Np, _ = MODES[mode]
    m = mode_model(case, mode)
    logl, counts, paths = [], [], set()
    for k in range(0, len(seeds), group):
        fs = []
        try:
            for s in seeds[k:k + group]:
                # (a sweep of at most 15 rows: rings of 256 records a slot and 64 generations, not the megabyte a slot of the defaults)
                f = ParticleFilter(m, Np, ess_fraction=ess, seed=s, max_trace_events=0, log_cap=256, gen_cap=64)
                fs.append(f)
                f.init_prior(rows["start"][0]); f.load_segments(rows)
                if mode == "apf2":
                    f.load_lookahead(lookahead_rows(case), 2, _device_table(case), pipeline=P == 1, structured=P > 1)
            if ParticleFilter.can_run_many(fs):
                paths.add("many:" + str(fs[0].run_path(many=True)))
                ParticleFilter.run_many(fs)
            else:
                paths.add(str(fs[0].run_path()))
                for f in fs:
                    f.run()
            for f in fs:
                f.finish()
                logl.append(f.logl()); counts.append(flat_counts(f.counts(), P))
        finally:
            for f in fs:
                f.close()
    return logl, counts, paths


def device_check(case, mode):
    logl, counts, paths = device_runs(case, mode)
    res = combine(case, logl, counts, MODES[mode][2])
    verdict(res, "%s %s device %s" % (case, mode, sorted(paths)))
    return res, logl
