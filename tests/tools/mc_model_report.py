#!/usr/bin/env python3
"""The tables of profiles/round18/mc_model.md.

    python tests/tools/mc_model_report.py oracle [--procs 4]                  golden against oracle, per case and mode (CPU)
    python tests/tools/mc_model_report.py device                              the same for ParticleFilter (needs the GPU)
    python tests/tools/mc_model_report.py sensitivity [--procs 7] [--draws N] what the check can see (CPU, tests/mc_model.py alone)

The sensitivity table perturbs the *model* handed to tests/mc_model.py -- never a kernel, never the oracle -- and gives the
change of log p and of every compared statistic against the fixture in units of the test's combined standard error (the
fixture's and, in quadrature, the oracle's over the test's seeds in mode "rs", measured here), with the Monte Carlo error
of the perturbed run in the same units.  A shift of four units fails the test.
"""
import argparse
import math
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mc_model  # noqa: E402
import mc_model_check as chk  # noqa: E402


def z_table(kind, procs):
    print("| case | mode | golden log p | log mean Z | combined rel. s.e. | z | compared cells | largest cell s.e. | largest abs(z) of a cell |")
    print("|---|---|---|---|---|---|---|---|---|")
    pool = mp.Pool(procs) if kind == "oracle" else None
    for case in chk.CASES:
        for mode in chk.MODES:
            if kind == "oracle":
                r = pool.map(chk.oracle_run, [(case, mode, s) for s in chk.SEEDS])
                res = chk.combine(case, [x[0] for x in r], [x[1] for x in r], chk.MODES[mode][2])
            else:
                logl, counts, _ = chk.device_runs(case, mode)
                res = chk.combine(case, logl, counts, chk.MODES[mode][2])
            cells = res["cells"]
            worst = max(cells, key=lambda c: abs(c[4])) if cells else None
            print("| %s | %s | %.4f | %.4f | %.4f | %+.2f | %d | %s | %s |" % (
                case, mode, res["golden"], res["logz"], res["rse"], res["z"], len(cells),
                "%.3f" % max(c[3] for c in cells) if cells else "-",
                "%+.2f (%s)" % (worst[4], worst[0]) if worst else "-"), flush=True)


def perturbations(model):
    E = len(model["change_times"])
    P = int(model.get("n_pops", 1))
    out = [("rho x 1.25", dict(model, recombination_rate=model["recombination_rate"] * 1.25), {}),
           ("mu x 1.1", dict(model, mutation_rate=model["mutation_rate"] * 1.1), {})]
    ps = np.array(model["pop_sizes"], float).reshape(E, P).copy()
    ps[1] *= 1.3
    out.append(("size of epoch 1 x 1.3", dict(model, pop_sizes=ps if P > 1 else ps[:, 0]), {}))
    if P > 1:
        out.append(("migration rate x 2", dict(model, mig_rates=np.array(model["mig_rates"]) * 2.0), {}))
    out.append(("SMC instead of SMC' (no re-joining of the own stub)", model, dict(smc_prime=False)))
    if P > 1:
        out.append(("floating lineage started in the sample's population", model, dict(float_start="sample")))
    return out


def _chunk(a):
    m, rows, M, seed, kw = a
    return mc_model.accumulate(m, rows, M, seed, **kw)


def sensitivity(procs, draws, cases_, only=None):
    opool = mp.Pool(min(procs, 4))
    pool = mp.Pool(procs)
    for case in cases_:
        model, rows = chk.inputs(case)
        r = opool.map(chk.oracle_run, [(case, "rs", s) for s in chk.SEEDS])
        res = chk.combine(case, [x[0] for x in r], [x[1] for x in r], True)
        names, val, se, use = chk.golden_flat(case)
        unit = {c[0]: c[3] * c[1] for c in res["cells"]}            # combined s.e. of a cell, absolute
        print("\n**%s** (combined s.e. of log p in the test: %.4f)\n" % (case, res["rse"]))
        print("| perturbation | shift of log p / s.e. (its own error) | statistics moved by 4 s.e. or more | largest shift / s.e. |")
        print("|---|---|---|---|")
        for label, m, kw in perturbations(model):
            if only and only not in label:
                continue
            parts = pool.map(_chunk, [(m, rows, draws // 64, 77 * 10007 + k, kw) for k in range(64)], chunksize=1)
            s = mc_model.summarise(m, parts)
            K = ["rec_count", "rec_opp", "coal_count", "coal_opp"] + (["mig_count", "mig_opp"] if "mig_rates" in model else [])
            flat = np.concatenate([s["stats"][k].ravel() for k in K])
            ferr = np.concatenate([s["se"][k].ravel() for k in K])
            shifts = [(names[i], (flat[i] - val[i]) / unit[names[i]], ferr[i] / unit[names[i]]) for i in np.nonzero(use)[0]]
            big = [x for x in shifts if abs(x[1]) >= 4]
            top = max(shifts, key=lambda x: abs(x[1]))
            print("| %s | %+.1f (± %.1f) | %d of %d | %+.1f ± %.1f (%s) |" % (
                label, (s["logp"] - chk.GOLD[case]["logp"]) / res["rse"], s["logp_rse"] / res["rse"], len(big), len(shifts),
                top[1], top[2], top[0]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["oracle", "device", "sensitivity"])
    ap.add_argument("--procs", type=int, default=4)
    ap.add_argument("--draws", type=int, default=64 * 16000)
    ap.add_argument("--cases", default="n3,n4b,s4")
    ap.add_argument("--only", default=None, help="sensitivity: perturbations whose label contains this")
    a = ap.parse_args()
    if a.what == "sensitivity":
        sensitivity(a.procs, a.draws, a.cases.split(","), a.only)
    else:
        if a.what == "oracle":
            import oracle_lib
            oracle_lib.build()
        z_table(a.what, a.procs)


if __name__ == "__main__":
    main()
