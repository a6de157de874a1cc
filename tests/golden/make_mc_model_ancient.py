#!/usr/bin/env python3
"""Generates tests/golden/mc_model_ancient.json: make_mc_model.py for models with samples that are not from the present
(sample_times, -eI), by brute force with tests/mc_model_ancient.py -- plain Python: no reference code, no oracle, no device.

    python tests/golden/make_mc_model_ancient.py [--procs 7] [--only NAME] [--pilot]      (CPU only; minutes on 7 cores)

The same epochs (CT), sizes (SIZES) and chunked seeds (seed * 10007 + chunk, CHUNKS streams: the numbers do not depend on
--procs) as make_mc_model.py, and the same layout of a case.  The data come from the sampler itself run forward with
mutations.  tests/test_gpu_ancient.py holds the device to these numbers, under the rules of tests/mc_model_check.py; the
fixture itself has to satisfy mc_model_check.golden_is_usable (tests/test_mc_model_ancient_cpu.py).  --pilot prints what that
needs to know about a case (weight CV, the draws for 1 % on log p, the cells above the floor) from a fiftieth of the draws.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import cases  # noqa: E402
import make_mc_model as mk  # noqa: E402
import mc_model_ancient  # noqa: E402
from smcsmc_amd import segments as segmod, simulate  # noqa: E402

OUT = os.path.join(ROOT, "tests/golden/mc_model_ancient.json")
CHUNKS, CT, SIZES = mk.CHUNKS, mk.CT, mk.SIZES

# name: n, L, data seed, sample populations and times, migration (4 N0 m; one_way: none from 1 to 0), sizes per population, M, seed
CASES = {
    "a3": dict(n=3, L=4000, data_seed=3, M=64 * 24000, seed=21,
               structure=dict(mig=4.0, one_way=False, sizes=[1.0, 1.0], sample_pops=[0, 1, 1], sample_times=[0.0, 0.0, 2000.0])),
    "a4": dict(n=4, L=4000, data_seed=6, M=64 * 32000, seed=22,
               structure=dict(mig=4.0, one_way=True, sizes=[1.0, 0.5], sample_pops=[0, 1, 0, 1],
                              sample_times=[0.0, 0.0, 2000.0, 2000.0])),
}


def case_model(c):
    s = c["structure"]
    m = cases.make_model(n=c["n"], E=len(CT), L=c["L"], lag=1e9, sizes=SIZES)
    m["change_times"] = np.array(CT)
    m = cases.make_structured(m, P=2, split_epoch=len(CT) - 1, mig=s["mig"], sample_pops=s["sample_pops"], sizes=s["sizes"])
    if s["one_way"]:
        m["mig_rates"][:, 1, 0] = 0.0      # backwards in time lineages move 0 -> 1 only, until population 1 joins 0
    m["sample_times"] = list(s["sample_times"])
    return m


def case_rows(c, m):
    n, L = c["n"], c["L"]
    pos, pat = mc_model_ancient.simulate_sites(m, c["data_seed"])
    seg = simulate.sites_to_seg(pos, pat, n, L)
    S = segmod.Segments.from_sites(seg["start"], seg["length"], seg["alleles"], n, L)
    rows = S.pack(m["lags"])
    assert (rows["max_record_epoch"] == len(CT) - 1).all(), "every row must record every epoch"
    return {k: np.asarray(rows[k]) for k in ("start", "length", "state", "alleles", "max_record_epoch")}


def _chunk(args):
    m, rows, M, seed = args
    return mc_model_ancient.accumulate(m, rows, M, seed)


def generate(name, procs, pilot=False):
    c = CASES[name]
    m = case_model(c)
    rows = case_rows(c, m)
    per = (c["M"] // CHUNKS) // (50 if pilot else 1)
    t0 = time.time()
    with mp.Pool(procs) as pool:
        parts = pool.map(_chunk, [(m, rows, per, c["seed"] * 10007 + k) for k in range(CHUNKS)], chunksize=1)
    r = mc_model_ancient.summarise(m, parts)
    return dict(model=mk.to_json(m), rows=mk.to_json(rows), M=r["M"], seed=c["seed"], chunks=CHUNKS, data_seed=c["data_seed"],
                logp=r["logp"], logp_rse=r["logp_rse"], weight_cv=r["cv"],
                stats={k: v.tolist() for k, v in r["stats"].items()}, se={k: v.tolist() for k, v in r["se"].items()},
                seconds=round(time.time() - t0, 1), procs=procs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=7)
    ap.add_argument("--only", default=None)
    ap.add_argument("--pilot", action="store_true", help="a fiftieth of the draws, printed and not written")
    a = ap.parse_args()
    gold = json.load(open(OUT)) if os.path.exists(OUT) else {"cases": {}}
    for name in ([a.only] if a.only else list(CASES)):
        r = generate(name, a.procs, a.pilot)
        print(name, "rows", len(r["rows"]["start"]), "sites", int((np.array(r["rows"]["state"]) == 0).sum()), "M", r["M"],
              "logp %.4f +- %.4f" % (r["logp"], r["logp_rse"]), "cv %.1f" % r["weight_cv"],
              "draws for 1 %% on log p %.2g" % (r["weight_cv"] ** 2 / 1e-4), "%.0f s" % r["seconds"], flush=True)
        if a.pilot:
            for k in ("rec_count", "coal_count", "mig_count"):
                print("   ", k, np.round(np.array(r["stats"][k]), 3).tolist(), flush=True)
        else:
            gold["cases"][name] = r
            gold["cases"] = {k: gold["cases"][k] for k in CASES if k in gold["cases"]}
            with open(OUT, "w") as f:
                json.dump(gold, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
