#!/usr/bin/env python3
"""Generates tests/golden/mc_model.json: p(data | model) and the posterior expectation of every sufficient statistic of the
E-step on a few very small data sets, by brute force -- graphs drawn from the prior with tests/mc_model.py (plain Python: no
reference code, no oracle, no device) and weighted by the emission of the data.

    python tests/golden/make_mc_model.py [--procs 7] [--only NAME] [--pilot]      (CPU only; about ten minutes on 7 cores)

Per case the fixture holds the model, the packed rows, M, the seed, log p with its relative standard error, every expected
statistic with its standard error, the n = 2 case also the exact forward-backward answer of tests/exact_hmm2.py, and the
wall time.  The draws are made in CHUNKS independent streams (seed * 10007 + chunk), so the numbers do not depend on --procs.
One-population data come from smcsmc_amd.simulate.simulate_seg, structured data from the sampler itself run forward with
mutations; none from the device.  tests/test_mc_model_cpu.py (oracle) and tests/test_gpu_mc_model.py (device) hold the
filter to these numbers.

Unphased pairs and the flags dephase and ancestral_aware are stated in tests/mc_model.py and have a fixture of their own
(make_mc_model_emission.py, on the rows stored here).  The emission of partially missing rows (the tracked branch length) is
still not stated there, so no case has one.
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
import cases  # noqa: E402
import exact_hmm2  # noqa: E402
import mc_model  # noqa: E402
from smcsmc_amd import segments as segmod, simulate  # noqa: E402

OUT = os.path.join(ROOT, "tests/golden/mc_model.json")
CHUNKS = 64
CT = [0.0, 2000.0, 20000.0]
SIZES = [1.0, 0.4, 2.5]

# name: n, L, data seed, structure (None or dict(mig, one_way, pop_sizes factor per population, sample_pops)), M, seed
CASES = {
    "n2":  dict(n=2, L=10000, data_seed=5, M=64 * 8000, seed=11),
    "n3":  dict(n=3, L=8000, data_seed=3, M=64 * 32000, seed=12),
    "n4a": dict(n=4, L=5000, data_seed=2, M=64 * 48000, seed=13),
    "n4b": dict(n=4, L=5000, data_seed=4, M=64 * 128000, seed=14),
    "s2":  dict(n=2, L=5000, data_seed=8, M=64 * 16000, seed=15,
                structure=dict(mig=2.0, one_way=False, sizes=[1.0, 1.0], sample_pops=[0, 1])),
    "s4":  dict(n=4, L=4000, data_seed=6, M=64 * 32000, seed=16,
                structure=dict(mig=4.0, one_way=True, sizes=[1.0, 0.5], sample_pops=[0, 0, 1, 1])),
}


def case_model(c):
    m = cases.make_model(n=c["n"], E=len(CT), L=c["L"], lag=1e9, sizes=SIZES)
    m["change_times"] = np.array(CT)
    s = c.get("structure")
    if s:
        m = cases.make_structured(m, P=2, split_epoch=len(CT) - 1, mig=s["mig"], sample_pops=s["sample_pops"], sizes=s["sizes"])
        if s["one_way"]:
            m["mig_rates"][:, 1, 0] = 0.0      # backwards in time lineages move 0 -> 1 only, until population 1 joins 0
    return m


def case_rows(c, m):
    n, L = c["n"], c["L"]
    if c.get("structure"):
        pos, pat = mc_model.simulate_sites(m, c["data_seed"])
        seg = simulate.sites_to_seg(pos, pat, n, L)
    else:
        seg = simulate.simulate_seg(n, L, m["mutation_rate"], m["recombination_rate"], m["change_times"], m["pop_sizes"],
                                    seed=c["data_seed"])
    S = segmod.Segments.from_sites(seg["start"], seg["length"], seg["alleles"], n, L)
    rows = S.pack(m["lags"])
    assert (rows["max_record_epoch"] == len(CT) - 1).all(), "every row must record every epoch"
    return {k: np.asarray(rows[k]) for k in ("start", "length", "state", "alleles", "max_record_epoch")}


def to_json(d):
    return {k: (np.asarray(v).tolist() if isinstance(v, (np.ndarray, list)) else v) for k, v in d.items()}


def model_from_json(j):
    """the model dictionary (numpy arrays) of a stored case"""
    m = dict(j)
    for k in ("change_times", "pop_sizes", "lags", "mig_rates", "single_mig"):
        if k in m:
            m[k] = np.array(m[k], float)
    return m


def rows_from_json(j):
    return dict(start=np.array(j["start"], float), length=np.array(j["length"], float), state=np.array(j["state"], np.int8),
                alleles=np.array(j["alleles"], np.int8), max_record_epoch=np.array(j["max_record_epoch"], np.int32))


def _chunk(args):
    m, rows, M, seed = args
    return mc_model.accumulate(m, rows, M, seed)


def generate(name, procs, pilot=False):
    c = CASES[name]
    m = case_model(c)
    rows = case_rows(c, m)
    per = (c["M"] // CHUNKS) // (50 if pilot else 1)
    t0 = time.time()
    with mp.Pool(procs) as pool:
        parts = pool.map(_chunk, [(m, rows, per, c["seed"] * 10007 + k) for k in range(CHUNKS)], chunksize=1)
    r = mc_model.summarise(m, parts)
    out = dict(model=to_json(m), rows=to_json(rows), M=r["M"], seed=c["seed"], chunks=CHUNKS, data_seed=c["data_seed"],
               logp=r["logp"], logp_rse=r["logp_rse"], weight_cv=r["cv"],
               stats={k: v.tolist() for k, v in r["stats"].items()}, se={k: v.tolist() for k, v in r["se"].items()},
               seconds=round(time.time() - t0, 1), procs=procs)
    if name == "n2":
        h = {}
        for K in (300, 600):
            ex = exact_hmm2.ExactHMM2(m["change_times"], m["pop_sizes"], m["mutation_rate"], m["recombination_rate"], K=K)
            res = ex.run(rows, seq_len=m["loci_length"])
            h[K] = dict(logl=res["logl"], **{k: res[k].tolist() for k in ("rec_count", "rec_opp", "coal_count", "coal_opp")})
        out["exact"], out["exact_half_resolution"] = h[600], h[300]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=7)
    ap.add_argument("--only", default=None)
    ap.add_argument("--pilot", action="store_true", help="a fiftieth of the draws, printed and not written")
    a = ap.parse_args()
    gold = json.load(open(OUT)) if os.path.exists(OUT) else {"cases": {}}
    for name in ([a.only] if a.only else list(CASES)):
        r = generate(name, a.procs, a.pilot)
        print(name, "rows", len(r["rows"]["start"]), "M", r["M"], "logp %.4f +- %.4f" % (r["logp"], r["logp_rse"]),
              "cv %.1f" % r["weight_cv"], "%.0f s" % r["seconds"], flush=True)
        if not a.pilot:
            gold["cases"][name] = r
            gold["cases"] = {k: gold["cases"][k] for k in CASES if k in gold["cases"]}
            with open(OUT, "w") as f:
                json.dump(gold, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
