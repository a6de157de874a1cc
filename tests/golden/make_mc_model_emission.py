#!/usr/bin/env python3
"""Generates tests/golden/mc_model_emission.json: make_mc_model.py for the two model flags that enter the weight of a site
(dephase, ancestral_aware) and for unphased marks, by brute force with tests/mc_model.py -- plain Python: no reference code,
no oracle, no device.

    python tests/golden/make_mc_model_emission.py [--procs 7] [--only NAME] [--pilot]      (CPU only; minutes on 7 cores)

Every case takes the model and the stored rows of a case of tests/golden/mc_model.json (its twin, which has no flag and no
mark) and changes one thing, so that the twin's stored log p says what the flag is worth:

    n4b-aa           rows of n4b, ancestral_aware
    n4b-dephase      rows of n4b, dephase
    s4-dephase-aa    rows of s4, both flags
    s4-marks         rows of s4, no flag; the heterozygous pairs of every second site row rewritten as marks (2, 2)

The same chunked seeds (seed * 10007 + chunk, CHUNKS streams: the numbers do not depend on --procs) and the same layout of a
case as make_mc_model.py.  What the generator asserts of a case before it writes it: the conditions of
mc_model_check.golden_is_usable, and a distance of at least SEPARATION = 0.3 between its log p and the twin's -- ten times
mc_model_check.POWER_LOGP, the largest combined standard error the check admits, so that a filter which ignored the flag
would sit at |z| >= 10 however noisy it is within the cap.  tests/test_mc_model_emission_cpu.py (oracle) and
tests/test_gpu_mc_model_emission.py (device) hold the filter to these numbers.  --pilot prints a case from a fiftieth of
the draws and writes nothing.
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
import make_mc_model as mk  # noqa: E402
import mc_model  # noqa: E402

OUT = os.path.join(ROOT, "tests/golden/mc_model_emission.json")
TWINS = os.path.join(ROOT, "tests/golden/mc_model.json")
CHUNKS = mk.CHUNKS
SEPARATION = 0.3

# name: the twin in mc_model.json, model flags, every how many site rows the heterozygous pairs become marks (0: none), M, seed
CASES = {
    "n4b-aa":        dict(twin="n4b", flags=dict(ancestral_aware=True), mark_every=0, M=64 * 128000, seed=31),
    "n4b-dephase":   dict(twin="n4b", flags=dict(dephase=True), mark_every=0, M=64 * 48000, seed=32),
    "s4-dephase-aa": dict(twin="s4", flags=dict(dephase=True, ancestral_aware=True), mark_every=0, M=64 * 48000, seed=33),
    "s4-marks":      dict(twin="s4", flags=dict(), mark_every=2, M=64 * 48000, seed=34),
}


def twin(c):
    return json.load(open(TWINS))["cases"][c["twin"]]


def mark_rows(rows, every):
    """the heterozygous pairs (2k, 2k + 1) of every `every`-th site row, the first included, as marks (2, 2)"""
    al = np.array(rows["alleles"], np.int8).reshape(len(rows["start"]), -1)
    n = al.shape[1]
    sites = [s for s in range(len(al)) if int(rows["state"][s]) == 0]
    for s in sites[::every]:
        for i in range(0, n - 1, 2):
            if al[s, i] >= 0 and al[s, i + 1] >= 0 and al[s, i] != al[s, i + 1]:
                al[s, i] = al[s, i + 1] = 2
    return dict(rows, alleles=al)


def case_model(c):
    return dict(mk.model_from_json(twin(c)["model"]), **c["flags"])


def case_rows(c):
    rows = mk.rows_from_json(twin(c)["rows"])
    if c["mark_every"]:
        rows = mark_rows(rows, c["mark_every"])
    return {k: np.asarray(rows[k]) for k in ("start", "length", "state", "alleles", "max_record_epoch")}


def pairs_enumerated(m, rows):
    """per site row, the number of pairs whose phasings the weight averages over"""
    al = np.asarray(rows["alleles"]).reshape(len(rows["start"]), -1)
    out = []
    for s in range(len(al)):
        if int(rows["state"][s]) != 0:
            continue
        out.append(sum(1 for i in range(0, al.shape[1] - 1, 2)
                       if al[s, i] == 2 or (m.get("dephase") and sorted((al[s, i], al[s, i + 1])) == [0, 1])))
    return out


def _chunk(args):
    m, rows, M, seed = args
    return mc_model.accumulate(m, rows, M, seed)


def generate(name, procs, pilot=False):
    c = CASES[name]
    m = case_model(c)
    rows = case_rows(c)
    k = pairs_enumerated(m, rows)
    if "dephase" in c["flags"] or c["mark_every"]:
        assert sum(1 for x in k if x > 0) >= 2, "the case must average over phasings at more than one site"
    per = (c["M"] // CHUNKS) // (50 if pilot else 1)
    t0 = time.time()
    with mp.Pool(procs) as pool:
        parts = pool.map(_chunk, [(m, rows, per, c["seed"] * 10007 + j) for j in range(CHUNKS)], chunksize=1)
    r = mc_model.summarise(m, parts)
    tw = twin(c)
    return dict(model=mk.to_json(m), rows=mk.to_json(rows), M=r["M"], seed=c["seed"], chunks=CHUNKS, twin=c["twin"],
                twin_logp=tw["logp"], twin_logp_rse=tw["logp_rse"], separation=r["logp"] - tw["logp"], pairs_enumerated=k,
                logp=r["logp"], logp_rse=r["logp_rse"], weight_cv=r["cv"],
                stats={k_: v.tolist() for k_, v in r["stats"].items()}, se={k_: v.tolist() for k_, v in r["se"].items()},
                seconds=round(time.time() - t0, 1), procs=procs)


def check(name, r):
    """the conditions a case has to meet, the fixture alone"""
    import mc_model_check as chk
    assert abs(r["separation"]) >= SEPARATION, "%s: log p %.4f is %.4f from its twin's" % (name, r["logp"], r["separation"])
    had = name in chk.GOLD
    assert not had
    chk.GOLD[name] = r
    try:
        chk.golden_is_usable(name)
    finally:
        chk.GOLD.pop(name, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=7)
    ap.add_argument("--only", default=None)
    ap.add_argument("--pilot", action="store_true", help="a fiftieth of the draws, printed and not written")
    a = ap.parse_args()
    gold = json.load(open(OUT)) if os.path.exists(OUT) else {"cases": {}}
    for name in ([a.only] if a.only else list(CASES)):
        r = generate(name, a.procs, a.pilot)
        print(name, "rows", len(r["rows"]["start"]), "pairs enumerated per site", r["pairs_enumerated"], "M", r["M"],
              "logp %.4f +- %.4f" % (r["logp"], r["logp_rse"]), "twin %.4f +- %.4f" % (r["twin_logp"], r["twin_logp_rse"]),
              "separation %+.4f" % r["separation"], "cv %.1f" % r["weight_cv"],
              "draws for 1 %% on log p %.2g" % (r["weight_cv"] ** 2 / 1e-4), "%.0f s" % r["seconds"], flush=True)
        if a.pilot:
            for k in ("rec_count", "coal_count", "mig_count"):
                print("   ", k, np.round(np.array(r["stats"][k]), 3).tolist(), flush=True)
            continue
        check(name, r)
        gold["cases"][name] = r
        gold["cases"] = {k: gold["cases"][k] for k in CASES if k in gold["cases"]}
        with open(OUT, "w") as f:
            json.dump(gold, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
