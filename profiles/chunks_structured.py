#!/usr/bin/env python
"""K chunks of the structured bench shape (bench.build_workload: --nsam 8 --pops 2 --np 20000, same seeds as bench.py) filtered
three ways in one session, after a warm-up of each:

  (a) one after the other (pf_run per chunk: what bin/smcsmc -chunks K did for structured models),
  (b) in lockstep (pf_run_many: one k_sweep_xmp and one k_sweep_blc launch per row for all chunks),
  (c) a host thread and stream per chunk (what bench.py --pops 2 --chunks-per-gpu K does).

The three are alternated `--reps` times; each timed window ends in a synchronise of every filter.  Every mode must give the
same log-likelihoods, bit for bit.  Prints one JSON line per K.

    python profiles/chunks_structured.py --chunks 1 2 4 8 --length 4e6 --log-cap 4096 --reps 2

--log-cap: at the library's default (16 384 records per slot) the event log of one filter of this shape is about 31 GB; eight
filters need a smaller ring (too small a ring is a reported error, not a wrong result)."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--np", type=int, default=20000)
    ap.add_argument("--nsam", type=int, default=8)
    ap.add_argument("--pops", type=int, default=2)
    ap.add_argument("--length", type=float, default=4e6)
    ap.add_argument("--epochs", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log-cap", type=int, default=4096)
    ap.add_argument("--count-wgs", type=int, default=0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--modes", default="abc")
    args = ap.parse_args()
    args.device = 0
    from smcsmc_amd import ParticleFilter
    kmax = max(args.chunks)
    chunks = []
    for k in range(kmax):
        model, segs = bench.build_workload(args, seed=args.seed + k)
        f = ParticleFilter(model, args.np, ess_fraction=0.5, seed=args.seed + 1000 * k, max_trace_events=0, device=0,
                           local_recomb=True, count_wgs=args.count_wgs, log_cap=args.log_cap)
        f.load_segments(segs)
        chunks.append((f, segs))

    def one_after_the_other(cs):
        for f, sg in cs:
            bench.run_sweep(f, sg)

    def lockstep(cs):
        for f, sg in cs:
            f.init_prior(float(sg["start"][0]))
        if len(cs) > 1:
            ParticleFilter.run_many([f for f, _ in cs])
        else:
            cs[0][0].run()
        for f, _ in cs:
            f.finish()

    def threads(cs):
        th = [threading.Thread(target=bench.run_sweep, args=(f, sg)) for f, sg in cs]
        for t in th:
            t.start()
        for t in th:
            t.join()

    modes = {"a": ("one_after_the_other", one_after_the_other), "b": ("run_many", lockstep), "c": ("thread_per_chunk", threads)}
    for K in args.chunks:
        cs = chunks[:K]
        rows = sum(len(sg["start"]) for _, sg in cs)
        spent = {m: [] for m in args.modes}
        logl = {}
        for m in args.modes:                                # warm-up: every mode once at this K
            modes[m][1](cs)
            for f, _ in cs:
                f.sync()
            logl[m] = [np.float64(f.logl()).view(np.uint64) for f, _ in cs]
        for _ in range(args.reps):
            for m in args.modes:
                for f, _ in cs:
                    f.sync()
                t0 = time.perf_counter()
                modes[m][1](cs)
                for f, _ in cs:
                    f.sync()
                spent[m].append(time.perf_counter() - t0)
        same = all(logl[m] == logl[args.modes[0]] for m in args.modes)
        out = {"chunks": K, "rows": rows, "np": args.np, "nsam": args.nsam, "pops": args.pops, "length": args.length, "log_cap": args.log_cap,
               "count_wgs": args.count_wgs, "same_log_likelihoods": bool(same)}
        for m in args.modes:
            out[modes[m][0]] = {"segments_per_s": [rows / t for t in spent[m]], "best": rows / min(spent[m])}
        print(json.dumps(out), flush=True)
        if not same:
            raise SystemExit("the modes disagree on the log-likelihoods")


if __name__ == "__main__":
    main()
