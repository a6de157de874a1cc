#!/usr/bin/env python
"""One sweep of a structured model on the LDS-tree row kernel (9 to 16 haplotypes), with or without tree recording: what
-arg costs per launch of k_extend_mp (bench.build_workload: the bench's isolation-with-migration shape, same seeds).

    rocprofv3 --kernel-trace --stats -d OUT -o plain -- python profiles/arg_wide.py
    rocprofv3 --kernel-trace --stats -d OUT -o arg   -- python profiles/arg_wide.py --arg

One process per run; the kernel statistics of the two runs give k_extend_mp<false,false> against k_extend_mp<false,true>
on the same rows (the log-likelihoods of the two runs are equal bit for bit: the flag changes what is recorded, not the
sweep).  With --arg nothing in the rings may be overwritten: --log-cap records per slot (20 doubles each at n = 16) and four
times as many pieces (three doubles each), so keep --length short.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--np", type=int, default=10000)
    ap.add_argument("--nsam", type=int, default=16)
    ap.add_argument("--pops", type=int, default=2)
    ap.add_argument("--length", type=float, default=5e5)
    ap.add_argument("--epochs", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log-cap", type=int, default=32768)
    ap.add_argument("--gen-cap", type=int, default=8192)
    ap.add_argument("--arg", action="store_true")
    args = ap.parse_args()
    args.device = 0
    from smcsmc_amd import ParticleFilter
    model, segs = bench.build_workload(args, seed=args.seed)
    rows = len(segs["start"])
    kw = dict(record_trees=True, log_cap=args.log_cap, gen_cap=max(args.gen_cap, rows + 2)) if args.arg else dict(log_cap=args.log_cap)
    f = ParticleFilter(model, args.np, ess_fraction=0.5, seed=args.seed, max_trace_events=0, device=0, local_recomb=True, **kw)
    f.load_segments(segs)
    t0 = time.perf_counter()
    bench.run_sweep(f, segs)
    f.sync()
    dt = time.perf_counter() - t0
    out = {"arg": bool(args.arg), "nsam": args.nsam, "pops": args.pops, "np": args.np, "epochs": args.epochs, "length": args.length, "rows": rows,
           "seconds": dt, "segments_per_s": rows / dt, "log_likelihood": f.logl(), "log_likelihood_bits": "%016x" % int(np.float64(f.logl()).view(np.uint64)),
           "records": f.stats()["records"], "resamples": f.stats()["resamples"]}
    if args.arg:
        t1 = time.perf_counter()
        dump = f.sample_tree_events(pops=True)
        out["tree_events"] = len(dump[1])
        out["readout_seconds"] = time.perf_counter() - t1
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
