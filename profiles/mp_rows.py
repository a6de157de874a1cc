#!/usr/bin/env python
"""Structured models of 9 to 16 haplotypes: the general kernels (five launches a row: the path of a handle made without the flag, and of
every such handle before the flag existed) against the row pipeline on the LDS tree (pf_params.flags bit 3, ParticleFilter(mp_rows=True):
k_sweep_xlmp + k_sweep_blc, two launches a row), in one process and one session.

Workload: bench.build_workload's isolation-with-migration model, data drawn on the device, calibrated lags; --pops 2 --np 20000
--epochs 32, --nsam 12 and 16.  For every sample size, after a warm-up of each mode, alternated --reps times:

  off_1      one chunk, flag off (the baseline)
  on_1       one chunk, flag on
  off_4      K chunks one after the other, flag off (the baseline for several chunks: what bin/smcsmc -chunks K does without -mp_rows)
  on_4_seq   K chunks one after the other, flag on
  on_4_many  K chunks in lockstep (pf_run_many), flag on

Each timed window ends in a synchronise of every filter.  The flag changes no filter result: every mode must give the same
log-likelihoods, bit for bit.  Prints one JSON line per sample size.

    python profiles/mp_rows.py --nsam 12 16 --length 1e6 --chunks 4 --reps 3

--rows-only N: run the first N rows of one chunk with the flag on and leave (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
profiles/mp_rows.py --nsam 16 --rows-only 600 [--off for the general kernels])."""
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
    ap.add_argument("--nsam", type=int, nargs="+", default=[12, 16])
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--np", type=int, default=20000)
    ap.add_argument("--pops", type=int, default=2)
    ap.add_argument("--length", type=float, default=1e6)
    ap.add_argument("--epochs", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log-cap", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows-only", type=int, default=0)
    ap.add_argument("--off", action="store_true")
    args = ap.parse_args()
    args.device = 0
    from smcsmc_amd import ParticleFilter

    def make(model, segs, k, mp_rows):
        f = ParticleFilter(model, args.np, ess_fraction=0.5, seed=args.seed + 1000 * k, max_trace_events=0, device=0, local_recomb=True,
                           log_cap=args.log_cap, mp_rows=mp_rows)
        f.load_segments(segs)
        return f

    for n in args.nsam:
        args_n = argparse.Namespace(**dict(vars(args), nsam=n))
        if args.rows_only:
            model, segs = bench.build_workload(args_n, seed=args.seed)
            f = make(model, segs, 0, not args.off)
            f.init_prior(float(segs["start"][0]))
            f.run(0, min(args.rows_only, f.n_segs)); f.sync()
            print(json.dumps({"nsam": n, "rows": min(args.rows_only, f.n_segs), "run_path": f.run_path()}), flush=True)
            f.close()
            continue
        work = [bench.build_workload(args_n, seed=args.seed + k) for k in range(args.chunks)]
        off = [make(m, sg, k, False) for k, (m, sg) in enumerate(work)]
        on = [make(m, sg, k, True) for k, (m, sg) in enumerate(work)]
        assert all(f.run_path() == "General" for f in off) and all(f.run_path() == "SweepXlmp" for f in on)
        assert ParticleFilter.can_run_many(on) and not ParticleFilter.can_run_many(off)
        segs = [sg for _, sg in work]

        def alone(fs):
            for f, sg in zip(fs, segs):
                bench.run_sweep(f, sg)

        def lockstep(fs):
            for f, sg in zip(fs, segs):
                f.init_prior(float(sg["start"][0]))
            ParticleFilter.run_many(fs)
            for f in fs:
                f.finish()

        modes = [("off_1", alone, off[:1]), ("on_1", alone, on[:1]), ("off_4", alone, off), ("on_4_seq", alone, on), ("on_4_many", lockstep, on)]
        rows = {name: sum(f.n_segs for f in fs) for name, _, fs in modes}
        logl, spent = {}, {name: [] for name, _, _ in modes}
        for name, fn, fs in modes:                         # warm-up: every mode once
            fn(fs)
            for f in fs:
                f.sync()
            logl[name] = [int(np.float64(f.logl()).view(np.uint64)) for f in fs]
        for _ in range(args.reps):
            for name, fn, fs in modes:
                for f in off + on:
                    f.sync()
                t0 = time.perf_counter()
                fn(fs)
                for f in fs:
                    f.sync()
                spent[name].append(time.perf_counter() - t0)
        same = all(logl[name] == logl["off_4"][:len(logl[name])] for name, _, _ in modes)
        out = {"nsam": n, "pops": args.pops, "np": args.np, "epochs": args.epochs, "length": args.length, "chunks": args.chunks,
               "log_cap": args.log_cap, "rows_per_chunk": [f.n_segs for f in on], "same_log_likelihoods": bool(same)}
        for name, _, _ in modes:
            out[name] = {"segments_per_s": [rows[name] / t for t in spent[name]], "best": rows[name] / min(spent[name]),
                         "us_per_row": 1e6 * min(spent[name]) / rows[name]}
        print(json.dumps(out), flush=True)
        for f in off + on:
            f.close()
        if not same:
            raise SystemExit("the modes disagree on the log-likelihoods")


if __name__ == "__main__":
    main()
