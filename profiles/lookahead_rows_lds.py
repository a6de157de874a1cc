#!/usr/bin/env python
"""The look-ahead (-apf) at 9 to 16 haplotypes on the general kernels against the look-ahead in the extend role of the LDS-tree row
pipelines (pf_lookahead.flags bit 2, load_lookahead(..., lds=True)), in one session on one library.  The sibling of
profiles/lookahead_rows.py (one population, at most 8 haplotypes) and profiles/lookahead_rows_structured.py (structured, at most 8).

Workload: bench.build_workload (data from the device simulator, 32 epochs, calibrated lags), --pops populations, --nsam haplotypes,
--np particles, --length bases, look-ahead level --level.

--pops 2 to 4 (filters made with mp_rows=True), one chunk, three filters on the same data and seed:

  (a) look-ahead on the general kernels      k_extend_mp -> k_lookahead -> k_decide -> k_resample, counts and ledger on a second stream
  (b) look-ahead with the bit                k_sweep_xlmp<false, true> + k_sweep_blc: two launches a row
  (c) no look-ahead                          k_sweep_xlmp + k_sweep_blc (what the factor itself costs is b - c)

--pops 1 has no such comparison: pf_run of one chunk of 9 to 16 haplotypes stays on the general kernels with or without the bit.

Then, for any --pops, --chunks chunks (seeds of their own) one after the other with (a) against ParticleFilter.run_many with (b):
k_sweep_xl<false, true> for one population, k_sweep_xlmp<false, true> for structured models.

Before anything is timed (a) and (b) must agree: log-likelihood bit for bit, counts (migration statistics included) to 1e-9 of the
column scale.  Every variant is warmed up once, then the variants are alternated --reps times; a timed window is init_prior + run +
finish and ends in a synchronise.  One JSON line per measurement, microseconds a row in it.

    python profiles/lookahead_rows_lds.py --nsam 12 --pops 2 --np 20000 --length 1e6 --reps 3

The look-ahead records of a workload are packed on the host by smcsmc_amd.segments.pack_lookahead; that time is reported, not timed as
part of any variant."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

COUNT_KEYS = ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight")
MIG_KEYS = ("mig_count", "mig_opp", "mig_weight")


def workload(args, seed):
    from smcsmc_amd import segments as segmod
    a = argparse.Namespace(nsam=args.nsam, length=args.length, epochs=args.epochs, pops=args.pops, device=0)
    model, segs = bench.build_workload(a, seed=seed)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, al)))
            for s, l, st, al in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    t0 = time.perf_counter()
    la = segmod.pack_lookahead(rows, args.nsam)
    return model, segs, la, time.perf_counter() - t0


def new_filter(args, model, segs, la, tbl, variant, seed):
    from smcsmc_amd import ParticleFilter
    kw = dict(mp_rows=True) if args.pops > 1 else {}
    f = ParticleFilter(model, args.np, ess_fraction=0.5, seed=seed, max_trace_events=0, device=0, local_recomb=True, log_cap=args.log_cap, **kw)
    f.load_segments(segs)
    if variant == "a":
        f.load_lookahead(la, args.level, tbl)
    elif variant == "b":
        f.load_lookahead(la, args.level, tbl, lds=True)
    return f


def sweep(f, segs):
    f.init_prior(float(segs["start"][0]))
    f.run()
    f.finish()
    f.sync()


def spread(ts, rows):
    ts = sorted(ts)
    return {"us_per_row": {"min": 1e6 * ts[0] / rows, "median": 1e6 * ts[len(ts) // 2] / rows, "max": 1e6 * ts[-1] / rows},
            "segments_per_s": {"best": rows / ts[0], "median": rows / ts[len(ts) // 2], "worst": rows / ts[-1]}, "seconds": ts}


def agree(fa, fb):
    la, lb = np.float64(fa.logl()).view(np.uint64), np.float64(fb.logl()).view(np.uint64)
    ca, cb = fa.counts(), fb.counts()
    worst = 0.0
    for k in COUNT_KEYS + (MIG_KEYS if "mig_count" in ca else ()):
        scale = float(np.abs(ca[k]).max())
        if scale > 0:
            worst = max(worst, float(np.abs(np.asarray(ca[k]) - np.asarray(cb[k])).max()) / scale)
    return bool(la == lb), worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsam", type=int, default=12)
    ap.add_argument("--pops", type=int, default=2)
    ap.add_argument("--np", type=int, default=20000)
    ap.add_argument("--length", type=float, default=1e6)
    ap.add_argument("--epochs", type=int, default=32)
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log-cap", type=int, default=8192, help="pf_params.log_cap (20 000 particles x 16 384 records of 16 haplotypes are tens of GB a filter)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--variants", default="abc")
    ap.add_argument("--chunks", type=int, default=4, help="chunks of the lockstep comparison (0: skip it)")
    ap.add_argument("--chunks-length", type=float, default=None, help="bases per chunk of the lockstep comparison (default: --length)")
    ap.add_argument("--tbl-trees", type=int, default=200000)
    args = ap.parse_args()
    if not 9 <= args.nsam <= 16:
        raise SystemExit("--nsam 9 to 16: the bit means nothing below")
    from smcsmc_amd import ParticleFilter, pf

    if args.pops > 1:
        model, segs, la, pack_s = workload(args, args.seed)
        rows = len(segs["start"])
        tbl = pf.terminal_branch_quantiles(model, seed=1, n_trees=args.tbl_trees)
        fs = {v: new_filter(args, model, segs, la, tbl, v, args.seed) for v in args.variants}
        paths = {v: fs[v].run_path() for v in fs}
        for v in fs:                                         # warm-up, and what is compared before the clock starts
            sweep(fs[v], segs)
        head = {"nsam": args.nsam, "pops": args.pops, "np": args.np, "length": args.length, "level": args.level, "rows": rows, "paths": paths,
                "pack_lookahead_s": pack_s, "log_likelihood": {v: fs[v].logl() for v in fs}}
        if "a" in fs and "b" in fs:
            same, worst = agree(fs["a"], fs["b"])
            head.update(same_log_likelihood=same, worst_count_difference=worst)
            if not same or worst > 1e-9:
                print(json.dumps(head), flush=True)
                raise SystemExit("the two paths disagree: nothing is timed")
        spent = {v: [] for v in fs}
        for _ in range(args.reps):
            for v in fs:
                fs[v].sync()
                t0 = time.perf_counter()
                sweep(fs[v], segs)
                spent[v].append(time.perf_counter() - t0)
        head["rate"] = {v: spread(spent[v], rows) for v in fs}
        print(json.dumps(head), flush=True)
        for f in fs.values():
            f.close()

    if args.chunks > 0 and "a" in args.variants and "b" in args.variants:
        K = args.chunks
        if args.chunks_length:
            args.length = args.chunks_length
        cs = [workload(args, args.seed + 1 + k) for k in range(K)]
        tbl = pf.terminal_branch_quantiles(cs[0][0], seed=1, n_trees=args.tbl_trees)
        fa = [new_filter(args, m, sg, la, tbl, "a", args.seed + 1000 * k) for k, (m, sg, la, _) in enumerate(cs)]
        fb = [new_filter(args, m, sg, la, tbl, "b", args.seed + 1000 * k) for k, (m, sg, la, _) in enumerate(cs)]
        rows = sum(len(sg["start"]) for _, sg, _, _ in cs)

        def one_after_the_other():
            for f, (_, sg, _, _) in zip(fa, cs):
                sweep(f, sg)

        def lockstep():
            for f, (_, sg, _, _) in zip(fb, cs):
                f.init_prior(float(sg["start"][0]))
            ParticleFilter.run_many(fb)
            for f in fb:
                f.finish()
            for f in fb:
                f.sync()

        modes = {"one_after_the_other_general": one_after_the_other, "run_many_with_the_bit": lockstep}
        for fn in modes.values():
            fn()
        agreed = [agree(x, y) for x, y in zip(fa, fb)]
        out = {"chunks": K, "nsam": args.nsam, "pops": args.pops, "np": args.np, "length": args.length, "level": args.level, "rows": rows,
               "log_cap": args.log_cap, "can_run_many": bool(ParticleFilter.can_run_many(fb)), "path": fb[0].run_path(many=True),
               "same_log_likelihoods": all(s for s, _ in agreed), "worst_count_difference": max(w for _, w in agreed)}
        spent = {m: [] for m in modes}
        for _ in range(args.reps):
            for m, fn in modes.items():
                t0 = time.perf_counter()
                fn()
                spent[m].append(time.perf_counter() - t0)
        out["rate"] = {m: spread(spent[m], rows) for m in modes}
        print(json.dumps(out), flush=True)
        for f in fa + fb:
            f.close()


if __name__ == "__main__":
    main()
