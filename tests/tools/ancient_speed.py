"""A first speed figure for ancient samples: segments/s of one sweep at n = 8, two populations, Np 20 000 with four
ancient samples, and beside it the same model with all-zero sample times, which takes the same path (General, LDS-tree structured kernels).  The
model without times, on the path it has by default, is printed as a third line for orientation.

The workload is bench.py's two-population one (build_workload: 32 epochs, data simulated on the device from the model without times -- the
site simulator refuses sample times -- and lags calibrated for that model); the four samples of the second population enter at the first
epoch start at or after 2 000 generations, well below the split at 20 000.  Variants alternate, one warm-up sweep each, `--runs` timed
sweeps each; the median is the figure.

    python tests/tools/ancient_speed.py [--length 5e6] [--runs 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=float, default=5e6)
    ap.add_argument("--np", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from smcsmc_amd import ParticleFilter
    n = 8
    w = argparse.Namespace(nsam=n, length=a.length, epochs=32, pops=2, host_data=False, uncalibrated_lags=False, device=0)
    model, segs = bench.build_workload(w, seed=a.seed)
    ct = np.asarray(model["change_times"], float)
    t_anc = float(ct[np.searchsorted(ct, 2000.0)])
    assert list(model["sample_pops"]) == [0] * 4 + [1] * 4 and 0 < t_anc < 20000.0
    variants = [("four ancient samples", dict(model, sample_times=[0.0] * 4 + [t_anc] * 4)),
                ("all-zero times", dict(model, sample_times=[0.0] * n)),
                ("no times (default path)", model)]
    fs = []
    try:
        for name, m in variants:
            f = ParticleFilter(m, a.np, ess_fraction=0.5, seed=a.seed + 1000, max_trace_events=0)
            f.load_segments(segs)
            fs.append(f)
            bench.run_sweep(f, segs); f.sync()                 # warm-up
        S = len(segs["start"])
        dt = {name: [] for name, _ in variants}
        for _ in range(a.runs):
            for (name, _), f in zip(variants, fs):
                t0 = time.perf_counter()
                bench.run_sweep(f, segs); f.sync()
                dt[name].append(time.perf_counter() - t0)
        out = dict(nsam=n, pops=2, np=a.np, segments=S, length=a.length, t_ancient=t_anc, runs=a.runs, variants={})
        for (name, _), f in zip(variants, fs):
            rate = sorted(S / np.array(dt[name]))
            out["variants"][name] = dict(path=str(f.run_path()), logl=f.logl(), segments_per_s=float(np.median(rate)), lo=float(rate[0]), hi=float(rate[-1]))
            print("%-26s %-10s %9.1f segments/s  (%.1f .. %.1f, %d sweeps of %d rows)  logl %.3f" %
                  (name, f.run_path(), np.median(rate), rate[0], rate[-1], a.runs, S, f.logl()))
    finally:
        for f in fs:
            f.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
