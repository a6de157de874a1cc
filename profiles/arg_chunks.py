#!/usr/bin/env python
"""bin/smcsmc -arg -chunks K -ranks 1 (the chunks of one device in lockstep, one tree dump per chunk) against the only way to get
the same K dumps without it: K single-filter runs, one after the other, each on its own window (-startpos) with the chunk's seed.
The headline model (one population, 32 epochs, Np = 10 000, four haplotypes) over K x --chunk-length bases of data simulated on
the device.  Wall-clock time of the processes (start-up, ring allocation, readout and file writing included -- what a user waits
for) and the ring estimate every filter prints (" -arg: ... GiB").  Prints one JSON line.

    python profiles/arg_chunks.py --chunks 4 --chunk-length 5e6 --np 10000 --out /tmp/arg_chunks"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "bin", "smcsmc")


def timed(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("failed: %s\n%s" % (" ".join(cmd), (r.stderr + r.stdout)[-2000:]))
    gib = [float(x) for x in re.findall(r"-arg: event log of \d+ records per particle, \d+ generations \(([0-9.]+) GiB\)", r.stderr)]
    notes = [ln.strip() for ln in r.stderr.splitlines() if "chunk(s) ran" in ln or "fill the device" in ln]
    return dt, gib, notes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--chunk-length", type=float, default=5e6)
    ap.add_argument("--np", type=int, default=10000)
    ap.add_argument("--nsam", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=32)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default="/tmp/arg_chunks")
    args = ap.parse_args()
    from smcsmc_amd import simulate
    K, n, Lc = args.chunks, args.nsam, int(args.chunk_length)
    L = K * Lc
    N0, mu, rho = 1e4, 2.5e-8, 1e-8
    ct = simulate.default_epochs(args.epochs)
    os.makedirs(args.out, exist_ok=True)
    seg = os.path.join(args.out, "data.seg")
    simulate.write_seg(seg, simulate.simulate_seg_device(n, float(L), mu, rho, ct, np.full(args.epochs, N0), seed=1, nchunks=1, device=0)[0])

    def core(length):
        c = ["-N0", "%g" % N0, "-t", "%.10g" % (4 * N0 * mu * length), "-r", "%.10g" % (4 * N0 * rho * length), "%d" % length]
        for t in ct:
            c += ["-eN", "%.10g" % (t / (4 * N0)), "1"]
        return c

    common = ["-nsam", str(n), "-seg", seg, "-Np", str(args.np), "-tmax", "4", "-EM", "0", "-arg"]
    t_many, gib_many, notes = timed([BIN] + core(L) + common + ["-seed", str(args.seed), "-chunks", str(K), "-ranks", "1",
                                                                 "-o", os.path.join(args.out, "many")])
    singles = []
    for c in range(K):
        # chunk c of the chunked run: window [1 + c * Lc, 1 + (c + 1) * Lc), seed + c
        dt, gib, _ = timed([BIN] + core(Lc) + common + ["-seed", str(args.seed + c), "-startpos", str(1 + c * Lc),
                                                          "-o", os.path.join(args.out, "single%d" % c)])
        singles.append((dt, gib))
    same = []
    for c in range(K):
        a = open(os.path.join(args.out, "many.chunk%d.trees.gz" % c), "rb").read()
        b = open(os.path.join(args.out, "single%d.trees.gz" % c), "rb").read()
        same.append(a == b)
    print(json.dumps({"chunks": K, "chunk_length": Lc, "np": args.np, "nsam": n, "epochs": args.epochs,
                      "chunked_s": t_many, "chunked_ring_gib_per_filter": gib_many, "chunked_notes": notes,
                      "single_s": [s[0] for s in singles], "single_total_s": sum(s[0] for s in singles),
                      "single_ring_gib": [s[1] for s in singles], "same_tree_files": same}))


if __name__ == "__main__":
    main()
