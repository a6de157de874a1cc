#!/usr/bin/env python3
"""Idle time between consecutive kernels of one queue, from a rocprofv3 --kernel-trace CSV (run on the GPU box, where the
raw trace lives): usage gaps.py <dir with *kernel_trace.csv> [--by-grid KERNEL].  Prints, per (previous kernel -> next kernel) pair of the
busiest queues, the number of transitions and the mean / median gap between the end of one and the start of the other.

--by-grid KERNEL (round 20: k_sweep_blc4): the launches of every kernel whose name contains KERNEL, grouped by the workgroups of
their grid's x dimension, with count, mean and median duration and the share of the kernel's time.  The second launch of a split step
is 1 + ledger workgroups + count workgroups of the epoch columns the row moves, so the grid says how many columns a row had and the
table says what a column costs."""
import csv
import glob
import statistics
import sys
from collections import defaultdict

args = sys.argv[1:]
by_grid = None
if "--by-grid" in args:
    i = args.index("--by-grid")
    by_grid = args[i + 1]
    del args[i:i + 2]
path = glob.glob(args[0] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = list(csv.DictReader(open(path)))
byq = defaultdict(list)
for r in rows:
    byq[r["Queue_Id"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0][:40]))
for q, ks in sorted(byq.items(), key=lambda kv: -len(kv[1]))[:3]:
    ks.sort()
    gaps = defaultdict(list)
    for (s0, e0, n0), (s1, e1, n1) in zip(ks, ks[1:]):
        gaps[(n0, n1)].append(s1 - e0)
    busy = sum(e - s for s, e, _ in ks)
    span = ks[-1][1] - ks[0][0]
    print("queue %s: %d kernels, busy %.1f ms of %.1f ms" % (q, len(ks), busy / 1e6, span / 1e6))
    for (a, b), g in sorted(gaps.items(), key=lambda kv: -len(kv[1]))[:6]:
        print("   %-40s -> %-40s n=%6d  gap mean %8.2f us  median %8.2f us" % (a, b, len(g), statistics.mean(g) / 1e3, statistics.median(g) / 1e3))

if by_grid:
    # (rocprofv3 gives the grid in work-items: workgroups = Grid_Size_X / Workgroup_Size_X)
    dur = defaultdict(list)
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        if by_grid not in name:                     # ("void k_sweep_blc4<true>": the name carries its return type)
            continue
        wgs = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
        dur[(name[:40], wgs, int(r["Grid_Size_Y"]))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = sum(sum(d) for d in dur.values())
    n_all = sum(len(d) for d in dur.values())
    print("%s by grid: %d launches, %.1f ms, mean %.2f us" % (by_grid, n_all, total / 1e6, total / 1e3 / max(1, n_all)))
    for (name, wgs, gy), d in sorted(dur.items()):
        print("   %-40s grid %5d x %d  n=%6d  mean %8.2f us  median %8.2f us  min %7.2f  max %8.2f  %5.1f %% of its time" %
              (name, wgs, gy, len(d), statistics.mean(d) / 1e3, statistics.median(d) / 1e3, min(d) / 1e3, max(d) / 1e3, 100.0 * sum(d) / max(1, total)))
