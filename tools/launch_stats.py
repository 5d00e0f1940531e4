#!/usr/bin/env python3
"""Per-LAUNCH statistics from a rocprofv3 kernel trace: launches are keyed by (kernel, grid), so the three grouped chain
launches of a step, which share one kernel name, get a line each.   python3 tools/launch_stats.py <dir or kernel_trace.csv> [filter]"""
import csv
import glob
import os
import statistics
import sys

path = sys.argv[1]
want = sys.argv[2] if len(sys.argv) > 2 else ""
if os.path.isdir(path):
    path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))[0]
groups = {}
for r in csv.DictReader(open(path)):
    name = r["Kernel_Name"].replace("void ", "").replace("vgan::", "")
    if want in name:
        wg = int(r["Workgroup_Size_X"])
        groups.setdefault((name[:72], int(r["Grid_Size_X"]) // wg * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1), wg), []).append(
            (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print(f'{"calls":>7} {"mean":>8} {"median":>8} {"min":>7} {"max":>7}  kernel  workgroups x threads')
for (name, grid, wg), v in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
    if len(v) >= 10:
        print(f"{len(v):7d} {statistics.fmean(v):8.2f} {statistics.median(v):8.2f} {min(v):7.2f} {max(v):7.2f}  {name}  {grid}x{wg}")
