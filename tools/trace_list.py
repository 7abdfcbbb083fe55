#!/usr/bin/env python3
"""The kernels and copies of a rocprofv3 --kernel-trace --memory-copy-trace run in time order, in the format of
profiles/fleet_tick_trace.txt.  --after-gap MS: only what follows the last pause of at least MS milliseconds on the device
(a program that sleeps in front of the one call it wants listed).
Usage: python tools/trace_list.py DIR_WITH_CSVS [--after-gap 20] [--title TEXT]"""
import argparse
import csv
import glob
import os


def rows(pattern, root):
    for f in sorted(glob.glob(os.path.join(root, "**", pattern), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                yield r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("root")
    ap.add_argument("--after-gap", type=float, default=0.0)
    ap.add_argument("--title", default="")
    a = ap.parse_args()
    ev = []
    for r in rows("*kernel_trace.csv", a.root):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "kernel", name,
                   "grid %s wg %s" % (r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Workgroup_Size_X", r.get("Workgroup_Size", "?")))))
    for r in rows("*memory_copy_trace.csv", a.root):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy", r.get("Direction", r.get("Kind", "MEMORY_COPY")), ""))
    ev.sort()
    if a.after_gap > 0:
        cut = 0
        for i in range(1, len(ev)):
            if ev[i][0] - max(e[1] for e in ev[:i]) >= a.after_gap * 1e6:
                cut = i
        ev = ev[cut:]
    if a.title:
        print("== " + a.title)
    t0 = ev[0][0] if ev else 0
    for s, e, kind, name, extra in ev:
        print("%10.1f us  + %7.1f us  %-6s %-60s %s" % ((s - t0) / 1e3, (e - s) / 1e3, kind, name, extra))
    print("kernels: %s" % [n for _, _, k, n, _ in ev if k == "kernel"])


if __name__ == "__main__":
    main()
