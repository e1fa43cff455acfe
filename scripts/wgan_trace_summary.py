#!/usr/bin/env python3
"""Kernel times and launch gaps of ConditionalWGAN.fit from a rocprofv3 --kernel-trace CSV of
`scripts/wgan_time.py --trace`: per traced fit (a fit begins at its first k_step after a pause of more than 1 ms, or
when the grid of k_step changes shape class), the count, mean and total time of each kernel, and the idle time
between consecutive kernels (end of one to start of the next) inside the fit.

    python scripts/wgan_trace_summary.py <prefix>_kernel_trace.csv
"""
import csv
import re
import statistics
import sys


def short(name):
    m = re.search(r"(k_[a-z_0-9]+)", name)
    return m.group(1) if m else name.split("(")[0]


def main(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    rows = [r for r in rows if short(r["Kernel_Name"]) in ("k_step", "k_finish", "k_eloss", "k_eloss_finish")]
    fits, cur, last_end = [], None, None
    for r in rows:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if cur is None or (last_end is not None and s - last_end > 1_000_000):
            cur = {"kernels": {}, "gaps": [], "t0": s}
            fits.append(cur)
        elif last_end is not None:
            cur["gaps"].append((s - last_end) / 1e3)
        k = short(r["Kernel_Name"])
        cur["kernels"].setdefault(k, []).append((e - s) / 1e3)
        if k == "k_step":
            cur.setdefault("wg", int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
        cur["t1"] = e
        last_end = e
    for i, f in enumerate(fits):
        span = (f["t1"] - f["t0"]) / 1e6
        busy = sum(sum(v) for v in f["kernels"].values()) / 1e3
        g = f["gaps"]
        print("fit %d: %.2f ms first dispatch to last end, kernels busy %.2f ms (%.0f %%), k_step grid %s workgroups"
              % (i, span, busy, 100 * busy / span, f.get("wg")))
        for k, v in f["kernels"].items():
            print("    %-15s %6d x  mean %7.2f us  median %7.2f us  total %8.2f ms" % (k, len(v), statistics.mean(v),
                                                                                    statistics.median(v), sum(v) / 1e3))
        if g:
            print("    launch gaps     %6d    mean %7.2f us  median %7.2f us  total %8.2f ms" % (
                len(g), statistics.mean(g), statistics.median(g), sum(g) / 1e3))


if __name__ == "__main__":
    main(sys.argv[1])
