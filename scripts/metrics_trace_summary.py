#!/usr/bin/env python3
"""Per-call kernel times of probaforms_amd.metrics from a rocprofv3 --kernel-trace CSV of scripts/metrics_time.py:
dispatches in order, one call = k_mmd_init ... k_mmd_final or k_mean_partial ... k_cov_final; prints each
kernel's time per call and the call's kernel total (the shapes are those metrics_time.py runs, in its order).

    python scripts/metrics_trace_summary.py <prefix>_kernel_trace.csv
"""
import csv
import re
import sys


def short(name):
    m = re.search(r"(k_[a-z_0-9]+)", name)
    return m.group(1) if m else name.split("(")[0]


def main(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        k = short(r["Kernel_Name"])
        if not k.startswith("k_"):
            continue
        if k in ("k_mmd_init", "k_mean_partial"):
            cur = {"kind": "mmd" if k == "k_mmd_init" else "fd", "kernels": {}, "grid": None}
            calls.append(cur)
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        n, t = cur["kernels"].get(k, (0, 0.0))
        cur["kernels"][k] = (n + 1, t + us)
        if k in ("k_mmd_hist", "k_cov_partial") and cur["grid"] is None:
            cur["grid"] = (int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]))
    for i, c in enumerate(calls):
        tot = sum(t for _, t in c["kernels"].values())
        parts = ", ".join("%s %dx %.1f us" % (k, n, t) for k, (n, t) in c["kernels"].items())
        print("call %2d %-3s workgroups %s: kernels %.3f ms = %s" % (i, c["kind"], c["grid"], tot / 1e3, parts))


if __name__ == "__main__":
    main(sys.argv[1])
