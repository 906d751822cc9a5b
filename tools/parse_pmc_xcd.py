#!/usr/bin/env python3
"""Summarise tools/pmc_xcd.sh: busy cycles per XCD of the headline launch (the rows kernel's dispatches
with the largest grid), their max / mean and min / mean, and FETCH_SIZE per launch.

    python tools/parse_pmc_xcd.py prof_out/<out-name>
"""
import csv
import glob
import json
import os
import sys

KERNEL = "render_rows_kernel"


def main():
    out = sys.argv[1]
    res = {}
    for p in ("SQB", "TAB", "FETCH"):
        per = {}
        for f in glob.glob(os.path.join(out, p, "**", "*counter_collection.csv"), recursive=True):
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    if KERNEL not in r["Kernel_Name"]:
                        continue
                    d = per.setdefault((r["Dispatch_Id"], int(r["Grid_Size"])), {})
                    d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
        if not per:
            res[p] = None
            continue
        grid = max(g for _, g in per)
        sel = [v for (_, g), v in sorted(per.items()) if g == grid]
        names = sorted(sel[0])
        mean = {n: sum(d[n] for d in sel) / len(sel) for n in names}
        res[p] = {"grid": grid, "dispatches": len(sel), "mean": mean}
        if p != "FETCH":
            v = [mean[n] for n in names]
            res[p]["max_over_mean"] = max(v) / (sum(v) / len(v))
            res[p]["min_over_mean"] = min(v) / (sum(v) / len(v))
            res[p]["max_over_mean_each"] = [max(d.values()) / (sum(d.values()) / len(d)) for d in sel]
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
