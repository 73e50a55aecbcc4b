#!/usr/bin/env python3
"""Median per launch of the memory-side request counters (rocprofv3 --pmc TCC_EA0_RDREQ_DRAM_sum TCC_EA0_WRREQ_DRAM_sum, a run of its own,
no tracing beside it) of the dominant modgpu_cycle_ kernel of each run under <dir>/<name>/: one JSON object on stdout.

    python tools/summarize_memside.py <dir>      # <dir>/parent, <dir>/branch, ...: one rocprofv3 -d directory per build
"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def main():
    root = sys.argv[1]
    out = {}
    for run in sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d))):
        per = defaultdict(lambda: defaultdict(float))  # kernel -> (dispatch, counter) -> value
        for f in glob.glob(os.path.join(root, run, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "modgpu_cycle_" in r["Kernel_Name"]:
                    per[r["Kernel_Name"]][(r["Dispatch_Id"], r["Counter_Name"])] += float(r["Counter_Value"])
        if not per:
            continue
        kernel = max(per, key=lambda k: sum(per[k].values()))
        names = sorted({c for _, c in per[kernel]})
        row = {"kernel": kernel, "launches": len({d for d, _ in per[kernel]})}
        for c in names:
            v = sorted(x for (_, cc), x in per[kernel].items() if cc == c)
            big = [x for x in v if x > 0.5 * v[-1]]  # the 4 GiB launches (not the device preparation's tiny ones)
            row[c] = {"median_per_launch": big[len(big) // 2], "launches_counted": len(big)}
        out[run] = row
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
