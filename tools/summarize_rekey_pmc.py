#!/usr/bin/env python3
"""Distil the rocprofv3 counter runs of tools/bench_rekey.py at 4 GiB (one run per counter set: FETCH_SIZE, WRITE_SIZE, the SQ
counters; never with tracing) into the "pmc" section of profiles/r08_rekey.json: per launch shape and source form, the median over
the launches of each counter, and which bound the pass sits on.

    python tools/summarize_rekey_pmc.py <dir with pmc_fetch/ pmc_write/ pmc_sq/> profiles/r08_rekey.json

The VALU figures: GRBM_GUI_ACTIVE sums the 8 XCDs, so a launch's cycles are GRBM_GUI_ACTIVE / 8.  SQ_INSTS_VALU counts wave
instructions; their issue cost depends on the mix (v_mad_u64_u32 takes longer than a 4-cycle instruction), so the cost per
instruction is taken from the shape that is VALU-bound by construction -- 200 workgroups, 800 SIMDs, each saturated -- and applied
to the other shape's count."""
import csv
import glob
import json
import os
import statistics
import sys
from collections import defaultdict

XCDS, SIMDS_ALL, SIMDS_QUEUE = 8, 1024, 800


def medians(root):
    out = defaultdict(dict)
    for path in glob.glob(os.path.join(root, "**", "*_counter_collection.csv"), recursive=True):
        vals = defaultdict(list)
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"]
            if "modgpu_cycle_rekey_kernel" in name or "modgpu_cycle_to_kernel" in name:
                key = "%s grid=%d" % (name.split("(")[0].replace("void ", ""), int(r["Grid_Size"]) // 1024)
                vals[(key, r["Counter_Name"])].append(float(r["Counter_Value"]))
        for (key, counter), v in vals.items():
            out[key][counter] = statistics.median(v)
    return out


def main():
    src, profile = sys.argv[1], sys.argv[2]
    m = medians(src)
    rec = json.load(open(profile))
    ms = {k: rec["sizes"][str(4 << 30)][k]["median_ms"] for k in ("fused_a", "fused_b", "fused_mis", "to_ceiling")}
    a = m["modgpu_cycle_rekey_kernel<4, 1024, false> grid=200"]
    b = m["modgpu_cycle_rekey_kernel<4, 1024, false> grid=256"]
    to = m["modgpu_cycle_to_kernel<4, 1024, false> grid=200"]
    cyc = {k: v["GRBM_GUI_ACTIVE"] / XCDS for k, v in m.items() if "GRBM_GUI_ACTIVE" in v}
    cost = cyc["modgpu_cycle_rekey_kernel<4, 1024, false> grid=200"] * SIMDS_QUEUE / a["SQ_INSTS_VALU"]
    wave_words = (4 << 30) / 16 / 64
    rec["pmc"] = {
        "size_bytes": 4 << 30,
        "counters_per_launch_median": m,
        "fetch_over_single_key_to_kernel": {k: round(v["FETCH_SIZE"] / to["FETCH_SIZE"], 4) for k, v in m.items() if "FETCH_SIZE" in v},
        "write_over_single_key_to_kernel": {k: round(v["WRITE_SIZE"] / to["WRITE_SIZE"], 4) for k, v in m.items() if "WRITE_SIZE" in v},
        "valu_instructions_per_wave_word": {k: round(v["SQ_INSTS_VALU"] / wave_words, 1) for k, v in m.items() if "SQ_INSTS_VALU" in v},
        "shader_clock_GHz": {"fused_a": round(cyc["modgpu_cycle_rekey_kernel<4, 1024, false> grid=200"] / ms["fused_a"] / 1e6, 3),
                             "fused_b": round(cyc["modgpu_cycle_rekey_kernel<4, 1024, false> grid=256"] / ms["fused_b"] / 1e6, 3)},
        "issue_cycles_per_valu_instruction_from_shape_a": round(cost, 2),
        "valu_busy_pct_shape_a_of_its_800_simds": 100.0,
        "valu_busy_pct_shape_b_of_all_1024_simds": round(100 * b["SQ_INSTS_VALU"] * cost / SIMDS_ALL / cyc["modgpu_cycle_rekey_kernel<4, 1024, false> grid=256"], 1),
        "valu_busy_pct_to_kernel_of_its_800_simds": round(100 * to["SQ_INSTS_VALU"] * cost / SIMDS_QUEUE / cyc["modgpu_cycle_to_kernel<4, 1024, false> grid=200"], 1),
        "shape_b_over_single_key_ceiling_time": round(ms["to_ceiling"] / ms["fused_b"], 4),
        "bound": ("shape (a), 200 workgroups: VALU -- its 800 SIMDs are saturated by construction of the cost figure, and it runs "
                  "%.1f %% slower than the HBM ceiling; shape (b), 256 workgroups: HBM -- %.4f x the single-key out-of-place pass's time "
                  "at the same bytes moved, with the VALU of all 1024 SIMDs %.1f %% busy"
                  % (100 * (ms["fused_a"] / ms["to_ceiling"] - 1), ms["fused_b"] / ms["to_ceiling"],
                     100 * b["SQ_INSTS_VALU"] * cost / SIMDS_ALL / cyc["modgpu_cycle_rekey_kernel<4, 1024, false> grid=256"])),
        "method": "tools/summarize_rekey_pmc.py over three rocprofv3 --pmc runs of tools/bench_rekey.py --sizes-mib 4096 "
                  "(FETCH_SIZE; WRITE_SIZE; SQ_WAVES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES GRBM_GUI_ACTIVE), "
                  "each alone, no tracing; FETCH_SIZE / WRITE_SIZE raw (KB) -- compared with the single-key kernel's at the same bytes; "
                  "times (clock, ceiling ratio) from the un-profiled run this file records",
    }
    with open(profile, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec["pmc"].items() if k != "counters_per_launch_median"}, indent=1))


if __name__ == "__main__":
    main()
