#!/usr/bin/env python3
"""The relayout call (modgpu_rekey_relayout_table_device: a table of segments that slide BOTH ways, moved in one pass of ten launches)
against the routes a caller had before it, and the move table call it shares its kernels with against another build of the library.
One process, one stream, HIP events recorded on that stream around every single pass; the variants alternate step by step so drift hits
all of them alike; every variant is run a second time under another name in the same rotation, and the spread of the two medians (A/A)
is recorded (tools/bench_common.py).  Rate unit: the payload bytes moved per pass.  One key, off_to = off_from + the segment's shift.

    shapes     splice1000   a 4 GiB part spliced at 1 000 evenly spaced places: the first edit takes 64 KiB + 5 out, every later one
                            alternately puts twice that in and takes it out again, so the 1 000 surviving segments slide
                            alternately DOWN and UP by 64 KiB + 5
                 relayout,relayout2   the call
                 split,split2         two modgpu_rekey_move_table_device calls on tables split on the host (the downward entries, then
                                      the upward ones).  BAR: relayout / split <= 1 + the run's A/A spread
                 copy,copy2           modgpu_rekey_table_device into a second buffer, then one device-to-device copy back
               down1000     1 000 removed files of 64 KiB + 5 (bench_rekey_move_table.py's seg1000): a pure-down table through the move
                            table call (`move`) and through the relayout call (`relayout`), whose second sweep is idle -- its cost
               unchanged    modgpu_rekey_move_table_device on that table, this build against --other-lib (the parent commit's
                            libmodgpu.so), interleaved.  BAR: |this / other - 1| within the run's A/A spread

    python tools/bench_rekey_relayout.py [--shapes ...] [--other-lib PATH] [--warmup 2] [--steps 10] [--out profiles/r21_relayout.json]
"""
import ctypes

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY = M.KEY_PS4
OFF = (1 << 32) + (1 << 28)
PART = 4 << 30
FILE = 65536 + 5
EDITS = 1000
ALL_SHAPES = "splice1000,down1000,unchanged"
_vp = ctypes.c_void_p


def splice_edits():
    """the first edit takes FILE bytes out at offset 0, every later one alternately puts 2 * FILE in and takes 2 * FILE out"""
    pitch = PART // EDITS
    return [(0, FILE, 0)] + [(i * pitch, 0, 2 * FILE) if i % 2 else (i * pitch, 2 * FILE, 0) for i in range(1, EDITS)]


def resident(t):
    b = M.DeviceBuffer(t.nbytes)
    b.upload(t.view(np.uint8))
    return b


def splice(st, a):
    moves, new_size, _ = M.splice_moves(PART, splice_edits())
    part, other = M.DeviceBuffer(PART + 2 * FILE + 64), M.DeviceBuffer(PART + 2 * FILE + 64)
    H.fill(part, PART)
    t = M.relayout_table(part.ptr, moves, KEY, part_off=OFF)
    M.rekey_relayout_table_validate(t)
    up = t["dst"] > t["src"]
    assert int(up.sum()) == EDITS // 2 and int((t["dst"] < t["src"]).sum()) == EDITS // 2 and not (up[1:] == up[:-1]).any()
    halves = [t[~up], t[up]]
    for h in halves:
        M.rekey_move_table_validate(h)
    total = int(t["n"].sum())
    out_of_place = t.copy()
    out_of_place["dst"] = t["dst"] - np.uint64(part.ptr) + np.uint64(other.ptr)
    tabs = {"relayout": resident(t), "down": resident(halves[0]), "up": resident(halves[1]), "copy": resident(out_of_place)}
    ws = M.DeviceBuffer(M.rekey_move_table_workspace_bytes(t.size, total))
    ws_copy = M.DeviceBuffer(M.rekey_table_workspace_bytes(t.size))
    lo, hi = int(t["dst"].min()) - part.ptr, int((t["dst"] + t["n"]).max()) - part.ptr

    def one_pass(v):
        v = v.rstrip("2")
        if v == "relayout":
            M.rekey_relayout_table_device(tabs["relayout"], total, ws, n=t.size, stream=st.handle)
        elif v == "split":
            for name, h in zip(("down", "up"), halves):
                M.rekey_move_table_device(tabs[name], int(h["n"].sum()), ws, n=h.size, stream=st.handle)
        else:
            M.rekey_table_device(tabs["copy"], ws_copy, n=t.size, stream=st.handle)
            _ok(hip().hipMemcpyAsync(_vp(part.ptr + lo), _vp(other.ptr + lo), ctypes.c_size_t(hi - lo), 3, _vp(st.handle)), "hipMemcpyAsync")  # 3 = device to device
        return M.last_launch()

    variants = ["relayout", "split", "copy", "relayout2", "split2", "copy2"]
    times, info, launches = H.measure(st, variants, one_pass, a.warmup, a.steps)
    st.sync()
    assert M.rekey_move_table_status(ws) == (None, None) and M.table_status(ws_copy) is None
    row = {"bytes": total, "entries": int(t.size), "new_size": new_size, "launch": {v: info[v] for v in variants[:3]},
           "launches_per_pass": {v: launches[v] for v in variants[:3]}}
    for v in variants:
        row[v] = H.stats(times[v], total, 1, "TBps")
    for v in variants[:3]:
        row[v + "_aa_spread"] = H.aa_spread(row, v)
    row["aa_spread"] = max(row[v + "_aa_spread"] for v in variants[:3])
    row["relayout_over_split"] = round(row["relayout"]["median_ms"] / row["split"]["median_ms"], 5)
    row["copy_over_relayout"] = round(row["copy"]["median_ms"] / row["relayout"]["median_ms"], 4)
    row["bar"] = {"rule": "relayout / split <= 1 + the run's A/A spread", "aa_spread": row["aa_spread"], "met": row["relayout_over_split"] <= 1 + row["aa_spread"]}
    for b in [part, other, ws, ws_copy] + list(tabs.values()):
        b.free()
    return row, variants[:3]


def pure_down(st, a, other_lib):
    """the pure-down table: move against relayout (other_lib None), or the move table call of this build against other_lib's"""
    pitch = PART // EDITS
    keep = [(i * pitch + FILE, pitch - FILE) for i in range(EDITS)]
    part = M.DeviceBuffer(PART + 64)
    H.fill(part, PART)
    t = M.compaction_table(part.ptr, keep, KEY, part_off=OFF)
    t["dst"] -= np.uint64(FILE)
    t["off_to"] -= np.uint64(FILE)
    M.rekey_move_table_validate(t)
    M.rekey_relayout_table_validate(t)
    total = int(t["n"].sum())
    tab = resident(t)
    ws = M.DeviceBuffer(M.rekey_move_table_workspace_bytes(t.size, total))
    L = M.lib()

    def one_pass(v):
        if v.startswith("relayout"):
            M.rekey_relayout_table_device(tab, total, ws, n=t.size, stream=st.handle)
        else:
            lib = other_lib if v.startswith("other") else L
            if lib.modgpu_rekey_move_table_device(_vp(tab.ptr), t.size, total, _vp(ws.ptr), ws.nbytes, -1, _vp(st.handle)):
                raise RuntimeError(v + " failed")
        return None if v.startswith("other") else M.last_launch()

    first = ["this", "other"] if other_lib else ["move", "relayout"]
    row = H.measure_with_aa(st, first + [v + "2" for v in first], one_pass, a.warmup, a.steps, total)
    st.sync()
    assert M.rekey_move_table_status(ws) == (None, None)
    row["entries"] = int(t.size)
    if other_lib:
        row["launch"] = {v: i for v, i in row["launch"].items() if i}
        row["this_over_other"] = round(row["this"]["median_ms"] / row["other"]["median_ms"], 5)
        row["bar"] = {"rule": "|this / other - 1| <= the run's A/A spread", "aa_spread": row["aa_spread"], "met": abs(row["this_over_other"] - 1) <= row["aa_spread"]}
    else:
        row["idle_sweep_us"] = round(1000 * (row["relayout"]["median_ms"] - row["move"]["median_ms"]), 2)
        row["idle_sweep_us_second_run"] = round(1000 * (row["relayout2"]["median_ms"] - row["move2"]["median_ms"]), 2)
    for b in (part, tab, ws):
        b.free()
    return row, first


def main():
    ap = H.arguments("r21_relayout.json", warmup=2, steps=10, shapes=ALL_SHAPES)
    ap.add_argument("--other-lib", default=None, help="another build's libmodgpu.so (the parent commit's) for `unchanged`")
    a = ap.parse_args()
    assert a.warmup >= 1 and a.steps >= 1
    st = Stream()
    rows = {}
    for shape in a.shapes.split(","):
        if shape == "unchanged" and not a.other_lib:
            print(shape, "skipped: no --other-lib")
            continue
        if shape == "splice1000":
            row, shown = splice(st, a)
        else:
            other = H.other_library(a.other_lib, ["modgpu_rekey_move_table_device"], M.lib()) if shape == "unchanged" else None
            row, shown = pure_down(st, a, other)
        rows[shape] = row
        print("%-10s " % shape + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps"]) for v in shown)
              + "  A/A %.2f %%" % (100 * row["aa_spread"]) + ("  idle sweep %.1f us" % row["idle_sweep_us"] if "idle_sweep_us" in row else "")
              + ("  bar %s" % row["bar"] if "bar" in row else ""), flush=True)
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_rekey_relayout.py", "TB/s of payload bytes moved per pass", a),
                            "key": KEY, "off_from": OFF, "part_bytes": PART, "file_bytes": FILE, "edits": EDITS,
                            "rekey_move_table_kernel_source_hash": M.rekey_move_table_kernel_source_hash(),
                            "rekey_table_kernel_source_hash": M.rekey_table_kernel_source_hash(), "shapes": rows})


if __name__ == "__main__":
    main()
