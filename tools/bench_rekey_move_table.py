#!/usr/bin/env python3
"""The rekey move table call (modgpu_rekey_move_table_device: a table of segments moved with memmove rules in one pass) against the
route a caller had before it -- the same segments as k calls of modgpu_rekey_move_device in address order on one stream -- and against
rekeying the segments into a second buffer with modgpu_rekey_table_device and copying back; and the unchanged single calls against the
same calls of another build of the library.  One process, one stream, HIP events recorded on that stream around every single pass; the
variants alternate step by step so drift hits all of them alike; every variant is run a second time under another name in the same
rotation, and the spread of the two medians (A/A) is recorded (tools/bench_rekey_move.py's harness).  Rate unit: the payload bytes moved
per pass.  One key, off_to = off_from - the segment's shift: compacting a resident part.

    shapes     seg16 seg1000  a 4 GiB part with 16 / 1 000 evenly spaced removed files of 64 KiB + 5 each: as many surviving segments,
                              shifts growing from a chunk and 5 bytes to far above it
               one            one removed file at the start: one segment -- the table form against the single call
               cfg4           100 000 files of 42 949 bytes, every 100th removed: 99 000 entries
               rekey4g move4g modgpu_rekey_device_to / modgpu_rekey_move_device at 4 GiB, this build against --other-lib (the parent's
                              libmodgpu.so), interleaved
    variants   table,table2       the call at its shipped grid
               singles,singles2   k calls of modgpu_rekey_move_device.  BAR (seg1000): singles / table > 1 + the run's A/A spread
               copy,copy2         modgpu_rekey_table_device into a second buffer, then one device-to-device copy back
               this,this2 / other,other2   (rekey4g, move4g) BAR: |this / other - 1| within the run's A/A spread

    python tools/bench_rekey_move_table.py [--shapes ...] [--other-lib PATH] [--warmup 2] [--steps 10] [--out profiles/r15_move_table.json]
"""
import ctypes

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY = M.KEY_PS4
OFF = (1 << 32) + (1 << 28)
PART = 4 << 30
FILE = 65536 + 5
ALL_SHAPES = "seg16,seg1000,one,cfg4,rekey4g,move4g"
_vp = ctypes.c_void_p


def kept(shape):
    """the surviving (offset, n) ranges of the part"""
    if shape == "one":
        return [(FILE, PART - FILE)]
    if shape == "cfg4":
        size = PART // 100000
        return [(i * size, size) for i in range(100000) if i % 100 != 0]
    k = int(shape[3:])
    pitch = PART // k
    return [(i * pitch + FILE, pitch - FILE) for i in range(k)]


def against_other(L, O, shape, st, stv, a):
    n, d = 4 << 30, (64 << 20) + 5
    kk, k3 = M.as_int32(KEY), M.as_int32(M.KEY_PS3)
    src, dst = M.DeviceBuffer(n + d + 64), M.DeviceBuffer(n)
    ws = M.DeviceBuffer(M.move_workspace_bytes(n))
    H.fill(src, n + d)

    def one_pass(v):
        lib = O if v.startswith("other") else L
        if shape == "rekey4g":
            rc = lib.modgpu_rekey_device_to(_vp(dst.ptr), _vp(src.ptr), n, k3, 0, kk, 0, -1, stv)
        else:
            rc = lib.modgpu_rekey_move_device(_vp(src.ptr), _vp(src.ptr + d), n, kk, OFF, kk, OFF - d, _vp(ws.ptr), ws.nbytes, -1, stv)
        if rc:
            raise RuntimeError(shape + " failed")
        return None if lib is O else M.last_launch()

    row = H.measure_with_aa(st, ["this", "other", "this2", "other2"], one_pass, a.warmup, a.steps, n)
    row["this_over_other"] = round(row["this"]["median_ms"] / row["other"]["median_ms"], 5)
    row["bar"] = {"rule": "|this / other - 1| <= the run's A/A spread", "aa_spread": row["aa_spread"], "met": abs(row["this_over_other"] - 1) <= row["aa_spread"]}
    for b in (src, dst, ws):
        b.free()
    return row, ["this", "other"]


def main():
    ap = H.arguments("r15_move_table.json", warmup=2, steps=10, shapes=ALL_SHAPES)
    ap.add_argument("--other-lib", default=None, help="another build's libmodgpu.so (the parent commit's) for rekey4g and move4g")
    ap.add_argument("--singles-steps", type=int, default=3, help="steps of cfg4, whose 99 000 single calls take seconds per pass")
    a = ap.parse_args()
    assert a.warmup >= 1 and a.steps >= 1
    L = M.lib()
    st = Stream()
    stv = _vp(st.handle)
    kk = M.as_int32(KEY)
    rows = {}
    for shape in a.shapes.split(","):
        if shape in ("rekey4g", "move4g"):
            if not a.other_lib:
                print(shape, "skipped: no --other-lib")
                continue
            row, shown = against_other(L, H.other_library(a.other_lib, ["modgpu_rekey_device_to", "modgpu_rekey_move_device"], L), shape, st, stv, a)
        else:
            keep = kept(shape)
            part, other = M.DeviceBuffer(PART + 64), M.DeviceBuffer(PART + 64)
            H.fill(part, PART)
            # (compaction_table packs from the first kept range's offset; here the part BEGINS with a removed file, so the ranges are
            # packed from offset 0 and the first segment slides too)
            first = keep[0][0]
            t = M.compaction_table(part.ptr, keep, KEY, part_off=OFF)
            t["dst"] -= np.uint64(first)
            t["off_to"] -= np.uint64(first)
            M.rekey_move_table_validate(t)
            total = int(t["n"].sum())
            out_of_place = t.copy()
            out_of_place["dst"] = t["dst"] - np.uint64(part.ptr) + np.uint64(other.ptr)
            tables = {}
            for name, tab in (("table", t), ("copy", out_of_place)):
                tables[name] = M.DeviceBuffer(tab.nbytes)
                tables[name].upload(tab.view(np.uint8))
            ws = M.DeviceBuffer(M.rekey_move_table_workspace_bytes(t.size, total))
            ws_copy = M.DeviceBuffer(M.rekey_table_workspace_bytes(t.size))
            ws_single = M.DeviceBuffer(M.move_workspace_bytes(int(t["n"].max())))
            calls = [(_vp(int(e["dst"])), _vp(int(e["src"])), int(e["n"]), int(e["off_from"]), int(e["off_to"])) for e in t]

            def one_pass(v):
                v = v.rstrip("2")
                if v == "table":
                    M.rekey_move_table_device(tables["table"], total, ws, n=t.size, stream=st.handle)
                elif v == "singles":
                    for d, s, n, of, ot in calls:
                        if L.modgpu_rekey_move_device(d, s, n, kk, of, kk, ot, _vp(ws_single.ptr), ws_single.nbytes, -1, stv):
                            raise RuntimeError("single move failed")
                else:
                    M.rekey_table_device(tables["copy"], ws_copy, n=t.size, stream=st.handle)
                    _ok(hip().hipMemcpyAsync(_vp(part.ptr), _vp(other.ptr), ctypes.c_size_t(total), 3, stv), "hipMemcpyAsync")  # 3 = device to device
                return M.last_launch()

            variants = ["table", "singles", "copy", "table2", "singles2", "copy2"]
            row = H.measure_with_aa(st, variants, one_pass, 1 if shape == "cfg4" else a.warmup, a.singles_steps if shape == "cfg4" else a.steps, total)
            st.sync()
            assert M.rekey_move_table_status(ws) == (None, None) and M.move_status(ws_single) is None
            row["entries"] = int(t.size)
            row["singles_over_table"] = round(row["singles"]["median_ms"] / row["table"]["median_ms"], 4)
            row["copy_over_table"] = round(row["copy"]["median_ms"] / row["table"]["median_ms"], 4)
            if shape == "seg1000":
                row["bar"] = {"rule": "singles / table > 1 + the run's A/A spread", "aa_spread": row["aa_spread"], "met": row["singles_over_table"] > 1 + row["aa_spread"]}
            for b in [part, other, ws, ws_copy, ws_single] + list(tables.values()):
                b.free()
            shown = ["table", "singles", "copy"]
        rows[shape] = row
        print("%-8s " % shape + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps"]) for v in shown)
              + "  A/A %.2f %%" % (100 * row["aa_spread"]) + ("  bar %s" % row["bar"] if "bar" in row else ""), flush=True)
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_rekey_move_table.py", "TB/s of payload bytes moved per pass", a),
                            "singles_steps": a.singles_steps, "key": KEY, "off_from": OFF, "part_bytes": PART, "removed_file_bytes": FILE,
                            "rekey_move_table_kernel_source_hash": M.rekey_move_table_kernel_source_hash(),
                            "rekey_kernel_source_hash": M.rekey_kernel_source_hash(),
                            "rekey_table_kernel_source_hash": M.rekey_table_kernel_source_hash(), "shapes": rows})


if __name__ == "__main__":
    main()
