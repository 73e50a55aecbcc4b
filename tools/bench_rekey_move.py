#!/usr/bin/env python3
"""The move call (modgpu_rekey_move_device: rekey with memmove rules, destination and source overlapping) against the one-pass call on
disjoint buffers and against the route a caller had before, and the ordinary rekey call against the same call of another build of
the library.  One process, one stream, HIP events recorded on that stream around every single pass; the variants alternate step by
step so drift hits all of them alike; every variant is run a second time under another name in the same rotation, and the spread of
the two medians (A/A) is recorded.  Rate unit: n payload bytes per pass (DESIGN.md 4.7's: the bytes rekeyed).  The key pair is the
compaction one: one key, off_to = off_from - d.

    shapes     4g_64m5    4 GiB moved down by 64 MiB + 5 (closing a 64 MiB gap; funnel form, every chunk waits for two far below)
               4g_5       4 GiB moved down by 5 bytes (every chunk waits for its neighbour)
               64m_5 1m_5 64 MiB and 1 MiB moved down by 5 (report only: what the two extra launches and the copies cost)
               rekey4g    modgpu_rekey_device_to at 4 GiB, this build against --other-lib (the parent's libmodgpu.so), interleaved
    variants   move,move2 the call at its shipped grid
               one,one2   modgpu_rekey_device_to on disjoint buffers of the same size: the one-pass reference (ratio reported)
               old,old2   the route a caller had: modgpu_rekey_device_to into a second buffer, then a device-to-device copy back.
                          BAR: move must be faster than old by more than the run's A/A spread
               this,this2 / other,other2   (rekey4g) BAR: |this - other| / other within the run's A/A spread

    python tools/bench_rekey_move.py [--shapes ...] [--other-lib PATH] [--warmup 3] [--steps 20] [--out profiles/r14_move.json]
"""
import ctypes

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY = M.KEY_PS4
OFF = (1 << 32) + (1 << 28)
SHAPES = {"4g_64m5": (4 << 30, (64 << 20) + 5), "4g_5": (4 << 30, 5), "64m_5": (64 << 20, 5), "1m_5": (1 << 20, 5)}
ALL_SHAPES = "4g_64m5,4g_5,64m_5,1m_5,rekey4g"
_vp = ctypes.c_void_p


def main():
    ap = H.arguments("r14_move.json", shapes=ALL_SHAPES)
    ap.add_argument("--other-lib", default=None, help="another build's libmodgpu.so (the parent commit's) for rekey4g")
    a = ap.parse_args()
    assert a.warmup >= 1 and a.steps >= 1
    L = M.lib()
    st = Stream()
    stv = _vp(st.handle)
    kk = M.as_int32(KEY)
    rows = {}
    for shape in a.shapes.split(","):
        if shape == "rekey4g":
            if not a.other_lib:
                print("rekey4g skipped: no --other-lib")
                continue
            O = H.other_library(a.other_lib, ["modgpu_rekey_device_to"], L)
            n = 4 << 30
            src, dst = M.DeviceBuffer(n), M.DeviceBuffer(n)
            H.fill(src, n)
            k3 = M.as_int32(M.KEY_PS3)

            def one_pass(v):
                lib = O if v.startswith("other") else L
                if lib.modgpu_rekey_device_to(_vp(dst.ptr), _vp(src.ptr), n, k3, 0, kk, 0, -1, stv):
                    raise RuntimeError("rekey failed")
                return None if lib is O else M.last_launch()

            row = H.measure_with_aa(st, ["this", "other", "this2", "other2"], one_pass, a.warmup, a.steps, n)
            row["this_over_other"] = round(row["this"]["median_ms"] / row["other"]["median_ms"], 5)
            row["bar"] = {"rule": "|this / other - 1| <= the run's A/A spread", "aa_spread": row["aa_spread"],
                          "met": abs(row["this_over_other"] - 1) <= row["aa_spread"]}
            variants = ["this", "this2", "other", "other2"]
            src.free()
            dst.free()
        else:
            n, d = SHAPES[shape]
            part = M.DeviceBuffer(n + d + 64)   # the resident part: source at d, destination at 0
            other = M.DeviceBuffer(n + 64)      # disjoint destination / the old route's second buffer
            ws = M.DeviceBuffer(M.move_workspace_bytes(n))
            H.fill(part, n + d)

            def one_pass(v):
                v = v.rstrip("2")
                if v == "move":
                    M.rekey_move_device(part.ptr, part.ptr + d, n, KEY, KEY, OFF, OFF - d, ws, stream=st.handle)
                elif v == "one":
                    M.rekey_device_to(other.ptr, part.ptr + d, KEY, KEY, OFF, OFF - d, n=n, stream=st.handle)
                else:
                    M.rekey_device_to(other.ptr, part.ptr + d, KEY, KEY, OFF, OFF - d, n=n, stream=st.handle)
                    _ok(hip().hipMemcpyAsync(_vp(part.ptr), _vp(other.ptr), ctypes.c_size_t(n), 3, stv), "hipMemcpyAsync")  # 3 = device to device
                return M.last_launch()

            variants = ["move", "one", "old", "move2", "one2", "old2"]
            row = H.measure_with_aa(st, variants, one_pass, a.warmup, a.steps, n)
            st.sync()
            assert M.move_status(ws) is None
            row["shift"] = d
            row["move_over_one"] = round(row["move"]["median_ms"] / row["one"]["median_ms"], 4)
            row["old_over_move"] = round(row["old"]["median_ms"] / row["move"]["median_ms"], 4)
            if n >= 1 << 32:
                row["bar"] = {"rule": "old / move > 1 + the run's A/A spread", "aa_spread": row["aa_spread"], "met": row["old_over_move"] > 1 + row["aa_spread"]}
            for b in (part, other, ws):
                b.free()
        rows[shape] = row
        print("%-8s " % shape + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps"]) for v in variants if not v.endswith("2"))
              + "  A/A %.2f %%" % (100 * row["aa_spread"]) + ("  bar %s" % row["bar"] if "bar" in row else ""), flush=True)
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_rekey_move.py", "TB/s of n payload bytes per pass", a), "key": KEY, "off_from": OFF,
                            "rekey_kernel_source_hash": M.rekey_kernel_source_hash(), "kernel_source_hash": M.kernel_source_hash(),
                            "shapes": rows})


if __name__ == "__main__":
    main()
