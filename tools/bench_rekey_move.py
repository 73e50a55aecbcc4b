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
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MODGPU_REQUIRE_GPU"] = "1"
import numpy as np  # noqa: E402
import modulate_amd as M  # noqa: E402
from hip_rt import Stream, hip, _ok  # noqa: E402  (tests/hip_rt.py: streams over the HIP runtime libmodgpu.so brought in)

KEY = M.KEY_PS4
OFF = (1 << 32) + (1 << 28)
SHAPES = {"4g_64m5": (4 << 30, (64 << 20) + 5), "4g_5": (4 << 30, 5), "64m_5": (64 << 20, 5), "1m_5": (1 << 20, 5)}
ALL_SHAPES = "4g_64m5,4g_5,64m_5,1m_5,rekey4g"
_vp = ctypes.c_void_p


class Event:
    def __init__(self):
        self.h = ctypes.c_void_p()
        _ok(hip().hipEventCreate(ctypes.byref(self.h)), "hipEventCreate")

    def record(self, stream):
        _ok(hip().hipEventRecord(self.h, ctypes.c_void_p(stream.handle)), "hipEventRecord")


def elapsed_ms(e0, e1):
    _ok(hip().hipEventSynchronize(e1.h), "hipEventSynchronize")
    ms = ctypes.c_float()
    _ok(hip().hipEventElapsedTime(ctypes.byref(ms), e0.h, e1.h), "hipEventElapsedTime")
    return ms.value


def fill(buf, n):
    tile = np.random.default_rng(1).integers(0, 256, size=1 << 24, dtype=np.uint8)
    for off in range(0, n, tile.size):
        buf.upload(tile[:min(tile.size, n - off)], offset=off)


def measure(variants, one_pass, st, warmup, steps, n):
    e0, e1 = Event(), Event()
    launch = {}
    for v in variants:
        for _ in range(warmup):
            launch[v] = one_pass(v)
        st.sync()
    times = {v: [] for v in variants}
    for _ in range(steps):
        for v in variants:
            e0.record(st)
            one_pass(v)
            e1.record(st)
            times[v].append(elapsed_ms(e0, e1))
    row = {"bytes": n, "launch": launch}
    for v in variants:
        tt = sorted(times[v])
        med = tt[len(tt) // 2]
        row[v] = {"median_ms": round(med, 5), "min_ms": round(tt[0], 5), "max_ms": round(tt[-1], 5), "TBps": round(n / (med * 1e-3) / 1e12, 4)}
    for v in variants:
        if not v.endswith("2"):
            a, b = row[v]["median_ms"], row[v + "2"]["median_ms"]
            row[v + "_aa_spread"] = round(abs(a - b) / min(a, b), 5)
    row["aa_spread"] = max(row[v + "_aa_spread"] for v in variants if not v.endswith("2"))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=ALL_SHAPES)
    ap.add_argument("--other-lib", default=None, help="another build's libmodgpu.so (the parent commit's) for rekey4g")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_move.json"))
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
            O = ctypes.CDLL(a.other_lib)
            O.modgpu_rekey_device_to.restype = ctypes.c_int
            O.modgpu_rekey_device_to.argtypes = L.modgpu_rekey_device_to.argtypes
            n = 4 << 30
            src, dst = M.DeviceBuffer(n), M.DeviceBuffer(n)
            fill(src, n)
            k3 = M.as_int32(M.KEY_PS3)

            def one_pass(v):
                lib = O if v.startswith("other") else L
                if lib.modgpu_rekey_device_to(_vp(dst.ptr), _vp(src.ptr), n, k3, 0, kk, 0, -1, stv):
                    raise RuntimeError("rekey failed")
                return None if lib is O else M.last_launch()

            row = measure(["this", "other", "this2", "other2"], one_pass, st, a.warmup, a.steps, n)
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
            fill(part, n + d)

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
            row = measure(variants, one_pass, st, a.warmup, a.steps, n)
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
    out = {"tool": "tools/bench_rekey_move.py", "unit": "TB/s of n payload bytes per pass", "when": time.strftime("%Y-%m-%dT%H:%M:%S"),
           "warmup": a.warmup, "steps": a.steps, "key": KEY, "off_from": OFF, "rekey_kernel_source_hash": M.rekey_kernel_source_hash(),
           "kernel_source_hash": M.kernel_source_hash(), "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
