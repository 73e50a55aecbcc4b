#!/usr/bin/env python3
"""The out-of-place pass (modgpu_cycle_device_to) against the in-place one and against the two-pass way a caller had to do it
before (hipMemcpyAsync D2D, then modgpu_cycle_device).  One process, one stream, HIP events recorded on that stream around every
single pass; the variants alternate step by step so drift hits all of them alike.  Rate unit: 2n algorithmic bytes per pass
(n read + n written), as in DESIGN.md 5.

    variants   inplace      modgpu_cycle_device on dst (phase 0)
               to_aligned   modgpu_cycle_device_to, src and dst both at phase 0
               to_mis_a     src at phase 5, dst at phase 0, unaligned source loads       (form a)
               to_mis_b     the same, aligned loads + v_alignbyte_b32 funnel           (form b)
               copy_inplace hipMemcpyAsync D2D src -> dst, then modgpu_cycle_device on dst

    python tools/bench_cycle_to.py [--sizes-mib 64,256,1024,4096] [--warmup 3] [--steps 20] [--out profiles/r07_cycle_to.json]
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

VARIANTS = ("inplace", "to_aligned", "to_mis_a", "to_mis_b", "copy_inplace")
KEY = M.KEY_PS4
D2D = 3  # hipMemcpyDeviceToDevice


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


def one_pass(v, src, dst, n, st):
    if v == "inplace":
        M.cycle_device(dst, n, KEY, 0, stream=st.handle)
    elif v == "to_aligned":
        M.cycle_device_to(dst, src, n, KEY, 0, stream=st.handle)
    elif v in ("to_mis_a", "to_mis_b"):
        M.debug_set_to_form("unaligned" if v == "to_mis_a" else "funnel")
        M.cycle_device_to(dst, src + 5, n, KEY, 0, stream=st.handle)
    else:
        _ok(hip().hipMemcpyAsync(ctypes.c_void_p(dst), ctypes.c_void_p(src), ctypes.c_size_t(n), ctypes.c_int(D2D), ctypes.c_void_p(st.handle)),
            "hipMemcpyAsync")
        M.cycle_device(dst, n, KEY, 0, stream=st.handle)
    return M.last_launch()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", default="64,256,1024,4096")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_cycle_to.json"))
    a = ap.parse_args()
    assert a.warmup >= 3 and a.steps >= 20, "at least 3 warm-ups and 20 timed steps"
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch between the two source forms
    st = Stream()
    e0, e1 = Event(), Event()
    rows = {}
    tile = np.random.default_rng(1).integers(0, 256, size=1 << 24, dtype=np.uint8)
    for mib in [int(x) for x in a.sizes_mib.split(",")]:
        n = mib << 20
        sbuf, dbuf = M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64)
        for off in range(0, n + 64, tile.size):
            sbuf.upload(tile[:min(tile.size, n + 64 - off)], offset=off)
        src, dst = sbuf.ptr, dbuf.ptr  # hipMalloc: 256-byte aligned, phase 0
        kernels = {}
        for v in VARIANTS:
            for _ in range(a.warmup):
                kernels[v] = one_pass(v, src, dst, n, st)["kernel"]
        st.sync()
        times = {v: [] for v in VARIANTS}
        for _ in range(a.steps):
            for v in VARIANTS:
                e0.record(st)
                one_pass(v, src, dst, n, st)
                e1.record(st)
                times[v].append(elapsed_ms(e0, e1))
        M.debug_set_to_form(None)
        row = {"bytes": n, "kernel": kernels}
        for v in VARIANTS:
            t = sorted(times[v])
            med = t[len(t) // 2]
            row[v] = {"median_ms": round(med, 5), "min_ms": round(t[0], 5), "max_ms": round(t[-1], 5),
                      "TBps_2n": round(2 * n / (med * 1e-3) / 1e12, 4)}
        row["to_aligned_over_inplace"] = round(row["inplace"]["median_ms"] / row["to_aligned"]["median_ms"], 4)
        row["to_aligned_over_copy_inplace"] = round(row["copy_inplace"]["median_ms"] / row["to_aligned"]["median_ms"], 4)
        row["mis_a_over_mis_b"] = round(row["to_mis_b"]["median_ms"] / row["to_mis_a"]["median_ms"], 4)
        rows[str(n)] = row
        print("%5d MiB  " % mib + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps_2n"]) for v in VARIANTS), flush=True)
        sbuf.free()
        dbuf.free()
    st.destroy()
    out = {"tool": "tools/bench_cycle_to.py", "unit": "TB/s of 2n algorithmic bytes per pass (n read + n written)",
           "when": time.strftime("%Y-%m-%dT%H:%M:%S"), "warmup": a.warmup, "steps": a.steps, "key": KEY,
           "to_kernel_source_hash": M.to_kernel_source_hash(), "kernel_source_hash": M.kernel_source_hash(),
           "misaligned": "src phase 5, dst phase 0", "sizes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
