#!/usr/bin/env python3
"""The rekey pass (modgpu_rekey_device_to: ciphertext under one keystream to ciphertext under another) in its two launch shapes,
against the two-pass way a caller had to do it before (modgpu_cycle_device_to under the old key, then modgpu_cycle_device under the
new one) and against the single-key out-of-place pass as the ceiling.  One process, one stream, HIP events recorded on that stream
around every single pass; the variants alternate step by step so drift hits all of them alike.  Rate unit: 2n algorithmic bytes per
pass (n read + n written), as in DESIGN.md 5 -- the two-pass route counts 2n too, although it moves 4n.

    variants   fused_a      rekey, shape (a): the out-of-place kernel's grid (25 workgroups per 32 CUs), src and dst at phase 0
               fused_b      rekey, shape (b): one workgroup per CU on every CU, src and dst at phase 0
               fused_mis    rekey, shipped shape, src at phase 5 and dst at phase 0 (the v_alignbyte_b32 funnel)
               two_pass     modgpu_cycle_device_to under PS3, then modgpu_cycle_device under PS4
               to_ceiling   modgpu_cycle_device_to under PS4 alone (one keystream: the HBM-bound pass)

    python tools/bench_rekey.py [--sizes-mib 64,256,1024,4096] [--warmup 3] [--steps 20] [--out profiles/r08_rekey.json]
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

VARIANTS = ("fused_a", "fused_b", "fused_mis", "two_pass", "to_ceiling")
KF, KT = M.KEY_PS3, M.KEY_PS4


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
    if v in ("fused_a", "fused_b"):
        M.debug_set_rekey_form("queue" if v == "fused_a" else "all")
        M.rekey_device_to(dst, src, KF, KT, n=n, stream=st.handle)
    elif v == "fused_mis":
        M.debug_set_rekey_form(None)
        M.rekey_device_to(dst, src + 5, KF, KT, n=n, stream=st.handle)
    elif v == "two_pass":
        M.cycle_device_to(dst, src, n, KF, 0, stream=st.handle)
        M.cycle_device(dst, n, KT, 0, stream=st.handle)
    else:
        M.cycle_device_to(dst, src, n, KT, 0, stream=st.handle)
    return M.last_launch()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", default="64,256,1024,4096")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_rekey.json"))
    a = ap.parse_args()
    assert a.warmup >= 3 and a.steps >= 20, "at least 3 warm-ups and 20 timed steps"
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch between the two launch shapes
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
        launch = {}
        for v in VARIANTS:
            for _ in range(a.warmup):
                info = one_pass(v, src, dst, n, st)
            launch[v] = {"kernel": info["kernel"], "variant": info["variant"], "grid": info["grid"]}
        st.sync()
        times = {v: [] for v in VARIANTS}
        for _ in range(a.steps):
            for v in VARIANTS:
                e0.record(st)
                one_pass(v, src, dst, n, st)
                e1.record(st)
                times[v].append(elapsed_ms(e0, e1))
        M.debug_set_rekey_form(None)
        row = {"bytes": n, "launch": launch}
        for v in VARIANTS:
            t = sorted(times[v])
            med = t[len(t) // 2]
            row[v] = {"median_ms": round(med, 5), "min_ms": round(t[0], 5), "max_ms": round(t[-1], 5),
                      "TBps_2n": round(2 * n / (med * 1e-3) / 1e12, 4)}
        for v in ("fused_a", "fused_b", "fused_mis"):
            row[v + "_over_two_pass"] = round(row["two_pass"]["median_ms"] / row[v]["median_ms"], 4)
            row[v + "_of_ceiling"] = round(row["to_ceiling"]["median_ms"] / row[v]["median_ms"], 4)
        rows[str(n)] = row
        print("%5d MiB  " % mib + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps_2n"]) for v in VARIANTS), flush=True)
        sbuf.free()
        dbuf.free()
    st.destroy()
    out = {"tool": "tools/bench_rekey.py", "unit": "TB/s of 2n algorithmic bytes per pass (n read + n written)",
           "when": time.strftime("%Y-%m-%dT%H:%M:%S"), "warmup": a.warmup, "steps": a.steps, "key_from": KF, "key_to": KT,
           "rekey_kernel_source_hash": M.rekey_kernel_source_hash(), "to_kernel_source_hash": M.to_kernel_source_hash(),
           "kernel_source_hash": M.kernel_source_hash(), "misaligned": "src phase 5, dst phase 0", "sizes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
