#!/usr/bin/env python3
"""The table call (modgpu_cycle_table_device: a device-resident table of out-of-place entries in three launches) against what a caller
had before: modgpu_cycle_device_to for one buffer, modgpu_cycle_batch_device_to (16 entries per launch) for many.  One process, one
stream, HIP events recorded on that stream around every single pass; the variants alternate step by step so drift hits all of them
alike.  Rate unit: 2n algorithmic bytes per pass (n read + n written), as in DESIGN.md 5.

    shapes     4g         1 x 4 GiB, source and destination co-aligned (phase 0)           against modgpu_cycle_device_to
               16x256m    16 x 256 MiB, co-aligned                                          against modgpu_cycle_batch_device_to
               16kx64k    16 384 x 64 KiB, random source and destination phases            against the batch call (1 024 launches)
               config4    100 000 entries of [0, 64 KiB] (seeded), packed as in a part,    against the batch call (6 250 launches)
                          extracted to a second buffer of the same layout, stream_off = the entry's offset in the part
    variants   table      the shipped call (table and workspace resident)
               table_all  the same with one stream workgroup per CU (testing flavour: modgpu_debug_set_table_grid)
               base       the existing call named above (its argument arrays built once, outside the timed region); the batch call is
                          made per 16 entries -- what a launch takes anyway -- since its overlap check is quadratic in its entry count

    python tools/bench_table.py [--shapes 4g,16x256m,16kx64k,config4] [--warmup 3] [--steps 20] [--out profiles/r09_table.json]
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
VARIANTS = ("table", "table_all", "base")
_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


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


def layout(shape):
    """(sizes, src offsets, dst offsets, stream offsets, src bytes, dst bytes)"""
    rng = np.random.default_rng(0x4D6F6475)
    if shape == "4g":
        sz = np.array([4 << 30], np.int64)
        return sz, np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64), int(sz[0]) + 64, int(sz[0]) + 64
    if shape == "16x256m":
        sz = np.full(16, 256 << 20, np.int64)
        o = np.arange(16, dtype=np.int64) * (256 << 20)
        return sz, o, o, np.zeros(16, np.int64), int(sz.sum()) + 64, int(sz.sum()) + 64
    if shape == "16kx64k":
        sz = np.full(16384, 65536, np.int64)
        so = np.arange(16384, dtype=np.int64) * (65536 + 16) + rng.integers(0, 16, size=16384)
        do = np.arange(16384, dtype=np.int64) * (65536 + 16) + rng.integers(0, 16, size=16384)
        return sz, so, do, np.zeros(16384, np.int64), int(so[-1]) + 65536 + 64, int(do[-1]) + 65536 + 64
    if shape == "config4":
        sz = rng.integers(0, 65537, size=100000).astype(np.int64)
        o = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)
        return sz, o, o, o, int(sz.sum()) + 64, int(sz.sum()) + 64
    raise ValueError(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4g,16x256m,16kx64k,config4")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_table.json"))
    a = ap.parse_args()
    variants = a.variants.split(",")
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    L = M.lib()
    st = Stream()
    e0, e1 = Event(), Event()
    rows = {}
    tile = np.random.default_rng(1).integers(0, 256, size=1 << 24, dtype=np.uint8)
    for shape in a.shapes.split(","):
        sz, so, do, offs, sn, dn = layout(shape)
        n_bytes = int(sz.sum())
        sbuf, dbuf = M.DeviceBuffer(sn), M.DeviceBuffer(dn)
        for off in range(0, sn, tile.size):
            sbuf.upload(tile[:min(tile.size, sn - off)], offset=off)
        t = M.table(sz.size)
        t["dst"] = dbuf.ptr + do
        t["src"] = sbuf.ptr + so
        t["n"] = sz
        t["stream_off"] = offs
        t["key"] = M.as_int32(KEY)
        M.table_validate(t)
        tb = M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        ws = M.DeviceBuffer(M.table_workspace_bytes(sz.size))
        k = sz.size
        cd = (_vp * k)(*[int(x) for x in t["dst"]])
        cs = (_vp * k)(*[int(x) for x in t["src"]])
        cz = (_u64 * k)(*[int(x) for x in sz])
        co = (_u64 * k)(*[int(x) for x in offs])
        P = ctypes.POINTER
        groups = [(ctypes.cast(ctypes.addressof(cd) + 8 * i, P(_vp)), ctypes.cast(ctypes.addressof(cs) + 8 * i, P(_vp)),
                   ctypes.cast(ctypes.addressof(cz) + 8 * i, P(_u64)), ctypes.cast(ctypes.addressof(co) + 8 * i, P(_u64)), min(16, k - i))
                  for i in range(0, k, 16)]
        key32, stv = M.as_int32(KEY), _vp(st.handle)
        batch = L.modgpu_cycle_batch_device_to

        def one_pass(v):
            if v in ("table", "table_all"):
                M.debug_set_table_grid(256 if v == "table_all" else 0)
                M.cycle_table_device(tb, ws, n=k, stream=st.handle)
            elif shape == "4g":
                M.cycle_device_to(int(t["dst"][0]), int(t["src"][0]), n_bytes, KEY, 0, stream=st.handle)
            else:
                for gd, gs, gz, go, gn in groups:
                    if batch(gd, gs, gz, go, gn, key32, -1, stv):
                        raise RuntimeError(M.lib().modgpu_last_error().decode())
            return M.last_launch()

        launch = {}
        for v in variants:
            before = M.path_stats()["gpu_launches"]
            for _ in range(a.warmup):
                info = one_pass(v)
            launch[v] = {"kernel": info["kernel"], "variant": info["variant"], "grid": info["grid"],
                         "launches_per_pass": (M.path_stats()["gpu_launches"] - before) // a.warmup}
        st.sync()
        assert M.table_status(ws) is None
        times = {v: [] for v in variants}
        for _ in range(a.steps):
            for v in variants:
                e0.record(st)
                one_pass(v)
                e1.record(st)
                times[v].append(elapsed_ms(e0, e1))
        M.debug_set_table_grid(0)
        row = {"entries": int(k), "bytes": n_bytes, "launch": launch}
        for v in variants:
            tt = sorted(times[v])
            med = tt[len(tt) // 2]
            row[v] = {"median_ms": round(med, 5), "min_ms": round(tt[0], 5), "max_ms": round(tt[-1], 5),
                      "TBps_2n": round(2 * n_bytes / (med * 1e-3) / 1e12, 4)}
        if "base" in variants:
            for v in variants:
                if v != "base":
                    row[v + "_speedup_over_base"] = round(row["base"]["median_ms"] / row[v]["median_ms"], 4)
        rows[shape] = row
        print("%-8s %6d entries  " % (shape, k) + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps_2n"]) for v in variants),
              flush=True)
        for b in (sbuf, dbuf, tb, ws):
            b.free()
    st.destroy()
    out = {"tool": "tools/bench_table.py", "unit": "TB/s of 2n algorithmic bytes per pass (n read + n written)",
           "when": time.strftime("%Y-%m-%dT%H:%M:%S"), "warmup": a.warmup, "steps": a.steps, "key": KEY,
           "table_kernel_source_hash": M.table_kernel_source_hash(), "to_kernel_source_hash": M.to_kernel_source_hash(),
           "kernel_source_hash": M.kernel_source_hash(), "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
