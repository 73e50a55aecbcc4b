#!/usr/bin/env python3
"""The rekey table call (modgpu_rekey_table_device: a device-resident table of rekey entries in three launches) at both stream grids
against what a caller had before: modgpu_rekey_device_to for one buffer, modgpu_rekey_batch_device_to (16 entries per launch) for many.
One process, one stream, HIP events recorded on that stream around every single pass; the variants alternate step by step so drift hits
all of them alike.  Rate unit: 2n algorithmic bytes per pass (n read + n written), as in DESIGN.md 5.  Every entry goes PS3 -> PS4.

    shapes     4g         1 x 4 GiB, source and destination co-aligned (phase 0), both offsets 0   against modgpu_rekey_device_to
               16x256m    16 x 256 MiB, co-aligned                                             against modgpu_rekey_batch_device_to
               16kx64k    16 384 x 64 KiB, random source and destination phases, offsets = their places in a part  against the batch
                          call (1 024 launches)
               config4    100 000 entries of [0, 64 KiB] (seeded), packed as in a part, relocated into a second part in which every
                          entry moved by a random amount (a file inserted, files resized): off_from = the old offset, off_to = the new
                          one -- against the batch call (6 250 launches)
    variants   grid256    the call with one stream workgroup per CU on all 256 CUs (testing flavour: modgpu_debug_set_rekey_table_grid)
               grid200    the same with the table call's 25 per 32 CUs (200)
               base       the existing call named above (its argument arrays built once, outside the timed region); the batch call is
                          made per 16 entries -- what a launch takes anyway -- since its overlap check is quadratic in its entry count

    python tools/bench_rekey_table.py [--shapes 4g,16x256m,16kx64k,config4] [--warmup 3] [--steps 20] [--out profiles/r10_rekey_table.json]
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

KEY_FROM, KEY_TO = M.KEY_PS3, M.KEY_PS4
VARIANTS = ("grid256", "grid200", "base")
GRIDS = {"grid256": 256, "grid200": 200}
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
    """(sizes, src offsets, dst offsets, offsets under key_from, offsets under key_to, src bytes, dst bytes)"""
    rng = np.random.default_rng(0x4D6F6475)
    if shape == "4g":
        sz = np.array([4 << 30], np.int64)
        z = np.zeros(1, np.int64)
        return sz, z, z, z, z, int(sz[0]) + 64, int(sz[0]) + 64
    if shape == "16x256m":
        sz = np.full(16, 256 << 20, np.int64)
        o = np.arange(16, dtype=np.int64) * (256 << 20)
        return sz, o, o, o, o, int(sz.sum()) + 64, int(sz.sum()) + 64
    if shape == "16kx64k":
        sz = np.full(16384, 65536, np.int64)
        so = np.arange(16384, dtype=np.int64) * (65536 + 16) + rng.integers(0, 16, size=16384)
        do = np.arange(16384, dtype=np.int64) * (65536 + 16) + rng.integers(0, 16, size=16384)
        return sz, so, do, so, do, int(so[-1]) + 65536 + 64, int(do[-1]) + 65536 + 64
    if shape == "config4":
        sz = rng.integers(0, 65537, size=100000).astype(np.int64)
        o = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)
        moved = o + np.cumsum(rng.integers(0, 2, size=sz.size) * rng.integers(1, 4096, size=sz.size))  # every entry after a change moves
        return sz, o, moved, o, moved, int(sz.sum()) + 64, int(moved[-1] + sz[-1]) + 64
    raise ValueError(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4g,16x256m,16kx64k,config4")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_rekey_table.json"))
    a = ap.parse_args()
    variants = a.variants.split(",")
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    M.debug_set_rekey_table_grid(0)
    shipped = None
    L = M.lib()
    st = Stream()
    e0, e1 = Event(), Event()
    rows = {}
    tile = np.random.default_rng(1).integers(0, 256, size=1 << 24, dtype=np.uint8)
    for shape in a.shapes.split(","):
        sz, so, do, ofr, oto, sn, dn = layout(shape)
        n_bytes = int(sz.sum())
        sbuf, dbuf = M.DeviceBuffer(sn), M.DeviceBuffer(dn)
        for off in range(0, sn, tile.size):
            sbuf.upload(tile[:min(tile.size, sn - off)], offset=off)
        t = M.rekey_table(sz.size)
        t["dst"] = dbuf.ptr + do
        t["src"] = sbuf.ptr + so
        t["n"] = sz
        t["off_from"] = ofr
        t["off_to"] = oto
        t["key_from"] = M.as_int32(KEY_FROM)
        t["key_to"] = M.as_int32(KEY_TO)
        M.rekey_table_validate(t)
        tb = M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        ws = M.DeviceBuffer(M.rekey_table_workspace_bytes(sz.size))
        if shipped is None:
            M.rekey_table_device(tb, ws, n=sz.size, stream=st.handle)
            shipped = M.last_launch()["grid"]
        k = sz.size
        cd = (_vp * k)(*[int(x) for x in t["dst"]])
        cs = (_vp * k)(*[int(x) for x in t["src"]])
        cz = (_u64 * k)(*[int(x) for x in sz])
        cf = (_u64 * k)(*[int(x) for x in ofr])
        ct = (_u64 * k)(*[int(x) for x in oto])
        P = ctypes.POINTER
        groups = [(ctypes.cast(ctypes.addressof(cd) + 8 * i, P(_vp)), ctypes.cast(ctypes.addressof(cs) + 8 * i, P(_vp)),
                   ctypes.cast(ctypes.addressof(cz) + 8 * i, P(_u64)), ctypes.cast(ctypes.addressof(cf) + 8 * i, P(_u64)),
                   ctypes.cast(ctypes.addressof(ct) + 8 * i, P(_u64)), min(16, k - i))
                  for i in range(0, k, 16)]
        kf32, kt32, stv = M.as_int32(KEY_FROM), M.as_int32(KEY_TO), _vp(st.handle)
        batch = L.modgpu_rekey_batch_device_to

        def one_pass(v):
            if v in GRIDS:
                M.debug_set_rekey_table_grid(GRIDS[v])
                M.rekey_table_device(tb, ws, n=k, stream=st.handle)
            elif shape == "4g":
                M.rekey_device_to(int(t["dst"][0]), int(t["src"][0]), KEY_FROM, KEY_TO, 0, 0, stream=st.handle, n=n_bytes)
            else:
                for gd, gs, gz, gf, gt, gn in groups:
                    if batch(gd, gs, gz, gf, gt, gn, kf32, kt32, -1, stv):
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
        M.debug_set_rekey_table_grid(0)
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
    out = {"tool": "tools/bench_rekey_table.py", "unit": "TB/s of 2n algorithmic bytes per pass (n read + n written)",
           "when": time.strftime("%Y-%m-%dT%H:%M:%S"), "warmup": a.warmup, "steps": a.steps, "key_from": KEY_FROM, "key_to": KEY_TO,
           "shipped_grid": shipped, "rekey_table_kernel_source_hash": M.rekey_table_kernel_source_hash(),
           "rekey_kernel_source_hash": M.rekey_kernel_source_hash(), "kernel_source_hash": M.kernel_source_hash(), "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
