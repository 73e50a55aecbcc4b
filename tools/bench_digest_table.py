#!/usr/bin/env python3
"""The digest table call (modgpu_digest_table_device: a device-resident table of entries in three launches, one 32-byte record each)
against what a caller had before: modgpu_digest_device (digest only) for one buffer, modgpu_digest_batch_device (16 entries per launch,
one key per call, a memset node in front) for many.  One process, one stream, HIP events recorded on that stream around every single
pass; the variants alternate step by step so drift hits all of them alike.  Rate unit: n bytes read per pass.  Before anything is
timed every value of the table call is compared -- with zlib.adler32 of the host's own cycle of the source where the shape is small
(up to 16 MiB), with the existing call's values otherwise.

    shapes     64k, 1m, 16m 1 entry, launch-bound sizes                                            against modgpu_digest_device
               4g           1 x 4 GiB, the source chunk-aligned                                    against modgpu_digest_device
               4g_p5        the same with the source at phase 5                                    against modgpu_digest_device
               16kx64k      16 384 x 64 KiB at random source phases                                against the batch call (1 024 launches)
               config4      100 000 entries of [0, 64 KiB] (seeded), packed as in a part            against the batch call (6 250 launches)
    variants   table        the call at its shipped grid (one workgroup per CU)
               grid200      the same on 200 workgroups (testing flavour: modgpu_debug_set_digest_table_grid)
               base         the existing call named above (its argument arrays built once, outside the timed region)

    python tools/bench_digest_table.py [--shapes 64k,1m,16m,4g,4g_p5,16kx64k,config4] [--warmup 3] [--steps 20] [--out profiles/r17_digest_table.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MODGPU_REQUIRE_GPU"] = "1"
import numpy as np  # noqa: E402
import modulate_amd as M  # noqa: E402
from hip_rt import Stream, hip, _ok  # noqa: E402  (tests/hip_rt.py: streams over the HIP runtime libmodgpu.so brought in)

KEY = M.KEY_PS3
VARIANTS = ("table", "grid200", "base")
GRIDS = {"table": 0, "grid200": 200}
SINGLE = {"64k": 64 << 10, "1m": 1 << 20, "16m": 16 << 20, "4g": 4 << 30, "4g_p5": 4 << 30}
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
    """(sizes, source offsets from a chunk-aligned base, stream offsets, source bytes)"""
    rng = np.random.default_rng(0x4D6F6475)
    if shape in SINGLE:
        sz = np.array([SINGLE[shape]], np.int64)
        z = np.zeros(1, np.int64)
        return sz, z + (5 if shape == "4g_p5" else 0), z + 12345, int(sz[0]) + 64
    if shape == "16kx64k":
        sz = np.full(16384, 65536, np.int64)
        so = np.arange(16384, dtype=np.int64) * (65536 + 16) + rng.integers(0, 16, size=16384)
        return sz, so, so, int(so[-1]) + 65536 + 64
    if shape == "config4":
        sz = rng.integers(0, 65537, size=100000).astype(np.int64)
        o = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)
        return sz, o, o, int(sz.sum()) + 64
    raise ValueError(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64k,1m,16m,4g,4g_p5,16kx64k,config4")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_digest_table.json"))
    a = ap.parse_args()
    variants = a.variants.split(",")
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    M.debug_set_digest_table_grid(0)
    L = M.lib()
    st = Stream()
    e0, e1 = Event(), Event()
    rows = {}
    shipped = None
    tile = np.random.default_rng(1).integers(0, 256, size=1 << 24, dtype=np.uint8)
    for shape in a.shapes.split(","):
        sz, so, offs, sn = layout(shape)
        n_bytes, k = int(sz.sum()), sz.size
        sbuf = M.DeviceBuffer(sn + 65536)
        base = -sbuf.ptr % 65536  # the layout's offsets count from a chunk edge
        for off in range(0, sn, tile.size):
            sbuf.upload(tile[:min(tile.size, sn - off)], offset=base + off)
        t = M.table(k)
        t["src"] = sbuf.ptr + base + so
        t["n"], t["stream_off"], t["key"] = sz, offs, M.as_int32(KEY)
        tb = M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        ws = M.DeviceBuffer(M.digest_table_workspace_bytes(k))
        res, res_base = M.DeviceBuffer(32 * k), M.DeviceBuffer(32 * k)
        cs = (_vp * k)(*[int(x) for x in t["src"]])
        cz = (_u64 * k)(*[int(x) for x in sz])
        co = (_u64 * k)(*[int(x) for x in offs])
        key32, stv = M.as_int32(KEY), _vp(st.handle)
        batch = L.modgpu_digest_batch_device

        def one_pass(v):
            if v in GRIDS:
                M.debug_set_digest_table_grid(GRIDS[v])
                M.digest_table_device(tb, res, ws, n=k, stream=st.handle)
            elif k == 1:
                M.digest_device(int(t["src"][0]), KEY, int(offs[0]), None, res_base, -1, st.handle, n=n_bytes)
            elif batch(None, cs, cz, co, k, key32, _vp(res_base.ptr), -1, stv):
                raise RuntimeError(L.modgpu_last_error().decode())
            return M.last_launch()

        # every value, before anything is timed
        launch = {}
        for v in variants:
            before = M.path_stats()["gpu_launches"]
            for _ in range(a.warmup):
                info = one_pass(v)
            launch[v] = {"kernel": info["kernel"], "variant": info["variant"], "grid": info["grid"],
                         "launches_per_pass": (M.path_stats()["gpu_launches"] - before) // a.warmup}
            st.sync()
            if v in GRIDS:
                assert M.table_status(ws) is None and info["variant"] == 17, (shape, v, info)
                if v == "table" and shipped is None:
                    shipped = info["grid"]
                got = M.digest_results(res, k)[1]
                if n_bytes <= 16 << 20:
                    for i in range(k):  # the route a caller had: the out-of-place call into scratch, a download, zlib
                        scratch = M.DeviceBuffer(int(sz[i]) + 64)
                        M.cycle_device_to(scratch.ptr, int(t["src"][i]), int(sz[i]), KEY, int(offs[i]))
                        scratch.sync()
                        assert int(got[i]) == zlib.adler32(scratch.download(int(sz[i])).tobytes()) & 0xFFFFFFFF, (shape, v, i)
                        scratch.free()
                else:
                    one_pass("base")
                    st.sync()
                    assert np.array_equal(got, M.digest_results(res_base, k)[1]), (shape, v, "the table call and the existing call disagree")
        times = {v: [] for v in variants}
        for _ in range(a.steps):
            for v in variants:
                e0.record(st)
                one_pass(v)
                e1.record(st)
                times[v].append(elapsed_ms(e0, e1))
        M.debug_set_digest_table_grid(0)
        row = {"entries": int(k), "bytes": n_bytes, "launch": launch}
        for v in variants:
            tt = sorted(times[v])
            med = tt[len(tt) // 2]
            row[v] = {"median_ms": round(med, 5), "min_ms": round(tt[0], 5), "max_ms": round(tt[-1], 5), "TBps": round(n_bytes / (med * 1e-3) / 1e12, 4)}
        if "base" in variants:
            for v in variants:
                if v != "base":
                    row[v + "_speedup_over_base"] = round(row["base"]["median_ms"] / row[v]["median_ms"], 4)
        rows[shape] = row
        print("%-8s %6d entries  " % (shape, k) + "  ".join("%s %.4f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps"]) for v in variants), flush=True)
        for b in (sbuf, tb, ws, res, res_base):
            b.free()
    st.destroy()
    out = {"tool": "tools/bench_digest_table.py", "unit": "TB/s of n bytes read per pass", "when": time.strftime("%Y-%m-%dT%H:%M:%S"), "warmup": a.warmup,
           "steps": a.steps, "key": KEY, "shipped_grid": shipped, "verify_table_kernel_source_hash": M.verify_table_kernel_source_hash(),
           "to_kernel_source_hash": M.to_kernel_source_hash(), "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
