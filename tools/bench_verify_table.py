#!/usr/bin/env python3
"""The verify table call (modgpu_verify_table_device: a device-resident table of verify entries in three launches) at two stream grids
against what a caller had before: modgpu_verify_device for one buffer, modgpu_verify_batch_device (16 entries per compare launch) for
many.  One process, one stream, HIP events recorded on that stream around every single pass; the variants alternate step by step so
drift hits all of them alike.  Rate unit: 2n algorithmic bytes per pass (n of the comparand read + n of the source read), as in
DESIGN.md 4.10.  The comparand is made on the device by modgpu_cycle_table_device over the same table, so a pass under the same key
is clean.

    shapes     4g           1 x 4 GiB clean, source and comparand co-aligned                      against modgpu_verify_device
               4g_p5        the same with the source at phase 5 (the funnel read)                  against modgpu_verify_device
               16x256m      16 x 256 MiB, co-aligned                                               against modgpu_verify_batch_device
               16kx64k      16 384 x 64 KiB, random source and comparand phases                    against the batch call (1 + 1 024 launches)
               config4      100 000 entries of [0, 64 KiB] (seeded), packed as in a part            against the batch call (1 + 6 250 launches)
               config4dirty config4 compared under the WRONG key: every byte a mismatch, every wave of every chunk in the slow
                            path and every chunk a flush -- against the call's own clean run (`base` = the shipped grid, right key)
    variants   grid256      the call with one stream workgroup per CU on all 256 CUs (testing flavour: modgpu_debug_set_verify_table_grid)
               grid200      the same with the table call's 25 per 32 CUs (200)
               base         the existing call named above (its argument arrays built once, outside the timed region)

    python tools/bench_verify_table.py [--shapes 4g,4g_p5,16x256m,16kx64k,config4,config4dirty] [--warmup 3] [--steps 20] [--out profiles/r12_verify_table.json]
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

KEY, WRONG_KEY = M.KEY_PS3, M.KEY_PS4
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
    """(sizes, src offsets, comparand offsets, stream offsets, src bytes, comparand bytes)"""
    rng = np.random.default_rng(0x4D6F6475)
    if shape in ("4g", "4g_p5"):
        sz = np.array([4 << 30], np.int64)
        z = np.zeros(1, np.int64)
        return sz, z + (5 if shape == "4g_p5" else 0), z, z, int(sz[0]) + 64, int(sz[0]) + 64
    if shape == "16x256m":
        sz = np.full(16, 256 << 20, np.int64)
        o = np.arange(16, dtype=np.int64) * (256 << 20)
        return sz, o, o, o, int(sz.sum()) + 64, int(sz.sum()) + 64
    if shape == "16kx64k":
        sz = np.full(16384, 65536, np.int64)
        so = np.arange(16384, dtype=np.int64) * (65536 + 16) + rng.integers(0, 16, size=16384)
        eo = np.arange(16384, dtype=np.int64) * (65536 + 16) + rng.integers(0, 16, size=16384)
        return sz, so, eo, eo, int(so[-1]) + 65536 + 64, int(eo[-1]) + 65536 + 64
    if shape in ("config4", "config4dirty"):
        sz = rng.integers(0, 65537, size=100000).astype(np.int64)
        o = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)
        return sz, o, o, o, int(sz.sum()) + 64, int(sz.sum()) + 64
    raise ValueError(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4g,4g_p5,16x256m,16kx64k,config4,config4dirty")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_verify_table.json"))
    a = ap.parse_args()
    variants = a.variants.split(",")
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    M.debug_set_verify_table_grid(0)
    shipped = None
    L = M.lib()
    st = Stream()
    e0, e1 = Event(), Event()
    rows = {}
    tile = np.random.default_rng(1).integers(0, 256, size=1 << 24, dtype=np.uint8)
    for shape in a.shapes.split(","):
        sz, so, eo, offs, sn, en = layout(shape)
        dirty = shape == "config4dirty"
        n_bytes = int(sz.sum())
        k = sz.size
        sbuf, ebuf = M.DeviceBuffer(sn), M.DeviceBuffer(en)
        for off in range(0, sn, tile.size):
            sbuf.upload(tile[:min(tile.size, sn - off)], offset=off)
        t = M.table(k)
        t["dst"] = ebuf.ptr + eo
        t["src"] = sbuf.ptr + so
        t["n"] = sz
        t["stream_off"] = offs
        t["key"] = M.as_int32(KEY)
        M.cycle_table_device(t)  # the comparand: what the cipher writes
        tb = M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        tw = t.copy()
        tw["key"] = M.as_int32(WRONG_KEY)
        tbw = M.DeviceBuffer(tw.nbytes)
        tbw.upload(tw.view(np.uint8))
        ws = M.DeviceBuffer(M.verify_table_workspace_bytes(k))
        res = M.DeviceBuffer(32 * k)
        if shipped is None:
            M.verify_table_device(tb, res, ws, n=k, stream=st.handle)
            shipped = M.last_launch()["grid"]
        ce = (_vp * k)(*[int(x) for x in t["dst"]])
        cs = (_vp * k)(*[int(x) for x in t["src"]])
        cz = (_u64 * k)(*[int(x) for x in sz])
        co = (_u64 * k)(*[int(x) for x in offs])
        key32, stv = M.as_int32(KEY), _vp(st.handle)
        batch = L.modgpu_verify_batch_device

        def one_pass(v):
            if v in GRIDS:
                M.debug_set_verify_table_grid(GRIDS[v])
                M.verify_table_device(tbw if dirty else tb, res, ws, n=k, stream=st.handle)
            elif dirty:
                M.debug_set_verify_table_grid(0)
                M.verify_table_device(tb, res, ws, n=k, stream=st.handle)
            elif k == 1:
                M.verify_device(int(t["dst"][0]), int(t["src"][0]), KEY, 0, result=res, stream=st.handle, n=n_bytes)
            else:
                if batch(ce, cs, cz, co, k, key32, _vp(res.ptr), -1, stv):
                    raise RuntimeError(M.lib().modgpu_last_error().decode())
            return M.last_launch()

        launch, summaries = {}, {}
        for v in variants:
            before = M.path_stats()["gpu_launches"]
            for _ in range(a.warmup):
                info = one_pass(v)
            launch[v] = {"kernel": info["kernel"], "variant": info["variant"], "grid": info["grid"],
                         "launches_per_pass": (M.path_stats()["gpu_launches"] - before) // a.warmup}
            st.sync()
            if info["variant"] == 11:
                assert M.table_status(ws) is None
                summaries[v] = M.verify_table_summary(ws)
                assert (summaries[v]["mismatches"] == 0) == (not (dirty and v in GRIDS)), (shape, v, summaries[v])
            else:
                assert int(M.verify_results(res, k)["mismatches"].sum()) == 0, (shape, v)
        times = {v: [] for v in variants}
        for _ in range(a.steps):
            for v in variants:
                e0.record(st)
                one_pass(v)
                e1.record(st)
                times[v].append(elapsed_ms(e0, e1))
        M.debug_set_verify_table_grid(0)
        row = {"entries": int(k), "bytes": n_bytes, "launch": launch, "summary": summaries}
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
        print("%-12s %6d entries  " % (shape, k) + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps_2n"]) for v in variants),
              flush=True)
        for b in (sbuf, ebuf, tb, tbw, ws, res):
            b.free()
    st.destroy()
    out = {"tool": "tools/bench_verify_table.py", "unit": "TB/s of 2n algorithmic bytes per pass (n of the comparand + n of the source, both read)",
           "when": time.strftime("%Y-%m-%dT%H:%M:%S"), "warmup": a.warmup, "steps": a.steps, "key": KEY, "wrong_key": WRONG_KEY,
           "shipped_grid": shipped, "verify_table_kernel_source_hash": M.verify_table_kernel_source_hash(),
           "verify_kernel_source_hash": M.verify_kernel_source_hash(), "kernel_source_hash": M.kernel_source_hash(), "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
