#!/usr/bin/env python3
"""The cycle digest table call (modgpu_cycle_digest_table_device: modgpu_cycle_table_device and one digest record per entry in one pass
and three launches) against what a caller had before: modgpu_cycle_table_device followed by modgpu_digest_table_device on the same table
and stream (3n bytes of traffic, six launches).  One process, one stream, HIP events recorded on that stream around every single pass;
the variants alternate step by step so drift hits all of them alike.  Rate unit: n bytes cycled per pass.  Before anything is timed the
fused call's records are compared with modgpu_digest_table_device's (of the same table for the output side, of the table under the
identity key for the input side) and its destination with modgpu_cycle_table_device's, byte for byte.

    shapes     64k, 1m, 16m 1 entry, launch-bound sizes
               4g           1 x 4 GiB, destination and source chunk-aligned
               4g_p5        the same with the source at phase 5
               16kx64k      16 384 x 64 KiB at random phases
               config4      100 000 entries of [0, 64 KiB] (seeded), packed as in a part
    variants   fused_out    the call at its shipped grid, MODGPU_DIGEST_OUTPUT
               fused_in     the same, MODGPU_DIGEST_INPUT
               g200, g256   fused_out on 200 and on 256 stream workgroups (testing flavour: modgpu_debug_set_cycle_digest_table_grid)
               two_a, two_b modgpu_cycle_table_device + modgpu_digest_table_device, twice per step: their difference is the A/A spread
               cycle_a, _b  modgpu_cycle_table_device alone, twice per step
               parent_a, _b modgpu_cycle_table_device of another build's library (--other-lib) loaded into this process, twice per step
               single, single_to   (one entry) modgpu_digest_device with a destination, and modgpu_cycle_device_to: the single call's own fused cost

    python tools/bench_cycle_digest_table.py [--shapes ...] [--warmup 3] [--steps 20] [--other-lib PATH] [--out profiles/r19_cycle_digest_table.json]
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

KEY = M.KEY_PS3
GRIDS = {"fused_out": 0, "fused_in": 0, "g200": 200, "g256": 256}
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
    """(sizes, destination offsets and source offsets from chunk-aligned bases, stream offsets, bytes of an arena)"""
    rng = np.random.default_rng(0x4D6F6475)
    if shape in SINGLE:
        sz = np.array([SINGLE[shape]], np.int64)
        z = np.zeros(1, np.int64)
        return sz, z, z + (5 if shape == "4g_p5" else 0), z + 12345, int(sz[0]) + 64
    if shape == "16kx64k":
        sz = np.full(16384, 65536, np.int64)
        do = np.arange(16384, dtype=np.int64) * (65536 + 32) + rng.integers(0, 16, size=16384)
        so = np.arange(16384, dtype=np.int64) * (65536 + 32) + rng.integers(0, 16, size=16384)
        return sz, do, so, so, int(do[-1]) + 65536 + 64
    if shape == "config4":
        sz = rng.integers(0, 65537, size=100000).astype(np.int64)
        o = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)
        return sz, o, o, o, int(sz.sum()) + 64
    raise ValueError(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64k,1m,16m,4g,4g_p5,16kx64k,config4")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--other-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_cycle_digest_table.json"))
    a = ap.parse_args()
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    M.debug_set_cycle_digest_table_grid(0)
    other = ctypes.CDLL(os.path.abspath(a.other_lib)) if a.other_lib else None
    if other is not None:
        other.modgpu_cycle_table_device.restype = ctypes.c_int
        other.modgpu_cycle_table_device.argtypes = [_vp, _u64, _vp, _u64, ctypes.c_int, _vp]
        other.modgpu_table_kernel_source_hash.restype = ctypes.c_char_p
    st = Stream()
    e0, e1 = Event(), Event()
    rows = {}
    shipped = None
    tile = np.random.default_rng(1).integers(0, 256, size=1 << 24, dtype=np.uint8)
    for shape in a.shapes.split(","):
        sz, do, so, offs, sn = layout(shape)
        n_bytes, k = int(sz.sum()), sz.size
        sbuf, dbuf = M.DeviceBuffer(sn + 65536 + 16), M.DeviceBuffer(sn + 65536)
        sbase, dbase = -sbuf.ptr % 65536, -dbuf.ptr % 65536  # the layout's offsets count from a chunk edge
        for off in range(0, sn, tile.size):
            sbuf.upload(tile[:min(tile.size, sn - off)], offset=sbase + off)
        t = M.table(k)
        t["dst"], t["src"] = dbuf.ptr + dbase + do, sbuf.ptr + sbase + so
        t["n"], t["stream_off"], t["key"] = sz, offs, M.as_int32(KEY)
        tb, tb_plain = M.DeviceBuffer(t.nbytes), M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        plain = t.copy()
        plain["key"] = 0
        tb_plain.upload(plain.view(np.uint8))
        ws = M.DeviceBuffer(M.cycle_digest_table_workspace_bytes(k))
        res, res_base = M.DeviceBuffer(32 * k), M.DeviceBuffer(32 * k)
        variants = ["fused_out", "fused_in", "two_a", "two_b", "cycle_a", "cycle_b"]
        if shape in ("4g", "4g_p5"):
            variants += ["g200", "g256", "single", "single_to"]
        if other is not None and shape in ("4g", "config4"):
            variants += ["parent_a", "parent_b"]

        def one_pass(v):
            if v in GRIDS:
                M.debug_set_cycle_digest_table_grid(GRIDS[v])
                M.cycle_digest_table_device(tb, res, M.DIGEST_INPUT if v == "fused_in" else M.DIGEST_OUTPUT, ws, n=k, stream=st.handle)
            elif v.startswith("two"):
                M.cycle_table_device(tb, ws, n=k, stream=st.handle)
                M.digest_table_device(tb, res_base, ws, n=k, stream=st.handle)
            elif v.startswith("cycle"):
                M.cycle_table_device(tb, ws, n=k, stream=st.handle)
            elif v.startswith("parent"):
                if other.modgpu_cycle_table_device(_vp(tb.ptr), k, _vp(ws.ptr), ws.nbytes, -1, _vp(st.handle)):
                    raise RuntimeError("the other library refused the table call")
                return {"kernel": "other library", "variant": 8, "grid": 0}
            elif v == "single":
                M.digest_device(int(t["src"][0]), KEY, int(offs[0]), int(t["dst"][0]), res_base, -1, st.handle, n=n_bytes)
            elif v == "single_to":
                M.cycle_device_to(int(t["dst"][0]), int(t["src"][0]), n_bytes, KEY, int(offs[0]), stream=st.handle)
            return M.last_launch()

        # every value, before anything is timed: the two-call route's destination and records are the reference
        one_pass("two_a")
        st.sync()
        want_out = M.digest_results(res_base, k)[1]
        probe = [(0, min(sn, 1 << 22)), (max(0, sn - (1 << 22)), min(sn, 1 << 22))]
        want_img = [dbuf.download(m, offset=dbase + o) for o, m in probe]
        M.digest_table_device(tb_plain, res_base, ws, n=k, stream=st.handle)
        st.sync()
        want_in = M.digest_results(res_base, k)[1]
        launch = {}
        for v in variants:
            if v in GRIDS:
                for o, m in probe:
                    dbuf.upload(np.zeros(m, np.uint8), offset=dbase + o)
            before = M.path_stats()["gpu_launches"]
            for _ in range(a.warmup):
                info = one_pass(v)
            launch[v] = {"kernel": info["kernel"], "variant": info["variant"], "grid": info["grid"],
                         "launches_per_pass": (M.path_stats()["gpu_launches"] - before) // a.warmup}
            st.sync()
            if v in GRIDS:
                assert M.table_status(ws) is None and info["variant"] == 18, (shape, v, info)
                if v == "fused_out" and shipped is None:
                    shipped = info["grid"]
                got = M.digest_results(res, k)[1]
                assert np.array_equal(got, want_in if v == "fused_in" else want_out), (shape, v, "the fused call and the digest table call disagree")
                for (o, m), w in zip(probe, want_img):
                    assert np.array_equal(dbuf.download(m, offset=dbase + o), w), (shape, v, "the fused call and the table call wrote different bytes")
        times = {v: [] for v in variants}
        for _ in range(a.steps):
            for v in variants:
                e0.record(st)
                one_pass(v)
                e1.record(st)
                times[v].append(elapsed_ms(e0, e1))
        M.debug_set_cycle_digest_table_grid(0)
        row = {"entries": int(k), "bytes": n_bytes, "launch": launch}
        for v in variants:
            tt = sorted(times[v])
            med = tt[len(tt) // 2]
            row[v] = {"median_ms": round(med, 5), "min_ms": round(tt[0], 5), "max_ms": round(tt[-1], 5), "TBps": round(n_bytes / (med * 1e-3) / 1e12, 4)}
        med = {v: row[v]["median_ms"] for v in variants}
        two = min(med["two_a"], med["two_b"])
        row["two_call_aa_spread"] = round(abs(med["two_a"] - med["two_b"]) / two, 5)
        row["cycle_aa_spread"] = round(abs(med["cycle_a"] - med["cycle_b"]) / min(med["cycle_a"], med["cycle_b"]), 5)
        for v in ("fused_out", "fused_in"):
            row["two_call_over_" + v] = round(two / med[v], 4)
            row[v + "_over_cycle"] = round(med[v] / min(med["cycle_a"], med["cycle_b"]), 4)
        if "single" in variants:
            row["single_fused_over_single_to"] = round(med["single"] / med["single_to"], 4)
            row["g200_over_g256"] = round(med["g200"] / med["g256"], 4)
        if "parent_a" in variants:
            row["cycle_over_parent"] = [round(med["cycle_" + x] / med["parent_" + y], 5) for x in "ab" for y in "ab"]
            row["parent_aa_spread"] = round(abs(med["parent_a"] - med["parent_b"]) / min(med["parent_a"], med["parent_b"]), 5)
        rows[shape] = row
        print("%-8s %6d entries  " % (shape, k) + "  ".join("%s %.4f" % (v, med[v]) for v in variants) + " ms", flush=True)
        for b in (sbuf, dbuf, tb, tb_plain, ws, res, res_base):
            b.free()
    st.destroy()
    out = {"tool": "tools/bench_cycle_digest_table.py", "unit": "TB/s of n bytes cycled per pass", "when": time.strftime("%Y-%m-%dT%H:%M:%S"), "warmup": a.warmup,
           "steps": a.steps, "key": KEY, "shipped_grid": shipped, "table_kernel_source_hash": M.table_kernel_source_hash(),
           "other_table_kernel_source_hash": other.modgpu_table_kernel_source_hash().decode() if other is not None else None, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
