"""The harness of the event-timed tools/bench_*.py, once: the method behind every figure of DESIGN.md 4.6 to 4.18.  One process, one
stream, HIP events recorded on that stream around every single pass; the variants alternate step by step so drift hits all of them
alike; the median of the timed steps.  A tool keeps what is its own -- its variants and one_pass, its checks before timing, its
derived ratios and bars, its JSON keys -- and takes the rest from here.

Importing this module changes nothing (no environment variable, no library loaded) but sys.path; a tool calls setup() first."""
import argparse
import ctypes
import functools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
M = hip = _ok = None  # set by setup()


def setup():
    """Forbids the library's host loop (read once when libmodgpu.so is loaded, so before anything loads it) and imports what every
    tool needs: (modulate_amd, hip_rt.Stream, hip_rt.hip, hip_rt._ok).  tests/hip_rt.py: streams over the HIP runtime libmodgpu.so
    brought in."""
    global M, hip, _ok
    os.environ["MODGPU_REQUIRE_GPU"] = "1"
    import modulate_amd
    import hip_rt
    M, hip, _ok = modulate_amd, hip_rt.hip, hip_rt._ok
    return M, hip_rt.Stream, hip, _ok


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


@functools.lru_cache(maxsize=None)
def _events():
    return Event(), Event()


def timed(st, one_pass, v):
    """ms of one_pass(v) between two events recorded on `st`"""
    e0, e1 = _events()
    e0.record(st)
    one_pass(v)
    e1.record(st)
    return elapsed_ms(e0, e1)


@functools.lru_cache(maxsize=None)
def tile(tile_bytes=1 << 24):
    return np.random.default_rng(1).integers(0, 256, size=tile_bytes, dtype=np.uint8)


def fill(buf, n, offset=0, tile_bytes=1 << 24):
    """n bytes of `buf` from `offset`: the seeded tile, over and over"""
    t = tile(tile_bytes)
    for off in range(0, n, t.size):
        buf.upload(t[:min(t.size, n - off)], offset=offset + off)


def arguments(out, warmup=3, steps=20, **lists):
    """the parser every tool starts from: its list of sizes or shapes (e.g. shapes="4g,config4"), --warmup, --steps, --out"""
    ap = argparse.ArgumentParser()
    for name, default in lists.items():
        ap.add_argument("--" + name.replace("_", "-"), default=default)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))
    return ap


def measure(st, variants, one_pass, warmup, steps, warm_order=None, before_warmup=None, after_warmup=None):
    """The alternating measurement.  Per variant, in `warm_order` (default: `variants`): before_warmup(v), `warmup` passes, a
    synchronise, after_warmup(v, info) -- where a tool checks what the passes computed.  Then `steps` rounds, each timing every
    variant once.  Returns (times, info, launches): per variant the ms of every step, what its last warm-up pass returned (the
    tool's one_pass returns M.last_launch()), and the launches one pass took by the library's counter."""
    info, launches = {}, {}
    for v in warm_order or variants:
        if before_warmup:
            before_warmup(v)
        before = M.path_stats()["gpu_launches"]
        for _ in range(warmup):
            info[v] = one_pass(v)
        launches[v] = (M.path_stats()["gpu_launches"] - before) // warmup
        st.sync()
        if after_warmup:
            after_warmup(v, info[v])
    times = {v: [] for v in variants}
    for _ in range(steps):
        for v in variants:
            times[v].append(timed(st, one_pass, v))
    return times, info, launches


def launch_row(info, launches_per_pass=None):
    """what a profile records of a variant's launch"""
    row = {"kernel": info["kernel"], "variant": info["variant"], "grid": info["grid"]}
    if launches_per_pass is not None:
        row["launches_per_pass"] = launches_per_pass
    return row


def stats(times, nbytes, factor, rate_key):
    """median (the upper one of an even count), min and max of `times` in ms, and the rate of factor * nbytes bytes at the median
    in TB/s, under the tool's name for it (TBps, TBps_n, TBps_2n)"""
    t = sorted(times)
    med = t[len(t) // 2]
    return {"median_ms": round(med, 5), "min_ms": round(t[0], 5), "max_ms": round(t[-1], 5),
            rate_key: round(factor * nbytes / (med * 1e-3) / 1e12, 4)}


def spread(a, b):
    return abs(a - b) / min(a, b)


def add_speedups(row, variants):
    """row[v + "_speedup_over_base"] for every variant but `base`, if `base` ran"""
    if "base" in variants:
        for v in variants:
            if v != "base":
                row[v + "_speedup_over_base"] = round(row["base"]["median_ms"] / row[v]["median_ms"], 4)


def aa_spread(row, v):
    """the A/A spread of variant v: the distance of its median from that of its second run in the same rotation, v + "2" """
    return round(spread(row[v]["median_ms"], row[v + "2"]["median_ms"]), 5)


def measure_with_aa(st, variants, one_pass, warmup, steps, nbytes):
    """measure() of a rotation in which every variant v runs a second time as v + "2", as a row: bytes, launch, the stats of every
    variant at nbytes bytes per pass, every v's A/A spread and, as `aa_spread`, the largest of them."""
    times, info, _ = measure(st, variants, one_pass, warmup, steps)
    row = {"bytes": nbytes, "launch": info}
    for v in variants:
        row[v] = stats(times[v], nbytes, 1, "TBps")
    firsts = [v for v in variants if not v.endswith("2")]
    for v in firsts:
        row[v + "_aa_spread"] = aa_spread(row, v)
    row["aa_spread"] = max(row[v + "_aa_spread"] for v in firsts)
    return row


def other_library(path, names, like):
    """another build's libmodgpu.so loaded into this process, `names` declared as the loaded library `like` declares them"""
    lib = ctypes.CDLL(path)
    for name in names:
        getattr(lib, name).restype = getattr(like, name).restype
        getattr(lib, name).argtypes = getattr(like, name).argtypes
    return lib


def profile_head(tool, unit, a):
    """the keys every profile begins with"""
    return {"tool": "tools/" + tool, "unit": unit, "when": time.strftime("%Y-%m-%dT%H:%M:%S"), "warmup": a.warmup, "steps": a.steps}


def write_profile(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path)


SINGLE_ENTRY = {"64k": 64 << 10, "1m": 1 << 20, "16m": 16 << 20, "4g": 4 << 30, "4g_p5": 4 << 30, "4gdirty": 4 << 30}
_TABLES = ("4g", "16x256m", "16kx64k", "config4")
_DIGESTS = ("64k", "1m", "16m", "4g", "4g_p5", "16kx64k", "config4")
LAYOUT_SHAPES = {"table": _TABLES, "rekey_table": _TABLES, "verify_table": _TABLES + ("4g_p5", "config4dirty"),
                 "verify_rekey_table": _TABLES + ("4g_p5", "config4dirty", "4gdirty", "64k", "1m", "16m"),
                 "digest_table": _DIGESTS, "cycle_digest_table": _DIGESTS}


def table_layout(tool, shape):
    """The table of tools/bench_<tool>.py at `shape`, as offsets into the tool's buffers (int64 arrays), seeded:
        table               (sizes, src offsets, dst offsets, stream offsets, src bytes, dst bytes)
        rekey_table         (sizes, src offsets, dst offsets, offsets under key_from, offsets under key_to, src bytes, dst bytes)
        verify_table        (sizes, src offsets, comparand offsets, stream offsets, src bytes, comparand bytes)
        verify_rekey_table  (sizes, src offsets, comparand offsets, off_from, off_to, src bytes, comparand bytes)
        digest_table        (sizes, src offsets from a chunk-aligned base, stream offsets, src bytes)
        cycle_digest_table  (sizes, dst offsets and src offsets from chunk-aligned bases, stream offsets, bytes of an arena)
    4g / 64k / 1m / 16m: one entry (4g_p5: its source at phase 5); 16x256m: 16 co-aligned entries; 16kx64k: 16 384 entries of 64 KiB
    at random phases; config4: 100 000 entries of [0, 64 KiB], packed as in a part (rekey_table: every entry after a change moves).
    The draws from the generator come in each tool's own order, so every tool keeps the table its recorded profiles were taken on."""
    if shape not in LAYOUT_SHAPES[tool]:
        raise ValueError(shape)
    rng = np.random.default_rng(0x4D6F6475)
    single = shape in SINGLE_ENTRY

    def zeros(k):
        return np.zeros(k, np.int64)

    if single:
        sz = np.array([SINGLE_ENTRY[shape]], np.int64)
        src, dst = zeros(1) + (5 if shape == "4g_p5" else 0), zeros(1)
    elif shape == "16x256m":
        sz = np.full(16, 256 << 20, np.int64)
        src = dst = np.arange(16, dtype=np.int64) * (256 << 20)
    elif shape == "16kx64k":
        sz = np.full(16384, 65536, np.int64)
        pitch = 65536 + (32 if tool == "cycle_digest_table" else 16)

        def draw():
            return np.arange(16384, dtype=np.int64) * pitch + rng.integers(0, 16, size=16384)

        if tool == "cycle_digest_table":
            dst = draw()
            src = draw()
        else:
            src = draw()
            dst = draw() if tool != "digest_table" else None
    else:
        sz = rng.integers(0, 65537, size=100000).astype(np.int64)
        src = dst = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)
        if tool == "rekey_table":
            dst = src + np.cumsum(rng.integers(0, 2, size=sz.size) * rng.integers(1, 4096, size=sz.size))

    def room(offsets):
        return int(sz[0] if single else offsets[-1] + sz[-1]) + 64

    if tool == "table":
        return sz, src, dst, src if shape == "config4" else zeros(sz.size), room(src), room(dst)
    if tool == "rekey_table":
        return sz, src, dst, src, dst, room(src), room(dst)
    if tool == "verify_table":
        return sz, src, dst, dst, room(src), room(dst)
    if tool == "verify_rekey_table":
        return sz, src, dst, zeros(1) + 7 if single else src, dst + (1 << 40) + (0 if shape == "16kx64k" else 3), room(src), room(dst)
    offs = zeros(1) + 12345 if single else src
    if tool == "digest_table":
        return sz, src, offs, room(src)
    return sz, dst, src, offs, room(dst)
