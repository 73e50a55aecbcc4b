#!/usr/bin/env python3
"""The resident slice of large in-place passes (cycle_keep_kernel.hip) against the main work-queue kernel on the same buffer.

The project's protocol: one process, one stream, HIP events recorded on that stream around every single pass; the variants alternate step
by step so drift hits all of them alike; 3 warm-ups, the median of 20.  Rate unit: 2n bytes per pass (n read + n written).

    variants   main, main_again    modgpu_cycle_queue_kernel<4, 1024> (route off): their medians' distance is the A/A spread
               run0                the keep kernel with no chunk resident (must equal main within the A/A spread: the copy is a copy)
               s64 s128 s192 s224  strided: mask 255, `run` chunks of 64 KiB resident out of every 16 MiB, S MiB of the buffer in all
               c192                contiguous: one slice of 192 MiB (a mask as large as the buffer)
    modes      warm   the same buffer pass after pass, as bench.py does.  A variant's pass is timed directly behind an untimed pass of
                      the SAME variant (which leaves the cache as that policy leaves it -- otherwise a row would be timed on what its
                      neighbour in the rotation left behind); the untimed pass's own time is recorded as `after_other_ms`.
               cold   768 MiB of hipMemset on another allocation in front of every timed pass (profiles/r02_tune_cycle_sizes_cold.txt's
                      method): nothing of the buffer is in the cache, whatever was stored how.

    python tools/bench_keep.py [--sizes-mib 4096,1024] [--warmup 3] [--steps 20] [--out profiles/r13_keep.json]
"""
import ctypes

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY = M.KEY_PS4
CHUNK = 65536
STRIDED = (64, 128, 192, 224)
FLUSH_BYTES = 768 << 20


def policies(n):
    """variant -> (min_bytes, mask, run) for modgpu_debug_set_keep"""
    out = {"main": (M.KEEP_OFF, 0, 0), "main_again": (M.KEEP_OFF, 0, 0), "run0": (1, 255, 0)}
    for s in STRIDED:
        out["s%d" % s] = (1, 255, (s << 20) * 256 // n)
    period = 1
    while period * CHUNK < n:
        period *= 2
    out["c192"] = (1, period - 1, min((192 << 20) // CHUNK, n // CHUNK))
    return out


def main():
    a = H.arguments("r13_keep.json", sizes_mib="4096,1024").parse_args()
    assert a.warmup >= 3 and a.steps >= 20, "at least 3 warm-ups and 20 timed steps"
    M.use_testing_flavour()
    st = Stream()
    flush = M.DeviceBuffer(FLUSH_BYTES)
    rows = {}
    tile = H.tile(1 << 26)
    for n in [int(x) << 20 for x in a.sizes_mib.split(",")]:
        buf = M.DeviceBuffer(n)
        H.fill(buf, n, tile_bytes=1 << 26)
        pol = policies(n)
        variants = list(pol)

        def one_pass(v):
            M.debug_set_keep(*pol[v])
            M.cycle_device(buf.ptr, n, KEY, 0, stream=st.handle)
            return M.last_launch()

        def timed(v):
            return H.timed(st, one_pass, v)

        launch = {}
        for v in variants:
            for _ in range(a.warmup):
                info = one_pass(v)
            launch[v] = {"kernel": info["kernel"], "variant": info["variant"], "grid": info["grid"], "main_groups": info["main_groups"],
                         "mask": pol[v][1], "run": pol[v][2], "resident_mib": 0 if v.startswith("main") else round(n / CHUNK / (pol[v][1] + 1) * pol[v][2] * CHUNK / 2**20, 1)}
        st.sync()
        warm, after_other, cold = ({v: [] for v in variants} for _ in range(3))
        for _ in range(a.steps):
            for v in variants:
                after_other[v].append(timed(v))
                warm[v].append(timed(v))
        for _ in range(a.steps):
            for v in variants:
                _ok(hip().hipMemsetAsync(ctypes.c_void_p(flush.ptr), 0, ctypes.c_size_t(FLUSH_BYTES), ctypes.c_void_p(st.handle)), "hipMemsetAsync")
                cold[v].append(timed(v))
        # an even number of passes per variant and mode: the buffer holds the tile again
        st.sync()
        assert np.array_equal(buf.download(1 << 20, offset=n - (1 << 20)), tile[(n - (1 << 20)) % tile.size:][:1 << 20]), "the passes did not cancel"
        row = {"bytes": n, "launch": launch, "warm": {}, "cold": {}, "after_other": {}}
        for v in variants:
            row["warm"][v] = H.stats(warm[v], n, 2, "TBps_2n")
            row["cold"][v] = H.stats(cold[v], n, 2, "TBps_2n")
            row["after_other"][v] = H.stats(after_other[v], n, 2, "TBps_2n")
        for mode in ("warm", "cold"):
            m = {v: row[mode][v]["median_ms"] for v in variants}
            row[mode + "_aa_spread_of_main"] = round(H.spread(m["main"], m["main_again"]), 5)
            row[mode + "_over_main"] = {v: round(m[v] / m["main"], 5) for v in variants}
        rows[str(n)] = row
        for mode in ("warm", "cold"):
            print("%5d MiB %s  " % (n >> 20, mode) + "  ".join("%s %.4f" % (v, row[mode][v]["median_ms"]) for v in variants)
                  + "  | A/A %.4f" % row[mode + "_aa_spread_of_main"], flush=True)
        buf.free()
    M.debug_set_keep(0, 0, 0)
    flush.free()
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_keep.py", "TB/s of 2n bytes per pass (n read + n written)", a), "key": KEY,
                            "flush_bytes_cold": FLUSH_BYTES, "kernel_source_hash": M.kernel_source_hash(),
                            "keep_kernel_source_hash": M.keep_kernel_source_hash(), "sizes": rows})


if __name__ == "__main__":
    main()
