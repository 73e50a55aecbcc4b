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
import ctypes

import bench_common as H

M, Stream, hip, _ok = H.setup()

VARIANTS = ("inplace", "to_aligned", "to_mis_a", "to_mis_b", "copy_inplace")
KEY = M.KEY_PS4
D2D = 3  # hipMemcpyDeviceToDevice


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
    a = H.arguments("r07_cycle_to.json", sizes_mib="64,256,1024,4096").parse_args()
    assert a.warmup >= 3 and a.steps >= 20, "at least 3 warm-ups and 20 timed steps"
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch between the two source forms
    st = Stream()
    rows = {}
    for mib in [int(x) for x in a.sizes_mib.split(",")]:
        n = mib << 20
        sbuf, dbuf = M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64)
        H.fill(sbuf, n + 64)
        src, dst = sbuf.ptr, dbuf.ptr  # hipMalloc: 256-byte aligned, phase 0
        times, info, _ = H.measure(st, VARIANTS, lambda v: one_pass(v, src, dst, n, st), a.warmup, a.steps)
        M.debug_set_to_form(None)
        row = {"bytes": n, "kernel": {v: info[v]["kernel"] for v in VARIANTS}}
        for v in VARIANTS:
            row[v] = H.stats(times[v], n, 2, "TBps_2n")
        row["to_aligned_over_inplace"] = round(row["inplace"]["median_ms"] / row["to_aligned"]["median_ms"], 4)
        row["to_aligned_over_copy_inplace"] = round(row["copy_inplace"]["median_ms"] / row["to_aligned"]["median_ms"], 4)
        row["mis_a_over_mis_b"] = round(row["to_mis_b"]["median_ms"] / row["to_mis_a"]["median_ms"], 4)
        rows[str(n)] = row
        print("%5d MiB  " % mib + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps_2n"]) for v in VARIANTS), flush=True)
        sbuf.free()
        dbuf.free()
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_cycle_to.py", "TB/s of 2n algorithmic bytes per pass (n read + n written)", a),
                            "key": KEY, "to_kernel_source_hash": M.to_kernel_source_hash(), "kernel_source_hash": M.kernel_source_hash(),
                            "misaligned": "src phase 5, dst phase 0", "sizes": rows})


if __name__ == "__main__":
    main()
