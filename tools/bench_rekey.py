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
import bench_common as H

M, Stream, hip, _ok = H.setup()

VARIANTS = ("fused_a", "fused_b", "fused_mis", "two_pass", "to_ceiling")
KF, KT = M.KEY_PS3, M.KEY_PS4


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
    a = H.arguments("r08_rekey.json", sizes_mib="64,256,1024,4096").parse_args()
    assert a.warmup >= 3 and a.steps >= 20, "at least 3 warm-ups and 20 timed steps"
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch between the two launch shapes
    st = Stream()
    rows = {}
    for mib in [int(x) for x in a.sizes_mib.split(",")]:
        n = mib << 20
        sbuf, dbuf = M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64)
        H.fill(sbuf, n + 64)
        src, dst = sbuf.ptr, dbuf.ptr  # hipMalloc: 256-byte aligned, phase 0
        times, info, _ = H.measure(st, VARIANTS, lambda v: one_pass(v, src, dst, n, st), a.warmup, a.steps)
        M.debug_set_rekey_form(None)
        row = {"bytes": n, "launch": {v: H.launch_row(info[v]) for v in VARIANTS}}
        for v in VARIANTS:
            row[v] = H.stats(times[v], n, 2, "TBps_2n")
        for v in ("fused_a", "fused_b", "fused_mis"):
            row[v + "_over_two_pass"] = round(row["two_pass"]["median_ms"] / row[v]["median_ms"], 4)
            row[v + "_of_ceiling"] = round(row["to_ceiling"]["median_ms"] / row[v]["median_ms"], 4)
        rows[str(n)] = row
        print("%5d MiB  " % mib + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps_2n"]) for v in VARIANTS), flush=True)
        sbuf.free()
        dbuf.free()
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_rekey.py", "TB/s of 2n algorithmic bytes per pass (n read + n written)", a),
                            "key_from": KF, "key_to": KT, "rekey_kernel_source_hash": M.rekey_kernel_source_hash(),
                            "to_kernel_source_hash": M.to_kernel_source_hash(), "kernel_source_hash": M.kernel_source_hash(),
                            "misaligned": "src phase 5, dst phase 0", "sizes": rows})


if __name__ == "__main__":
    main()
