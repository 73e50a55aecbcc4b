#!/usr/bin/env python3
"""The verify pass (modgpu_verify_device: is `expect` what the cipher makes of `src`? -- a read-only pass over 2n bytes) against the
out-of-place pass on the same buffers (modgpu_cycle_device_to: the same 2n bytes and the same keystream work, plus stores), which is
the yardstick ISSUE/DESIGN 4.10 sets.  One process, one stream, HIP events recorded on that stream around every single pass; the variants
alternate step by step so drift hits all of them alike.  Rate unit: 2n bytes per pass (verify reads 2n; the out-of-place pass reads n
and writes n).

    variants   verify        clean, expect and src at phase 0, shipped grid (one workgroup per CU)
               verify_200    the same on the out-of-place kernel's grid (25 workgroups per 32 CUs): the grid A/B
               to, to_again  modgpu_cycle_device_to on the same buffers, twice per step: their medians' distance is the A/A spread
               verify_mis    clean, src at phase 5 (the v_alignbyte_b32 funnel);   to_mis   modgpu_cycle_device_to at the same phases
               verify_wrong  the wrong key: every byte takes the slow path
    at the largest size also
               verify_batch / to_batch   16 equal entries in one call
               route_today   modgpu_cycle_device_to into scratch + modgpu_d2h of the scratch (wall clock, 3 runs; the host compare not counted)

    python tools/bench_verify.py [--sizes-kib 64,1024,16384,4194304] [--warmup 3] [--steps 20] [--out profiles/r11_verify.json]
"""
import ctypes
import time

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

SINGLE = ("verify", "verify_200", "to", "to_again", "verify_mis", "to_mis", "verify_wrong")
BATCH = ("verify_batch", "to_batch")
KEY, WRONG = M.KEY_PS4, M.KEY_PS3


def one_pass(v, B, n, st):
    """B: src (+64 bytes of room), dst (= cipher of src at phase 0), dst_mis (= cipher of src + 5), res (16 results)"""
    s = st.handle
    if v in ("verify", "verify_200", "verify_wrong"):
        M.debug_set_verify_form(200 if v == "verify_200" else 0)
        M.verify_device(B["dst"], B["src"], WRONG if v == "verify_wrong" else KEY, 0, result=B["res"], n=n, stream=s)
    elif v == "verify_mis":
        M.debug_set_verify_form(0)
        M.verify_device(B["dst_mis"], B["src"] + 5, KEY, 0, result=B["res"], n=n, stream=s)
    elif v in ("to", "to_again"):
        M.cycle_device_to(B["dst"], B["src"], n, KEY, 0, stream=s)
    elif v == "to_mis":
        M.cycle_device_to(B["dst_mis"], B["src"] + 5, n, KEY, 0, stream=s)
    else:
        part = n // 16
        d = [B["dst"] + i * part for i in range(16)]
        sp = [B["src"] + i * part for i in range(16)]
        offs = [i * part for i in range(16)]
        if v == "verify_batch":
            M.debug_set_verify_form(0)
            M.verify_batch_device(d, sp, [part] * 16, KEY, B["res"], stream_offs=offs, stream=s)
        else:
            M.cycle_batch_device_to(d, sp, [part] * 16, KEY, stream_offs=offs, stream=s)
    return M.last_launch()


def main():
    a = H.arguments("r11_verify.json", sizes_kib="64,1024,16384,4194304").parse_args()
    assert a.warmup >= 3 and a.steps >= 20, "at least 3 warm-ups and 20 timed steps"
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the grid switch
    st = Stream()
    rows = {}
    sizes = [int(x) << 10 for x in a.sizes_kib.split(",")]
    for n in sizes:
        sbuf, dbuf, mbuf, rbuf = M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64), M.DeviceBuffer(32 * 16)
        H.fill(sbuf, n + 64)
        B = {"src": sbuf.ptr, "dst": dbuf.ptr, "dst_mis": mbuf.ptr, "res": rbuf.ptr}  # hipMalloc: 256-byte aligned, phase 0
        variants = SINGLE + (BATCH if n == max(sizes) and n % 16 == 0 else ())
        order = [v for v in variants if v.startswith("to")] + [v for v in variants if not v.startswith("to")]  # the `to` passes make `expect`
        seen = {}

        def checked(v, info):
            if v.startswith("verify"):
                r = M.verify_results(rbuf, 16 if v == "verify_batch" else 1)
                seen[v] = {"mismatches": int(r["mismatches"].sum()), "first_mismatch": int(r["first_mismatch"].min()), "n": int(r["n"].sum())}
                assert seen[v]["n"] == n and (seen[v]["mismatches"] == 0) == (v != "verify_wrong"), (v, seen[v])

        times, info, _ = H.measure(st, variants, lambda v: one_pass(v, B, n, st), a.warmup, a.steps, warm_order=order, after_warmup=checked)
        M.debug_set_verify_form(0)
        row = {"bytes": n, "launch": {v: H.launch_row(info[v]) for v in order}, "results": seen}
        for v in variants:
            row[v] = H.stats(times[v], n, 2, "TBps_2n")
        med = {v: row[v]["median_ms"] for v in variants}
        spread = H.spread(med["to"], med["to_again"])
        bound = max(1.05, 1 + 2 * spread)
        row["aa_spread_of_to"] = round(spread, 5)
        row["bound"] = round(bound, 5)
        row["verify_over_to"] = round(med["verify"] / med["to"], 4)
        row["verify_200_over_to"] = round(med["verify_200"] / med["to"], 4)
        row["verify_mis_over_to_mis"] = round(med["verify_mis"] / med["to_mis"], 4)
        row["verify_wrong_over_verify"] = round(med["verify_wrong"] / med["verify"], 4)
        if "verify_batch" in med:
            row["verify_batch_over_to_batch"] = round(med["verify_batch"] / med["to_batch"], 4)
        if n == max(sizes):  # the route a caller has today: out of place into scratch, then the scratch across the link
            host = np.empty(n, np.uint8)
            walls = []
            for _ in range(3):
                st.sync()
                t0 = time.perf_counter()
                M.cycle_device_to(B["dst"], B["src"], n, KEY, 0, stream=st.handle)
                st.sync()
                M.lib().modgpu_d2h(ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(B["dst"]), n, -1)
                walls.append((time.perf_counter() - t0) * 1e3)
            row["route_today"] = {"wall_ms": [round(w, 3) for w in walls], "median_ms": round(sorted(walls)[1], 3), "host_memory": "pageable"}
            row["route_today_over_verify"] = round(sorted(walls)[1] / med["verify"], 2)
            del host
        rows[str(n)] = row
        print("%8d KiB  " % (n >> 10) + "  ".join("%s %.4f ms" % (v, med[v]) for v in variants) + "  | verify/to %.3f mis %.3f bound %.3f"
              % (row["verify_over_to"], row["verify_mis_over_to_mis"], bound), flush=True)
        for b in (sbuf, dbuf, mbuf, rbuf):
            b.free()
    st.destroy()
    H.write_profile(a.out, {
        **H.profile_head("bench_verify.py", "TB/s of 2n bytes per pass (verify: 2n read; out of place: n read + n written)", a),
        "key": KEY, "wrong_key": WRONG,
        "rule": "verify's median <= the out-of-place median x max(1.05, 1 + 2 x A/A spread of the out-of-place pass in the same run)",
        "verify_kernel_source_hash": M.verify_kernel_source_hash(), "to_kernel_source_hash": M.to_kernel_source_hash(),
        "misaligned": "src phase 5, expect / dst phase 0", "sizes": rows})


if __name__ == "__main__":
    main()
