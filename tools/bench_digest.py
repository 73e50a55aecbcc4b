#!/usr/bin/env python3
"""The digest pass (modgpu_digest_device: Adler-32 of what the cipher makes of `src` -- a pass that reads n bytes and writes 32) against
the two yardsticks DESIGN 4.16 sets: digest only against the verify pass on the same source (verify reads twice the bytes with the same
keystream work), fused against the out-of-place pass on the same buffers (the same loads, stores and keystream work, plus the sums).
tools/bench_verify.py's method: one process, one stream, HIP events recorded on that stream around every single pass; the variants
alternate step by step so drift hits all of them alike; 3 warm-ups, median of 20.

    variants   digest, digest_p5     digest only, source at phase 0 / at phase 5
               verify, verify_p5     modgpu_verify_device on the same source (expect at phase 0)
               fused, fused_p5       digest with a destination (phase 0), source at phase 0 / 5 (the v_alignbyte_b32 funnel)
               digest_g200, fused_g256   the grid A/B: digest only on the out-of-place kernel's grid (25 workgroups per 32 CUs), fused
                                     on one workgroup per CU
               to, to_again, to_p5   modgpu_cycle_device_to on the same buffers; to / to_again: their medians' distance is the A/A spread
               to_parent             the same call from a library built from the parent commit (--parent-lib), interleaved: has the
                                     second loop moved the first?
    at the largest size also
               digest_batch          16 equal entries in one call, digest only
               route_today           modgpu_cycle_device_to into scratch + modgpu_d2h + zlib.adler32 (wall clock, 3 runs), whose value
                                     the digest pass must reproduce

    python tools/bench_digest.py [--sizes-kib 64,1024,16384,4194304] [--warmup 3] [--steps 20] [--parent-lib PATH] [--out profiles/r16_digest.json]
"""
import ctypes
import time
import zlib

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

SINGLE = ("digest", "digest_g200", "digest_p5", "verify", "verify_p5", "fused", "fused_g256", "fused_p5", "to", "to_again", "to_p5")
GRID = {"digest_g200": 200, "fused_g256": 256}  # the grid A/B: each mode on the other's shipped grid
KEY = M.KEY_PS4
_vp = ctypes.c_void_p


def one_pass(v, B, n, st, parent):
    """B: src (+64 bytes of room), dst (= cipher of src at phase 0), dst_p5 (= cipher of src + 5), res (16 records), vres (a verify result)"""
    s = st.handle
    src = B["src"] + (5 if v.endswith("_p5") else 0)
    dst = B["dst_p5"] if v.endswith("_p5") else B["dst"]
    M.debug_set_digest_grid(GRID.get(v, 0))
    if v in ("digest", "digest_g200", "digest_p5"):
        M.digest_device(src, KEY, 0, result=B["res"], n=n, stream=s)
    elif v in ("fused", "fused_g256", "fused_p5"):
        M.digest_device(src, KEY, 0, dst=dst, result=B["res"], n=n, stream=s)
    elif v in ("verify", "verify_p5"):
        M.verify_device(dst, src, KEY, 0, result=B["vres"], n=n, stream=s)
    elif v in ("to", "to_again", "to_p5"):
        M.cycle_device_to(dst, src, n, KEY, 0, stream=s)
    elif v == "to_parent":
        rc = parent.modgpu_cycle_device_to(_vp(dst), _vp(src), ctypes.c_uint64(n), ctypes.c_int32(M.as_int32(KEY)), ctypes.c_uint64(0), -1, _vp(s))
        assert rc == 0, rc
        return None
    else:
        part = n // 16
        M.digest_batch_device([B["src"] + i * part for i in range(16)], [part] * 16, KEY, B["res"], stream_offs=[i * part for i in range(16)], stream=s)
    return M.last_launch()


def main():
    ap = H.arguments("r16_digest.json", sizes_kib="64,1024,16384,4194304")
    ap.add_argument("--parent-lib", default=None, help="libmodgpu.so built from the parent commit: modgpu_cycle_device_to before / after")
    a = ap.parse_args()
    assert a.warmup >= 3 and a.steps >= 20, "at least 3 warm-ups and 20 timed steps"
    parent = ctypes.CDLL(a.parent_lib) if a.parent_lib else None
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the grid switch
    st = Stream()
    rows = {}
    sizes = [int(x) << 10 for x in a.sizes_kib.split(",")]
    for n in sizes:
        sbuf, dbuf, mbuf, rbuf, vbuf = M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64), M.DeviceBuffer(32 * 16), M.DeviceBuffer(32)
        H.fill(sbuf, n + 64)
        B = {"src": sbuf.ptr, "dst": dbuf.ptr, "dst_p5": mbuf.ptr, "res": rbuf.ptr, "vres": vbuf.ptr}  # hipMalloc: 256-byte aligned, phase 0
        largest = n == max(sizes) and n % 16 == 0
        variants = SINGLE + (("to_parent",) if parent else ()) + (("digest_batch",) if largest else ())
        order = [v for v in variants if v.startswith("to")] + [v for v in variants if not v.startswith("to")]  # the `to` passes make `expect`
        seen = {}

        def checked(v, info):
            if v.startswith("verify"):
                r = M.verify_results(vbuf, 1)
                assert int(r["mismatches"][0]) == 0 and int(r["n"][0]) == n, (v, r)
            elif v.startswith(("digest", "fused")):
                recs, adlers = M.digest_results(rbuf, 16 if v == "digest_batch" else 1)
                assert int(recs["n"].sum()) == n, (v, recs)
                seen[v] = [int(x) for x in adlers]
            if v == order[-1]:
                assert seen["digest"] == seen["fused"] and seen["digest_p5"] == seen["fused_p5"], seen

        times, info, _ = H.measure(st, variants, lambda v: one_pass(v, B, n, st, parent), a.warmup, a.steps, warm_order=order, after_warmup=checked)
        row = {"bytes": n, "launch": {v: H.launch_row(info[v]) for v in order if info[v]}, "adler32": seen}
        for v in variants:
            row[v] = H.stats(times[v], n, 1, "TBps_n")
        med = {v: row[v]["median_ms"] for v in variants}
        spread = H.spread(med["to"], med["to_again"])
        row["aa_spread_of_to"] = round(spread, 5)
        row["digest_over_verify"] = round(med["digest"] / med["verify"], 4)
        row["digest_p5_over_verify_p5"] = round(med["digest_p5"] / med["verify_p5"], 4)
        row["digest_bar"] = 1.05
        row["fused_over_to"] = round(med["fused"] / med["to"], 4)
        row["fused_p5_over_to_p5"] = round(med["fused_p5"] / med["to_p5"], 4)
        row["fused_bar"] = round(1.05 + spread, 5)
        row["digest_g200_over_digest"] = round(med["digest_g200"] / med["digest"], 4)
        row["fused_g256_over_fused"] = round(med["fused_g256"] / med["fused"], 4)
        if parent:
            row["to_over_to_parent"] = round(med["to"] / med["to_parent"], 4)
        if largest:  # the route a caller has today: out of place into scratch, the scratch across the link, a host checksum
            host = np.empty(n, np.uint8)
            walls, value = [], None
            for _ in range(3):
                st.sync()
                t0 = time.perf_counter()
                M.cycle_device_to(B["dst"], B["src"], n, KEY, 0, stream=st.handle)
                st.sync()
                t1 = time.perf_counter()
                M.lib().modgpu_d2h(_vp(host.ctypes.data), _vp(B["dst"]), n, -1)
                t2 = time.perf_counter()
                value = zlib.adler32(host) & 0xFFFFFFFF
                walls.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3])
            walls.sort(key=sum)
            row["route_today"] = {"to_d2h_zlib_ms": [[round(x, 3) for x in w] for w in walls], "median_ms": round(sum(walls[1]), 3), "host_memory": "pageable",
                                  "adler32": value}
            row["route_today_over_digest"] = round(sum(walls[1]) / med["digest"], 1)
            assert value == seen["digest"][0], (value, seen["digest"])  # the whole part, checked against zlib
            del host
        M.debug_set_digest_grid(0)
        rows[str(n)] = row
        print("%8d KiB  " % (n >> 10) + "  ".join("%s %.4f" % (v, med[v]) for v in variants) + "  ms | digest/verify %.3f p5 %.3f  fused/to %.3f p5 %.3f  A/A %.4f%s"
              % (row["digest_over_verify"], row["digest_p5_over_verify_p5"], row["fused_over_to"], row["fused_p5_over_to_p5"], spread,
                 "  to/parent %.4f" % row["to_over_to_parent"] if parent else ""), flush=True)
        for b in (sbuf, dbuf, mbuf, rbuf, vbuf):
            b.free()
    st.destroy()
    H.write_profile(a.out, {
        **H.profile_head("bench_digest.py", "TB/s of n bytes per pass (digest only reads n; fused and out of place read n and write n; verify reads 2n)", a),
        "key": KEY,
        "rules": {"digest only": "median <= verify's median x 1.05 on the same source in the same run",
                  "fused": "median <= the out-of-place median x (1.05 + A/A spread of the out-of-place pass in the same run)",
                  "to before / after": "to_over_to_parent within the A/A spread"},
        "to_kernel_source_hash": M.to_kernel_source_hash(), "verify_kernel_source_hash": M.verify_kernel_source_hash(),
        "parent_lib": bool(parent), "p5": "source at phase 5, destination / expect at phase 0", "sizes": rows})


if __name__ == "__main__":
    main()
