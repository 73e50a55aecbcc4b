#!/usr/bin/env python3
"""The digest check (modgpu_digest_check_device: the records of a digest call against a manifest of Adler-32 values, on the device, in
two launches) against what a caller had before it.  One process, one stream, on the recorded digest table layouts.  Three figures per
shape:

    (a) check        the check alone -- the init launch and the check launch -- by HIP events recorded on the stream around every pass
    (b) device       digest table + check, from the first call to the answer on the host (the summary read back; the bitmap too when an
                     entry is bad -- none is, here), by wall clock
    (c) host         the route without the check: digest table, a synchronise, modgpu_digest_results (32 bytes per entry downloaded and
                     closed on the host), a numpy compare of the closed values with the manifest, by wall clock

(b) and (c) alternate step by step so drift hits both alike; the median of the timed steps.  Before anything is timed the manifest is
taken from the records themselves, the check must find it clean, and with three values of the manifest changed it must name those three.

    python tools/bench_digest_check.py [--shapes config4,16kx64k] [--warmup 3] [--steps 20] [--out profiles/r20_digest_check.json]
"""
import time

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY = M.KEY_PS3


def median(times):
    t = sorted(times)
    return round(t[len(t) // 2], 5)


def main():
    a = H.arguments("r20_digest_check.json", shapes="config4,16kx64k").parse_args()
    assert a.warmup >= 1 and a.steps >= 1
    st = Stream()
    rows = {}
    for shape in a.shapes.split(","):
        sz, so, offs, sn = H.table_layout("digest_table", shape)
        n_bytes, k = int(sz.sum()), sz.size
        sbuf = M.DeviceBuffer(sn + 65536)
        base = -sbuf.ptr % 65536  # the layout's offsets count from a chunk edge
        H.fill(sbuf, sn, offset=base)
        t = M.table(k)
        t["src"] = sbuf.ptr + base + so
        t["n"], t["stream_off"], t["key"] = sz, offs, M.as_int32(KEY)
        tb = M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        ws = M.DeviceBuffer(M.digest_table_workspace_bytes(k))
        res, expect = M.DeviceBuffer(32 * k), M.DeviceBuffer(4 * k)
        summary, bits = M.DeviceBuffer(32), M.DeviceBuffer(M.digest_check_bits_bytes(k))

        def digest():
            M.digest_table_device(tb, res, ws, n=k, stream=st.handle)

        def check():
            M.digest_check_device(res, expect, k, ws, summary, bits, stream=st.handle)
            return M.last_launch()

        def device_route():
            digest()
            check()
            st.sync()
            return M.digest_check_result(summary, k, bits)

        def host_route():
            digest()
            st.sync()
            return np.flatnonzero(M.digest_results(res, k)[1] != manifest)

        # the manifest is what the records close to; the check finds it clean, and names three changed values
        digest()
        st.sync()
        assert M.table_status(ws) is None
        manifest = M.digest_results(res, k)[1].copy()
        expect.upload(manifest.view(np.uint8))
        assert device_route()[:2] == (0, None) and host_route().size == 0, shape
        planted = sorted({0, k // 2, k - 1})
        wrong = manifest.copy()
        wrong[planted] ^= np.uint32(1 << 16)
        expect.upload(wrong.view(np.uint8))
        got = device_route()
        assert (got[0], got[1], got[2].tolist()) == (len(planted), 0, planted), (shape, got)
        expect.upload(manifest.view(np.uint8))

        times, info, launches = H.measure(st, ("check",), lambda v: check(), a.warmup, a.steps)
        assert info["check"]["variant"] == 19 and launches["check"] == 2, info
        wall = {"device": [], "host": []}
        for step in range(a.warmup + a.steps):
            for name, route in (("device", device_route), ("host", host_route)):
                t0 = time.perf_counter()
                route()
                if step >= a.warmup:
                    wall[name].append((time.perf_counter() - t0) * 1e3)
        ts = sorted(times["check"])
        row = {"entries": int(k), "bytes": n_bytes, "launch": H.launch_row(info["check"], launches["check"]),
               "check_ms": {"median_ms": median(ts), "min_ms": round(ts[0], 5), "max_ms": round(ts[-1], 5)},
               "device_route_wall_ms": {"median_ms": median(wall["device"]), "min_ms": round(min(wall["device"]), 5)},
               "host_route_wall_ms": {"median_ms": median(wall["host"]), "min_ms": round(min(wall["host"]), 5)},
               "bytes_read_back": {"device_route": 32, "host_route": 32 * int(k)}}
        row["device_over_host"] = round(row["device_route_wall_ms"]["median_ms"] / row["host_route_wall_ms"]["median_ms"], 4)
        rows[shape] = row
        print("%-8s %6d entries  (a) check %.4f ms  (b) digest table + check %.4f ms  (c) digest table + results + compare %.4f ms  (b)/(c) %.3f"
              % (shape, k, row["check_ms"]["median_ms"], row["device_route_wall_ms"]["median_ms"], row["host_route_wall_ms"]["median_ms"], row["device_over_host"]), flush=True)
        for b in (sbuf, tb, ws, res, expect, summary, bits):
            b.free()
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_digest_check.py", "ms: (a) by events, (b) and (c) by wall clock from the first call to the answer on the host", a),
                            "key": KEY, "verify_table_kernel_source_hash": M.verify_table_kernel_source_hash(), "shapes": rows})


if __name__ == "__main__":
    main()
