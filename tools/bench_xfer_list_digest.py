#!/usr/bin/env python3
"""The digesting list transfers (modgpu_cycle_host_to_device_list_digest / modgpu_cycle_device_to_host_list_digest) against the route a
caller had without them, and the plain list calls against the library of the commit before the digest mode.  One process; every call is
synchronous, so each is timed on the wall clock around the call; the variants of a shape alternate step by step so drift hits all of
them alike.  All host memory is pageable.  Unit: ms per pass (median of --steps).

    shapes     config4   tests/bench_layouts.json's table/config4 (bench_common.table_layout): 100 000 files packed as in a part
               holes     1 000 holes of 64 KiB + 5 spread over the part
               1g        one entry of 1 GiB
    variants   digest    the digesting list call (records resident, side OUTPUT on the upload, INPUT on the download: the device bytes)
               two       the route before: the plain list call, then a table of the same device ranges under the identity key uploaded
                         next to it, modgpu_digest_table_device over it, a synchronise
               plain     the plain list call, and plain2, the same again: the A/A spread of the run
               parent    the plain list call of ANOTHER build of the library (--parent-lib: the commit before), loaded beside this one:
                         what the mode's uniform branches cost the calls that do not use it

    python tools/bench_xfer_list_digest.py [--shapes config4,holes,1g] [--parent-lib PATH/libmodgpu.so] [--warmup 1] [--steps 5]
                                           [--out profiles/r24_xfer_list_digest.json]
"""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_common as C  # noqa: E402
from bench_xfer_list import KEY, layout  # noqa: E402


def main():
    ap = C.arguments("r24_xfer_list_digest.json", warmup=1, steps=5, shapes="config4,holes,1g")
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    M, _, _, _ = C.setup()
    import numpy as np
    lib, vp = M.lib(), M.capi._vp
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for f in (parent.modgpu_cycle_host_to_device_list, parent.modgpu_cycle_device_to_host_list):
            f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
        parent.modgpu_xfer_kernel_source_hash.restype = ctypes.c_char_p
    shapes = a.shapes.split(",")
    lay = {s: layout(s) for s in shapes}
    room_dev = max(int((d + z).max()) for z, d, _, _ in lay.values()) + 64
    room_host = max(int((h + z).max()) for z, _, h, _ in lay.values()) + 64
    block = np.frombuffer(np.random.default_rng(7).bytes(64 << 20), np.uint8)
    host = np.tile(block, room_host // block.size + 1)[:room_host].copy()
    host_out = np.zeros(room_host, np.uint8)
    dev = M.DeviceBuffer(room_dev)
    res = {}
    for shape in shapes:
        sz, d_at, h_at, offs = lay[shape]
        total, n = int(sz.sum()), int(sz.size)
        up, down = M.table(n), M.table(n)
        up["dst"], up["src"] = dev.ptr + d_at, host.ctypes.data + h_at
        down["dst"], down["src"] = host_out.ctypes.data + h_at, dev.ptr + d_at
        for t in (up, down):
            t["n"], t["stream_off"], t["key"] = sz, offs, M.as_int32(KEY)
        dtab_host = M.table(n)  # the device ranges as they are: what the upload stored, what the download read
        dtab_host["src"], dtab_host["n"], dtab_host["key"] = dev.ptr + d_at, sz, 0
        dtab = M.DeviceBuffer(max(dtab_host.nbytes, 64))
        ws = M.DeviceBuffer(M.digest_table_workspace_bytes(n))
        rec, rec2 = M.DeviceBuffer(32 * n), M.DeviceBuffer(32 * n)

        def run(v, upload):
            t = up if upload else down
            t0 = time.perf_counter()
            if v == "digest":
                f = lib.modgpu_cycle_host_to_device_list_digest if upload else lib.modgpu_cycle_device_to_host_list_digest
                M.capi._check(f(vp(t.ctypes.data), n, 0 if upload else 1, vp(rec.ptr), -1))
            elif v == "two":
                (M.cycle_host_to_device_list if upload else M.cycle_device_to_host_list)(t)
                dtab.upload(dtab_host.view(np.uint8))
                M.digest_table_device(dtab, rec2, ws, n=n)
                dev.sync()
            elif v in ("plain", "plain2"):
                (M.cycle_host_to_device_list if upload else M.cycle_device_to_host_list)(t)
            elif v == "parent":
                f = parent.modgpu_cycle_host_to_device_list if upload else parent.modgpu_cycle_device_to_host_list
                if f(t.ctypes.data, n, -1):
                    raise SystemExit("the parent library's list call failed")
            return (time.perf_counter() - t0) * 1e3

        # what is timed computes the same: the same device image, the same records by both routes, the download undoing the upload
        variants = ("digest", "two", "plain", "plain2") + (("parent",) if parent else ())
        img = None
        for v in variants:
            run(v, True)
            got = dev.download(min(room_dev, int((d_at + sz).max())))
            assert img is None or np.array_equal(img, got), shape + ": " + v + " uploads another image"
            img = got
        del img, got
        for upload in (True, False):
            run("digest", upload)
            run("two", upload)
            ra, rb = M.digest_results(rec, n)[1], M.digest_results(rec2, n)[1]
            assert np.array_equal(ra, rb), shape + ": the digesting call's checksums differ from the two-call route's"
        for h, z in zip(h_at[:64], sz[:64]):
            assert np.array_equal(host_out[int(h):int(h + z)], host[int(h):int(h + z)]), shape + ": download did not undo the upload"
        row = {"entries": n, "bytes": total}
        for upload in (True, False):
            times, launches = {v: [] for v in variants}, {}
            for step in range(a.warmup + a.steps):
                for v in variants:
                    before = M.path_stats()["gpu_launches"]
                    ms = run(v, upload)
                    launches[v] = M.path_stats()["gpu_launches"] - before
                    if step >= a.warmup:
                        times[v].append(ms)
            med = {v: round(statistics.median(x), 4) for v, x in times.items()}
            d = {"median_ms": med, "all_ms": {v: [round(x, 4) for x in xs] for v, xs in times.items()}, "launches_per_pass": dict(launches),
                 "plain_aa_spread": round(C.spread(med["plain"], med["plain2"]), 4),
                 "digest_over_two": round(med["digest"] / med["two"], 4), "digest_over_plain": round(med["digest"] / med["plain"], 4),
                 "two_minus_digest_ms": round(med["two"] - med["digest"], 4), "digest_GBps": round(total / med["digest"] / 1e6, 2)}
            if parent:
                d["plain_over_parent"] = round(min(med["plain"], med["plain2"]) / med["parent"], 4)
                d["plain_pays_for_the_mode"] = bool(min(med["plain"], med["plain2"]) > med["parent"] * (1 + d["plain_aa_spread"]))
            d["digest_slower_than_two_beyond_aa"] = bool(med["digest"] > med["two"] * (1 + d["plain_aa_spread"]))
            row["upload" if upload else "download"] = d
            print(shape, "upload" if upload else "download", json.dumps({k: v for k, v in d.items() if k != "all_ms"}), flush=True)
        res[shape] = row
        for b in (dtab, ws, rec, rec2):
            b.free()
    doc = C.profile_head("bench_xfer_list_digest.py", "ms per synchronous call on the wall clock, median of --steps; pageable host memory", a)
    doc.update({"shapes": res, "xfer_kernel_source_hash": M.xfer_kernel_source_hash(),
                "parent_xfer_kernel_source_hash": parent.modgpu_xfer_kernel_source_hash().decode() if parent else None})
    C.write_profile(a.out, doc)
    keys = ("digest_over_two", "digest_over_plain", "plain_aa_spread", "digest_GBps") + (("plain_over_parent",) if parent else ())
    print(json.dumps({"tool": "tools/bench_xfer_list_digest.py", "shapes": {s: {d: {k: r[d][k] for k in keys} for d in ("upload", "download")} for s, r in res.items()}}))


if __name__ == "__main__":
    main()
