#!/usr/bin/env python3
"""The list transfers (modgpu_cycle_host_to_device_list / modgpu_cycle_device_to_host_list) against the routes a caller had without
them.  One process; every call is synchronous, so each is timed on the wall clock around the call; the variants of a shape alternate
step by step so drift hits all of them alike.  All host memory is pageable.  Unit: ms per pass (median of --steps).

    shapes     config4   tests/bench_layouts.json's table/config4 (bench_common.table_layout): 100 000 files packed as in a part
               holes     1 000 holes of 64 KiB + 5 spread over the part (DeviceBuffer.splice's figure), the fills packed on the host
               16x64m    16 entries of 64 MiB
               1g        one entry of 1 GiB: what taking the funnel kernels costs against the single call
    variants   list      the list call, one launch
               loop      the same entries through the single call, one by one
               single    the single call on ONE range of the same total, and single2, the same again: the A/A spread of the run
               pack      (uploads) the route without the list call: pack on the host, modgpu_h2d, modgpu_cycle_table_device from a
                         second device buffer as large as the payload, synchronise
    check      the list call's validation alone at 100 000 entries: a list whose LAST entry is refused, so that every lookup has
               happened and nothing is queued -- on the part's own layout (device ranges touch: looked up as runs) and on the same
               entries one byte shorter each (no two touch: two lookups per entry)

    python tools/bench_xfer_list.py [--shapes config4,holes,16x64m,1g] [--warmup 1] [--steps 5] [--out profiles/r23_xfer_list.json]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_common as C  # noqa: E402

KEY = 0x90CFC0AB


def layout(shape):
    """(sizes, device offsets, host offsets, stream offsets) of a shape, int64 arrays"""
    import numpy as np
    if shape == "config4":
        sz, src, _, offs, _, _ = C.table_layout("table", "config4")
        return sz, src, src.copy(), offs
    if shape == "holes":
        sz = np.full(1000, 65536 + 5, np.int64)
        dev = np.arange(1000, dtype=np.int64) * ((3 << 20) + 7) + 11
        return sz, dev, np.arange(1000, dtype=np.int64) * (65536 + 5), dev.copy()
    if shape == "16x64m":
        sz = np.full(16, 64 << 20, np.int64)
        at = np.arange(16, dtype=np.int64) * (64 << 20)
        return sz, at, at.copy(), at.copy()
    if shape == "1g":
        z = np.zeros(1, np.int64)
        return np.full(1, 1 << 30, np.int64), z, z.copy(), z.copy()
    raise ValueError(shape)


def main():
    a = C.arguments("r23_xfer_list.json", warmup=1, steps=5, shapes="config4,holes,16x64m,1g").parse_args()
    M, _, _, _ = C.setup()
    import numpy as np
    lib, vp = M.lib(), M.capi._vp
    shapes = a.shapes.split(",")
    lay = {s: layout(s) for s in shapes}
    room_dev = max(int((d + z).max()) for z, d, _, _ in lay.values()) + 64
    room_host = max(int((h + z).max()) for z, _, h, _ in lay.values()) + 64
    block = np.frombuffer(np.random.default_rng(7).bytes(64 << 20), np.uint8)
    host = np.tile(block, room_host // block.size + 1)[:room_host].copy()
    host_out = np.zeros(room_host, np.uint8)
    packed = np.zeros(max(int(z.sum()) for z, _, _, _ in lay.values()) + 64, np.uint8)
    dev, dev2 = M.DeviceBuffer(room_dev), M.DeviceBuffer(packed.size)
    res = {}
    for shape in shapes:
        sz, d_at, h_at, offs = lay[shape]
        total, n = int(sz.sum()), int(sz.size)
        up, down = M.table(n), M.table(n)
        up["dst"], up["src"] = dev.ptr + d_at, host.ctypes.data + h_at
        down["dst"], down["src"] = host_out.ctypes.data + h_at, dev.ptr + d_at
        for t in (up, down):
            t["n"], t["stream_off"], t["key"] = sz, offs, M.as_int32(KEY)
        # the route without the list call: a table in device memory from the packed copy in dev2 into the part
        ptab = M.table(n)
        ptab["dst"], ptab["src"], ptab["n"], ptab["stream_off"], ptab["key"] = dev.ptr + d_at, dev2.ptr + np.concatenate([[0], np.cumsum(sz)[:-1]]), sz, offs, M.as_int32(KEY)
        dtab = M.DeviceBuffer(max(ptab.nbytes, 64))
        dtab.upload(ptab.view(np.uint8))
        ws = M.DeviceBuffer(M.table_workspace_bytes(n))
        views = [host[int(h):int(h + z)] for h, z in zip(h_at, sz)]
        rows_up = [(int(d), int(h), int(z), int(o)) for d, h, z, o in zip(up["dst"], up["src"], sz, offs) if z]
        rows_dn = [(int(h), int(d), int(z), int(o)) for h, d, z, o in zip(down["dst"], down["src"], sz, offs) if z]
        k32 = M.as_int32(KEY)

        def run(v, upload):
            t0 = time.perf_counter()
            if v == "list":
                (M.cycle_host_to_device_list if upload else M.cycle_device_to_host_list)(up if upload else down)
            elif v == "loop":
                f = lib.modgpu_cycle_host_to_device if upload else lib.modgpu_cycle_device_to_host
                for x, y, z, o in (rows_up if upload else rows_dn):
                    if f(x, y, z, k32, o, -1):
                        raise SystemExit("single call failed: " + lib.modgpu_last_error().decode())
            elif v in ("single", "single2"):
                if upload:
                    M.cycle_host_to_device(dev.ptr, host[:total], KEY)
                else:
                    M.cycle_device_to_host(host_out[:total], dev.ptr, KEY)
            elif v == "pack":
                np.concatenate(views, out=packed[:total])
                M.capi._check(lib.modgpu_h2d(vp(dev2.ptr), vp(packed.ctypes.data), total, -1))
                M.cycle_table_device(dtab, ws, n=n)
                dev.sync()
            return (time.perf_counter() - t0) * 1e3

        # what is timed computes the same bytes: the list upload against the loop's image, the list download against the source
        run("list", True)
        img = dev.download(min(room_dev, int((d_at + sz).max())))
        run("loop", True)
        assert np.array_equal(img, dev.download(img.size)), shape + ": list upload != the single calls one by one"
        run("pack", True)
        assert np.array_equal(img, dev.download(img.size)), shape + ": list upload != pack + h2d + table"
        del img
        run("list", True)
        run("list", False)
        for h, z in zip(h_at[:64], sz[:64]):
            assert np.array_equal(host_out[int(h):int(h + z)], host[int(h):int(h + z)]), shape + ": download did not undo the upload"
        launches = {}
        row = {"entries": n, "bytes": total}
        for upload in (True, False):
            variants = ("list", "loop", "single", "single2") + (("pack",) if upload else ())
            times = {v: [] for v in variants}
            for step in range(a.warmup + a.steps):
                for v in variants:
                    before = M.path_stats()["gpu_launches"]
                    ms = run(v, upload)
                    launches[v] = M.path_stats()["gpu_launches"] - before
                    if step >= a.warmup:
                        times[v].append(ms)
            med = {v: round(statistics.median(x), 4) for v, x in times.items()}
            d = {"median_ms": med, "all_ms": {v: [round(x, 4) for x in xs] for v, xs in times.items()}, "launches_per_pass": dict(launches),
                 "single_aa_spread": round(C.spread(med["single"], med["single2"]), 4),
                 "list_over_loop": round(med["list"] / med["loop"], 4), "list_over_single": round(med["list"] / med["single"], 4),
                 "list_GBps": round(total / med["list"] / 1e6, 2), "single_GBps": round(total / med["single"] / 1e6, 2),
                 "bytes_over_single_rate_ms": med["single"]}
            if upload:
                d["list_over_pack"] = round(med["list"] / med["pack"], 4)
            row["upload" if upload else "download"] = d
            print(shape, "upload" if upload else "download", json.dumps({k: v for k, v in d.items() if k != "all_ms"}), flush=True)
        res[shape] = row
        for b in (dtab, ws):
            b.free()
    # the check alone, at config4's 100 000 entries: the last entry's device side is host memory, so the call is refused with every
    # lookup made and nothing queued
    check = {}
    if "config4" in lay:
        sz, d_at, h_at, offs = lay["config4"]
        for name, shrink in (("touching", 0), ("apart", 1)):
            t = M.table(sz.size)
            t["dst"], t["src"], t["n"], t["stream_off"], t["key"] = dev.ptr + d_at, host.ctypes.data + h_at, np.maximum(sz - shrink, 0), offs, M.as_int32(KEY)
            t["dst"][-1], t["n"][-1] = host_out.ctypes.data, 16
            ms = []
            for _ in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                rc = lib.modgpu_cycle_host_to_device_list(vp(t.ctypes.data), t.size, -1)
                ms.append((time.perf_counter() - t0) * 1e3)
                assert rc == 1 and lib.modgpu_last_error().decode().startswith("entry %d:" % (t.size - 1))
            check[name] = {"median_ms": round(statistics.median(ms[a.warmup:]), 4), "all_ms": [round(x, 4) for x in ms[a.warmup:]],
                           "non_empty_entries": int((t["n"] > 0).sum())}
        print("check", json.dumps(check), flush=True)
    doc = C.profile_head("bench_xfer_list.py", "ms per synchronous call on the wall clock, median of --steps; pageable host memory", a)
    doc.update({"shapes": res, "check_100000_entries": check, "xfer_kernel_source_hash": M.xfer_kernel_source_hash(),
                "table_kernel_source_hash": M.table_kernel_source_hash()})
    C.write_profile(a.out, doc)
    print(json.dumps({"tool": "tools/bench_xfer_list.py", "shapes": {s: {d: {k: r[d][k] for k in ("list_over_loop", "list_over_single", "single_aa_spread", "list_GBps")}
                                                                      for d in ("upload", "download")} for s, r in res.items()}, "check": check}))


if __name__ == "__main__":
    main()
