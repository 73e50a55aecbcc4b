#!/usr/bin/env python3
"""The transfer calls (modgpu_cycle_host_to_device & co.) against what a caller had to do before and against the link's one-way
ceilings.  One process; every call is synchronous, so each is timed on the wall clock around the call; the variants alternate step by
step so drift hits all of them alike.  Rate unit: GB/s of payload (n bytes per call, one direction of the link).

    upload     up_pageable    modgpu_cycle_host_to_device from pageable memory (the transfer kernel, slots + pipelines)
               up_pinned      the same from page-locked memory (the kernel reads the caller's pages across PCIe)
               up_file        modgpu_cycle_file_to_device from a part file in the page cache
               up_dma         up_pageable in the DMA reference form (testing flavour: H2D into a device slot + cycle_to, per chunk)
               ref_h2d_cycle  modgpu_h2d (pageable) + modgpu_cycle_device + sync: the two steps it replaces
               h2d_only       modgpu_h2d from pageable memory alone (a synchronous hipMemcpy)
    download   down_pageable  modgpu_cycle_device_to_host into pageable memory
               down_pinned    the same into page-locked memory
               down_file      modgpu_cycle_device_to_file (a part file, written and not synced)
               down_dma       down_pageable in the DMA reference form (cycle_to into a device slot + D2H, per chunk)
               ref_to_d2h     modgpu_cycle_device_to into a second device buffer + modgpu_d2h (pageable)
    ceilings   tools/ubench_pcie_ceiling 1024 5, run first in a child process: dma_h2d, dma_d2h, kernel_read_only, kernel_write_only

    python tools/bench_xfer.py [--sizes-mib 16,64,256,1024,4096] [--warmup 1] [--steps 5] [--out profiles/r07_xfer.json]
    python tools/bench_xfer.py --trace-once 1024     one upload and one download of 1024 MiB from pageable memory (for rocprofv3)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["MODGPU_REQUIRE_GPU"] = "1"
import numpy as np  # noqa: E402

KEY = 0x90CFC0AB
UP = ("up_pageable", "up_pinned", "up_file", "up_dma", "ref_h2d_cycle", "h2d_only")
DOWN = ("down_pageable", "down_pinned", "down_file", "down_dma", "ref_to_d2h")


def ceilings():
    exe = os.path.join(ROOT, "tools", "ubench_pcie_ceiling")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools"), "ubench_pcie_ceiling"])
    r = subprocess.run([exe, "1024", "5"], capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CEILING ")]
    if r.returncode != 0 or not line:
        raise SystemExit("ubench_pcie_ceiling failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    c = json.loads(line[0][len("CEILING "):])
    return {"dma_h2d": c["dma_h2d"], "dma_d2h": c["dma_d2h"], "kernel_read_only": c["kernel_read_only_grid32"],
            "kernel_write_only": c["kernel_write_only_grid32"], "raw": c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", default="16,64,256,1024,4096")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_xfer.json"))
    ap.add_argument("--trace-once", type=int, default=0, help="MiB: one upload + one download from pageable memory, nothing else")
    args = ap.parse_args()

    ceil = None if args.trace_once else ceilings()  # (a child with the GPU to itself, before this process opens it)
    import modulate_amd as M
    M.use_testing_flavour()  # (the DMA reference form is a testing-flavour switch; the routes' defaults are the shipped ones)

    if args.trace_once:
        n = args.trace_once << 20
        host = np.frombuffer(np.random.default_rng(1).bytes(n), np.uint8)
        dev = M.DeviceBuffer(n)
        out = np.empty(n, np.uint8)
        M.cycle_host_to_device(dev.ptr, host, KEY)
        M.cycle_device_to_host(out, dev.ptr, KEY)
        assert np.array_equal(out, host)
        print("TRACE_ONCE_OK", M.last_launch()["kernel"], M.path_stats()["gpu_launches"])
        return

    sizes = [int(s) << 20 for s in args.sizes_mib.split(",")]
    big = max(sizes)
    rng = np.random.default_rng(7)
    block = np.frombuffer(rng.bytes(64 << 20), np.uint8)
    host = np.tile(block, max(1, big // block.size))[:big].copy()
    host_out = np.empty(big, np.uint8)
    pin_in, pin_out = M.PinnedBuffer(big), M.PinnedBuffer(big)
    pin_in.array[:] = host
    assert pin_in.pinned and pin_out.pinned
    dev, dev2 = M.DeviceBuffer(big), M.DeviceBuffer(big)
    tmp = tempfile.mkdtemp(prefix="bench_xfer_")
    part, outf = os.path.join(tmp, "part.bin"), os.path.join(tmp, "out.bin")
    host.tofile(part)
    with open(part, "rb") as f:  # (into the page cache)
        while f.read(256 << 20):
            pass
    lib = M.lib()

    def run(v, n):
        M.debug_set_xfer_form("dma" if v in ("up_dma", "down_dma") else None)
        t0 = time.perf_counter()
        if v in ("up_pageable", "up_dma"):
            M.cycle_host_to_device(dev.ptr, host[:n], KEY)
        elif v == "up_pinned":
            M.cycle_host_to_device(dev.ptr, pin_in.array[:n], KEY)
        elif v == "up_file":
            M.cycle_file_to_device(part, dev.ptr, n, KEY)
        elif v == "ref_h2d_cycle":
            M.capi._check(lib.modgpu_h2d(M.capi._vp(dev.ptr), M.capi._vp(host.ctypes.data), n, -1))
            M.cycle_device(dev.ptr, n, KEY)
            dev.sync()
        elif v == "h2d_only":
            M.capi._check(lib.modgpu_h2d(M.capi._vp(dev.ptr), M.capi._vp(host.ctypes.data), n, -1))
        elif v in ("down_pageable", "down_dma"):
            M.cycle_device_to_host(host_out[:n], dev.ptr, KEY)
        elif v == "down_pinned":
            M.cycle_device_to_host(pin_out.array[:n], dev.ptr, KEY)
        elif v == "down_file":
            M.cycle_device_to_file(dev.ptr, n, outf, KEY)
        elif v == "ref_to_d2h":
            M.cycle_device_to(dev2.ptr, dev.ptr, n, KEY)
            dev2.sync()
            M.capi._check(lib.modgpu_d2h(M.capi._vp(host_out.ctypes.data), M.capi._vp(dev2.ptr), n, -1))
        dt = time.perf_counter() - t0
        M.debug_set_xfer_form(None)
        return n / dt / 1e9

    # correctness of what is timed: one upload and one download at the largest size against the two-step reference
    M.cycle_host_to_device(dev.ptr, host, KEY)
    ref = dev.download()
    M.capi._check(lib.modgpu_h2d(M.capi._vp(dev2.ptr), M.capi._vp(host.ctypes.data), big, -1))
    M.cycle_device(dev2.ptr, big, KEY)
    dev2.sync()
    assert np.array_equal(ref, dev2.download()), "upload != modgpu_h2d + modgpu_cycle_device"
    M.cycle_device_to_host(host_out, dev.ptr, KEY)
    assert np.array_equal(host_out, host), "download did not undo the upload"
    del ref

    res = {}
    for n in sizes:
        rows = {v: [] for v in UP + DOWN}
        kernels = {}
        for step in range(args.warmup + args.steps):
            for v in UP + DOWN:
                g = run(v, n)
                if step >= args.warmup:
                    rows[v].append(g)
                if v in ("up_pageable", "down_pageable", "up_pinned", "down_pinned"):
                    kernels[v] = M.last_launch()["kernel"]
        med = {v: round(statistics.median(x), 2) for v, x in rows.items()}
        frac = {
            "up_pageable_of_ref_h2d_cycle": round(med["up_pageable"] / med["ref_h2d_cycle"], 3),
            "up_file_of_ref_h2d_cycle": round(med["up_file"] / med["ref_h2d_cycle"], 3),
            "up_pageable_of_dma_h2d": round(med["up_pageable"] / ceil["dma_h2d"], 3),
            "up_pinned_of_kernel_read_only": round(med["up_pinned"] / ceil["kernel_read_only"], 3),
            "up_pageable_of_up_dma": round(med["up_pageable"] / med["up_dma"], 3),
            "down_pageable_of_ref_to_d2h": round(med["down_pageable"] / med["ref_to_d2h"], 3),
            "down_file_of_ref_to_d2h": round(med["down_file"] / med["ref_to_d2h"], 3),
            "down_pageable_of_dma_d2h": round(med["down_pageable"] / ceil["dma_d2h"], 3),
            "down_pinned_of_kernel_write_only": round(med["down_pinned"] / ceil["kernel_write_only"], 3),
            "down_pageable_of_down_dma": round(med["down_pageable"] / med["down_dma"], 3),
        }
        res[str(n >> 20)] = {"GBps_median": med, "GBps_all": {v: [round(x, 2) for x in xs] for v, xs in rows.items()}, "frac_of": frac,
                             "kernels": kernels}
        print(n >> 20, "MiB", json.dumps(med), json.dumps(frac), flush=True)
    out = {"what": "transfer calls with the cipher in flight vs the two-step references and the link's one-way ceilings (GB/s of payload, "
                   "median of --steps wall-clock timed synchronous calls)",
           "tool": "tools/bench_xfer.py", "warmup": args.warmup, "steps": args.steps, "ceilings": ceil,
           "modgpu_h2d_pageable_GBps": {k: v["GBps_median"]["h2d_only"] for k, v in res.items()},
           "sizes_mib": res, "xfer_kernel_source_hash": M.xfer_kernel_source_hash(), "kernel_source_hash": M.kernel_source_hash(),
           "to_kernel_source_hash": M.to_kernel_source_hash()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    for p in (part, outf):
        if os.path.exists(p):
            os.unlink(p)
    os.rmdir(tmp)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
