#!/usr/bin/env python3
"""The table call (modgpu_cycle_table_device: a device-resident table of out-of-place entries in three launches) against what a caller
had before: modgpu_cycle_device_to for one buffer, modgpu_cycle_batch_device_to (16 entries per launch) for many.  One process, one
stream, HIP events recorded on that stream around every single pass; the variants alternate step by step so drift hits all of them
alike.  Rate unit: 2n algorithmic bytes per pass (n read + n written), as in DESIGN.md 5.

    shapes     4g         1 x 4 GiB, source and destination co-aligned (phase 0)           against modgpu_cycle_device_to
               16x256m    16 x 256 MiB, co-aligned                                          against modgpu_cycle_batch_device_to
               16kx64k    16 384 x 64 KiB, random source and destination phases            against the batch call (1 024 launches)
               config4    100 000 entries of [0, 64 KiB] (seeded), packed as in a part,    against the batch call (6 250 launches)
                          extracted to a second buffer of the same layout, stream_off = the entry's offset in the part
    variants   table      the shipped call (table and workspace resident)
               table_all  the same with one stream workgroup per CU (testing flavour: modgpu_debug_set_table_grid)
               base       the existing call named above (its argument arrays built once, outside the timed region); the batch call is
                          made per 16 entries -- what a launch takes anyway -- since its overlap check is quadratic in its entry count

    python tools/bench_table.py [--shapes 4g,16x256m,16kx64k,config4] [--warmup 3] [--steps 20] [--out profiles/r09_table.json]
"""
import ctypes

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY = M.KEY_PS4
VARIANTS = ("table", "table_all", "base")
_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


def main():
    a = H.arguments("r09_table.json", shapes="4g,16x256m,16kx64k,config4", variants=",".join(VARIANTS)).parse_args()
    variants = a.variants.split(",")
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    L = M.lib()
    st = Stream()
    rows = {}
    for shape in a.shapes.split(","):
        sz, so, do, offs, sn, dn = H.table_layout("table", shape)
        n_bytes = int(sz.sum())
        sbuf, dbuf = M.DeviceBuffer(sn), M.DeviceBuffer(dn)
        H.fill(sbuf, sn)
        t = M.table(sz.size)
        t["dst"] = dbuf.ptr + do
        t["src"] = sbuf.ptr + so
        t["n"] = sz
        t["stream_off"] = offs
        t["key"] = M.as_int32(KEY)
        M.table_validate(t)
        tb = M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        ws = M.DeviceBuffer(M.table_workspace_bytes(sz.size))
        k = sz.size
        cd = (_vp * k)(*[int(x) for x in t["dst"]])
        cs = (_vp * k)(*[int(x) for x in t["src"]])
        cz = (_u64 * k)(*[int(x) for x in sz])
        co = (_u64 * k)(*[int(x) for x in offs])
        P = ctypes.POINTER
        groups = [(ctypes.cast(ctypes.addressof(cd) + 8 * i, P(_vp)), ctypes.cast(ctypes.addressof(cs) + 8 * i, P(_vp)),
                   ctypes.cast(ctypes.addressof(cz) + 8 * i, P(_u64)), ctypes.cast(ctypes.addressof(co) + 8 * i, P(_u64)), min(16, k - i))
                  for i in range(0, k, 16)]
        key32, stv = M.as_int32(KEY), _vp(st.handle)
        batch = L.modgpu_cycle_batch_device_to

        def one_pass(v):
            if v in ("table", "table_all"):
                M.debug_set_table_grid(256 if v == "table_all" else 0)
                M.cycle_table_device(tb, ws, n=k, stream=st.handle)
            elif shape == "4g":
                M.cycle_device_to(int(t["dst"][0]), int(t["src"][0]), n_bytes, KEY, 0, stream=st.handle)
            else:
                for gd, gs, gz, go, gn in groups:
                    if batch(gd, gs, gz, go, gn, key32, -1, stv):
                        raise RuntimeError(M.lib().modgpu_last_error().decode())
            return M.last_launch()

        def checked(v, info):
            assert M.table_status(ws) is None

        times, info, launches = H.measure(st, variants, one_pass, a.warmup, a.steps, after_warmup=checked)
        M.debug_set_table_grid(0)
        row = {"entries": int(k), "bytes": n_bytes, "launch": {v: H.launch_row(info[v], launches[v]) for v in variants}}
        for v in variants:
            row[v] = H.stats(times[v], n_bytes, 2, "TBps_2n")
        H.add_speedups(row, variants)
        rows[shape] = row
        print("%-8s %6d entries  " % (shape, k) + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps_2n"]) for v in variants),
              flush=True)
        for b in (sbuf, dbuf, tb, ws):
            b.free()
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_table.py", "TB/s of 2n algorithmic bytes per pass (n read + n written)", a), "key": KEY,
                            "table_kernel_source_hash": M.table_kernel_source_hash(), "to_kernel_source_hash": M.to_kernel_source_hash(),
                            "kernel_source_hash": M.kernel_source_hash(), "shapes": rows})


if __name__ == "__main__":
    main()
