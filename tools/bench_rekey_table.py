#!/usr/bin/env python3
"""The rekey table call (modgpu_rekey_table_device: a device-resident table of rekey entries in three launches) at both stream grids
against what a caller had before: modgpu_rekey_device_to for one buffer, modgpu_rekey_batch_device_to (16 entries per launch) for many.
One process, one stream, HIP events recorded on that stream around every single pass; the variants alternate step by step so drift hits
all of them alike.  Rate unit: 2n algorithmic bytes per pass (n read + n written), as in DESIGN.md 5.  Every entry goes PS3 -> PS4.

    shapes     4g         1 x 4 GiB, source and destination co-aligned (phase 0), both offsets 0   against modgpu_rekey_device_to
               16x256m    16 x 256 MiB, co-aligned                                             against modgpu_rekey_batch_device_to
               16kx64k    16 384 x 64 KiB, random source and destination phases, offsets = their places in a part  against the batch
                          call (1 024 launches)
               config4    100 000 entries of [0, 64 KiB] (seeded), packed as in a part, relocated into a second part in which every
                          entry moved by a random amount (a file inserted, files resized): off_from = the old offset, off_to = the new
                          one -- against the batch call (6 250 launches)
    variants   grid256    the call with one stream workgroup per CU on all 256 CUs (testing flavour: modgpu_debug_set_rekey_table_grid)
               grid200    the same with the table call's 25 per 32 CUs (200)
               base       the existing call named above (its argument arrays built once, outside the timed region); the batch call is
                          made per 16 entries -- what a launch takes anyway -- since its overlap check is quadratic in its entry count

    python tools/bench_rekey_table.py [--shapes 4g,16x256m,16kx64k,config4] [--warmup 3] [--steps 20] [--out profiles/r10_rekey_table.json]
"""
import ctypes

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY_FROM, KEY_TO = M.KEY_PS3, M.KEY_PS4
VARIANTS = ("grid256", "grid200", "base")
GRIDS = {"grid256": 256, "grid200": 200}
_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


def main():
    a = H.arguments("r10_rekey_table.json", shapes="4g,16x256m,16kx64k,config4", variants=",".join(VARIANTS)).parse_args()
    variants = a.variants.split(",")
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    M.debug_set_rekey_table_grid(0)
    shipped = None
    L = M.lib()
    st = Stream()
    rows = {}
    for shape in a.shapes.split(","):
        sz, so, do, ofr, oto, sn, dn = H.table_layout("rekey_table", shape)
        n_bytes = int(sz.sum())
        sbuf, dbuf = M.DeviceBuffer(sn), M.DeviceBuffer(dn)
        H.fill(sbuf, sn)
        t = M.rekey_table(sz.size)
        t["dst"] = dbuf.ptr + do
        t["src"] = sbuf.ptr + so
        t["n"] = sz
        t["off_from"] = ofr
        t["off_to"] = oto
        t["key_from"] = M.as_int32(KEY_FROM)
        t["key_to"] = M.as_int32(KEY_TO)
        M.rekey_table_validate(t)
        tb = M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        ws = M.DeviceBuffer(M.rekey_table_workspace_bytes(sz.size))
        if shipped is None:
            M.rekey_table_device(tb, ws, n=sz.size, stream=st.handle)
            shipped = M.last_launch()["grid"]
        k = sz.size
        cd = (_vp * k)(*[int(x) for x in t["dst"]])
        cs = (_vp * k)(*[int(x) for x in t["src"]])
        cz = (_u64 * k)(*[int(x) for x in sz])
        cf = (_u64 * k)(*[int(x) for x in ofr])
        ct = (_u64 * k)(*[int(x) for x in oto])
        P = ctypes.POINTER
        groups = [(ctypes.cast(ctypes.addressof(cd) + 8 * i, P(_vp)), ctypes.cast(ctypes.addressof(cs) + 8 * i, P(_vp)),
                   ctypes.cast(ctypes.addressof(cz) + 8 * i, P(_u64)), ctypes.cast(ctypes.addressof(cf) + 8 * i, P(_u64)),
                   ctypes.cast(ctypes.addressof(ct) + 8 * i, P(_u64)), min(16, k - i))
                  for i in range(0, k, 16)]
        kf32, kt32, stv = M.as_int32(KEY_FROM), M.as_int32(KEY_TO), _vp(st.handle)
        batch = L.modgpu_rekey_batch_device_to

        def one_pass(v):
            if v in GRIDS:
                M.debug_set_rekey_table_grid(GRIDS[v])
                M.rekey_table_device(tb, ws, n=k, stream=st.handle)
            elif shape == "4g":
                M.rekey_device_to(int(t["dst"][0]), int(t["src"][0]), KEY_FROM, KEY_TO, 0, 0, stream=st.handle, n=n_bytes)
            else:
                for gd, gs, gz, gf, gt, gn in groups:
                    if batch(gd, gs, gz, gf, gt, gn, kf32, kt32, -1, stv):
                        raise RuntimeError(M.lib().modgpu_last_error().decode())
            return M.last_launch()

        def checked(v, info):
            assert M.table_status(ws) is None

        times, info, launches = H.measure(st, variants, one_pass, a.warmup, a.steps, after_warmup=checked)
        M.debug_set_rekey_table_grid(0)
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
    H.write_profile(a.out, {**H.profile_head("bench_rekey_table.py", "TB/s of 2n algorithmic bytes per pass (n read + n written)", a),
                            "key_from": KEY_FROM, "key_to": KEY_TO, "shipped_grid": shipped,
                            "rekey_table_kernel_source_hash": M.rekey_table_kernel_source_hash(),
                            "rekey_kernel_source_hash": M.rekey_kernel_source_hash(), "kernel_source_hash": M.kernel_source_hash(), "shapes": rows})


if __name__ == "__main__":
    main()
