#!/usr/bin/env python3
"""The digest table call (modgpu_digest_table_device: a device-resident table of entries in three launches, one 32-byte record each)
against what a caller had before: modgpu_digest_device (digest only) for one buffer, modgpu_digest_batch_device (16 entries per launch,
one key per call, a memset node in front) for many.  One process, one stream, HIP events recorded on that stream around every single
pass; the variants alternate step by step so drift hits all of them alike.  Rate unit: n bytes read per pass.  Before anything is
timed every value of the table call is compared -- with zlib.adler32 of the host's own cycle of the source where the shape is small
(up to 16 MiB), with the existing call's values otherwise.

    shapes     64k, 1m, 16m 1 entry, launch-bound sizes                                            against modgpu_digest_device
               4g           1 x 4 GiB, the source chunk-aligned                                    against modgpu_digest_device
               4g_p5        the same with the source at phase 5                                    against modgpu_digest_device
               16kx64k      16 384 x 64 KiB at random source phases                                against the batch call (1 024 launches)
               config4      100 000 entries of [0, 64 KiB] (seeded), packed as in a part            against the batch call (6 250 launches)
    variants   table        the call at its shipped grid (one workgroup per CU)
               grid200      the same on 200 workgroups (testing flavour: modgpu_debug_set_digest_table_grid)
               base         the existing call named above (its argument arrays built once, outside the timed region)

    python tools/bench_digest_table.py [--shapes 64k,1m,16m,4g,4g_p5,16kx64k,config4] [--warmup 3] [--steps 20] [--out profiles/r17_digest_table.json]
"""
import ctypes
import zlib

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY = M.KEY_PS3
VARIANTS = ("table", "grid200", "base")
GRIDS = {"table": 0, "grid200": 200}
_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


def main():
    a = H.arguments("r17_digest_table.json", shapes="64k,1m,16m,4g,4g_p5,16kx64k,config4", variants=",".join(VARIANTS)).parse_args()
    variants = a.variants.split(",")
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    M.debug_set_digest_table_grid(0)
    L = M.lib()
    st = Stream()
    rows = {}
    shipped = None
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
        res, res_base = M.DeviceBuffer(32 * k), M.DeviceBuffer(32 * k)
        cs = (_vp * k)(*[int(x) for x in t["src"]])
        cz = (_u64 * k)(*[int(x) for x in sz])
        co = (_u64 * k)(*[int(x) for x in offs])
        key32, stv = M.as_int32(KEY), _vp(st.handle)
        batch = L.modgpu_digest_batch_device

        def one_pass(v):
            if v in GRIDS:
                M.debug_set_digest_table_grid(GRIDS[v])
                M.digest_table_device(tb, res, ws, n=k, stream=st.handle)
            elif k == 1:
                M.digest_device(int(t["src"][0]), KEY, int(offs[0]), None, res_base, -1, st.handle, n=n_bytes)
            elif batch(None, cs, cz, co, k, key32, _vp(res_base.ptr), -1, stv):
                raise RuntimeError(L.modgpu_last_error().decode())
            return M.last_launch()

        # every value, before anything is timed
        def checked(v, info):
            nonlocal shipped
            if v in GRIDS:
                assert M.table_status(ws) is None and info["variant"] == 17, (shape, v, info)
                if v == "table" and shipped is None:
                    shipped = info["grid"]
                got = M.digest_results(res, k)[1]
                if n_bytes <= 16 << 20:
                    for i in range(k):  # the route a caller had: the out-of-place call into scratch, a download, zlib
                        scratch = M.DeviceBuffer(int(sz[i]) + 64)
                        M.cycle_device_to(scratch.ptr, int(t["src"][i]), int(sz[i]), KEY, int(offs[i]))
                        scratch.sync()
                        assert int(got[i]) == zlib.adler32(scratch.download(int(sz[i])).tobytes()) & 0xFFFFFFFF, (shape, v, i)
                        scratch.free()
                else:
                    one_pass("base")
                    st.sync()
                    assert np.array_equal(got, M.digest_results(res_base, k)[1]), (shape, v, "the table call and the existing call disagree")

        times, info, launches = H.measure(st, variants, one_pass, a.warmup, a.steps, after_warmup=checked)
        M.debug_set_digest_table_grid(0)
        row = {"entries": int(k), "bytes": n_bytes, "launch": {v: H.launch_row(info[v], launches[v]) for v in variants}}
        for v in variants:
            row[v] = H.stats(times[v], n_bytes, 1, "TBps")
        H.add_speedups(row, variants)
        rows[shape] = row
        print("%-8s %6d entries  " % (shape, k) + "  ".join("%s %.4f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps"]) for v in variants), flush=True)
        for b in (sbuf, tb, ws, res, res_base):
            b.free()
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_digest_table.py", "TB/s of n bytes read per pass", a), "key": KEY, "shipped_grid": shipped,
                            "verify_table_kernel_source_hash": M.verify_table_kernel_source_hash(),
                            "to_kernel_source_hash": M.to_kernel_source_hash(), "shapes": rows})


if __name__ == "__main__":
    main()
