#!/usr/bin/env python3
"""The verify table call (modgpu_verify_table_device: a device-resident table of verify entries in three launches) at two stream grids
against what a caller had before: modgpu_verify_device for one buffer, modgpu_verify_batch_device (16 entries per compare launch) for
many.  One process, one stream, HIP events recorded on that stream around every single pass; the variants alternate step by step so
drift hits all of them alike.  Rate unit: 2n algorithmic bytes per pass (n of the comparand read + n of the source read), as in
DESIGN.md 4.10.  The comparand is made on the device by modgpu_cycle_table_device over the same table, so a pass under the same key
is clean.

    shapes     4g           1 x 4 GiB clean, source and comparand co-aligned                      against modgpu_verify_device
               4g_p5        the same with the source at phase 5 (the funnel read)                  against modgpu_verify_device
               16x256m      16 x 256 MiB, co-aligned                                               against modgpu_verify_batch_device
               16kx64k      16 384 x 64 KiB, random source and comparand phases                    against the batch call (1 + 1 024 launches)
               config4      100 000 entries of [0, 64 KiB] (seeded), packed as in a part            against the batch call (1 + 6 250 launches)
               config4dirty config4 compared under the WRONG key: every byte a mismatch, every wave of every chunk in the slow
                            path and every chunk a flush -- against the call's own clean run (`base` = the shipped grid, right key)
    variants   grid256      the call with one stream workgroup per CU on all 256 CUs (testing flavour: modgpu_debug_set_verify_table_grid)
               grid200      the same with the table call's 25 per 32 CUs (200)
               base         the existing call named above (its argument arrays built once, outside the timed region)

    python tools/bench_verify_table.py [--shapes 4g,4g_p5,16x256m,16kx64k,config4,config4dirty] [--warmup 3] [--steps 20] [--out profiles/r12_verify_table.json]
"""
import ctypes

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY, WRONG_KEY = M.KEY_PS3, M.KEY_PS4
VARIANTS = ("grid256", "grid200", "base")
GRIDS = {"grid256": 256, "grid200": 200}
_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


def main():
    a = H.arguments("r12_verify_table.json", shapes="4g,4g_p5,16x256m,16kx64k,config4,config4dirty", variants=",".join(VARIANTS)).parse_args()
    variants = a.variants.split(",")
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    M.debug_set_verify_table_grid(0)
    shipped = None
    L = M.lib()
    st = Stream()
    rows = {}
    for shape in a.shapes.split(","):
        sz, so, eo, offs, sn, en = H.table_layout("verify_table", shape)
        dirty = shape == "config4dirty"
        n_bytes = int(sz.sum())
        k = sz.size
        sbuf, ebuf = M.DeviceBuffer(sn), M.DeviceBuffer(en)
        H.fill(sbuf, sn)
        t = M.table(k)
        t["dst"] = ebuf.ptr + eo
        t["src"] = sbuf.ptr + so
        t["n"] = sz
        t["stream_off"] = offs
        t["key"] = M.as_int32(KEY)
        M.cycle_table_device(t)  # the comparand: what the cipher writes
        tb = M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        tw = t.copy()
        tw["key"] = M.as_int32(WRONG_KEY)
        tbw = M.DeviceBuffer(tw.nbytes)
        tbw.upload(tw.view(np.uint8))
        ws = M.DeviceBuffer(M.verify_table_workspace_bytes(k))
        res = M.DeviceBuffer(32 * k)
        if shipped is None:
            M.verify_table_device(tb, res, ws, n=k, stream=st.handle)
            shipped = M.last_launch()["grid"]
        ce = (_vp * k)(*[int(x) for x in t["dst"]])
        cs = (_vp * k)(*[int(x) for x in t["src"]])
        cz = (_u64 * k)(*[int(x) for x in sz])
        co = (_u64 * k)(*[int(x) for x in offs])
        key32, stv = M.as_int32(KEY), _vp(st.handle)
        batch = L.modgpu_verify_batch_device

        def one_pass(v):
            if v in GRIDS:
                M.debug_set_verify_table_grid(GRIDS[v])
                M.verify_table_device(tbw if dirty else tb, res, ws, n=k, stream=st.handle)
            elif dirty:
                M.debug_set_verify_table_grid(0)
                M.verify_table_device(tb, res, ws, n=k, stream=st.handle)
            elif k == 1:
                M.verify_device(int(t["dst"][0]), int(t["src"][0]), KEY, 0, result=res, stream=st.handle, n=n_bytes)
            else:
                if batch(ce, cs, cz, co, k, key32, _vp(res.ptr), -1, stv):
                    raise RuntimeError(M.lib().modgpu_last_error().decode())
            return M.last_launch()

        summaries = {}

        def checked(v, info):
            if info["variant"] == 11:
                assert M.table_status(ws) is None
                summaries[v] = M.verify_table_summary(ws)
                assert (summaries[v]["mismatches"] == 0) == (not (dirty and v in GRIDS)), (shape, v, summaries[v])
            else:
                assert int(M.verify_results(res, k)["mismatches"].sum()) == 0, (shape, v)

        times, info, launches = H.measure(st, variants, one_pass, a.warmup, a.steps, after_warmup=checked)
        M.debug_set_verify_table_grid(0)
        row = {"entries": int(k), "bytes": n_bytes, "launch": {v: H.launch_row(info[v], launches[v]) for v in variants}, "summary": summaries}
        for v in variants:
            row[v] = H.stats(times[v], n_bytes, 2, "TBps_2n")
        H.add_speedups(row, variants)
        rows[shape] = row
        print("%-12s %6d entries  " % (shape, k) + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps_2n"]) for v in variants),
              flush=True)
        for b in (sbuf, ebuf, tb, tbw, ws, res):
            b.free()
    st.destroy()
    H.write_profile(a.out, {
        **H.profile_head("bench_verify_table.py", "TB/s of 2n algorithmic bytes per pass (n of the comparand + n of the source, both read)", a),
        "key": KEY, "wrong_key": WRONG_KEY, "shipped_grid": shipped, "verify_table_kernel_source_hash": M.verify_table_kernel_source_hash(),
        "verify_kernel_source_hash": M.verify_kernel_source_hash(), "kernel_source_hash": M.kernel_source_hash(), "shapes": rows})


if __name__ == "__main__":
    main()
