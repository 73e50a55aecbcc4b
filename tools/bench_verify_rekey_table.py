#!/usr/bin/env python3
"""The rekey verify table call (modgpu_verify_rekey_table_device: a device-resident table of rekey entries verified in three launches)
against what a caller had before and against its single-keystream twin.  One process, one stream, HIP events recorded on that stream
around every single pass; the variants alternate step by step so drift hits all of them alike; every comparator is also run a second
time under another name in the same rotation, and the spread of the two medians (A/A) is recorded.  Rate unit: 2n algorithmic bytes per
pass (n of the comparand read + n of the source read), as in DESIGN.md 4.10.  The comparand is made on the device by
modgpu_rekey_table_device over the same table (PS3 at off_from -> PS4 at off_to: two genuinely different streams), so a pass is clean.

    shapes     4g           1 x 4 GiB clean, source and comparand co-aligned
               4g_p5        the same with the source at phase 5 (the funnel read)
               16x256m      16 x 256 MiB, co-aligned
               16kx64k      16 384 x 64 KiB, random source and comparand phases
               config4      100 000 entries of [0, 64 KiB] (seeded), packed as in a part
               config4dirty config4 verified under the WRONG key_to: every byte a mismatch (report only; against the clean run)
               4gdirty      4g under the wrong key_to (report only)
               64k 1m 16m   single entries (report only; against modgpu_verify_rekey_device)
    variants   new, new2    the call at its shipped grid, twice (its A/A)
               batch,batch2 modgpu_verify_rekey_batch_device on the same buffers, its argument arrays built once outside the timed
                            region (1 + ceil(n/16) launches): the structural comparator of 16kx64k and config4, run for 16x256m too
               one, one2    modgpu_verify_rekey_device on the same buffers (single entries)
               vt, vt2      modgpu_verify_table_device, the single-keystream twin, over the same SOURCE and the same layout; its
                            comparand is a second buffer of the same size made by modgpu_cycle_table_device under PS3 (the rekeyed
                            comparand would be dirty in every byte under one key, and a dirty pass is another code path): the
                            large-entry comparator.  Both calls read 2n bytes through the same descriptors' shapes.

    python tools/bench_verify_rekey_table.py [--shapes ...] [--warmup 3] [--steps 20] [--out profiles/r14_verify_rekey_table.json]
"""
import ctypes

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY_FROM, KEY_TO, WRONG_KEY = M.KEY_PS3, M.KEY_PS4, 12345
ALL_SHAPES = "4g,4g_p5,16x256m,16kx64k,config4,config4dirty,4gdirty,64k,1m,16m"
STRUCTURAL, LARGE, DIRTY, SINGLE = ("16kx64k", "config4"), ("4g", "4g_p5", "16x256m"), ("config4dirty", "4gdirty"), ("64k", "1m", "16m")
_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


def variants_of(shape):
    if shape in STRUCTURAL:
        return ["new", "new2", "batch", "batch2"]
    if shape == "16x256m":
        return ["new", "new2", "vt", "vt2", "batch", "batch2"]
    if shape in LARGE:
        return ["new", "new2", "vt", "vt2", "one", "one2"]
    if shape in DIRTY:
        return ["new", "new2", "clean", "clean2"]
    return ["new", "new2", "one", "one2"]


def main():
    a = H.arguments("r14_verify_rekey_table.json", shapes=ALL_SHAPES).parse_args()
    assert a.warmup >= 1 and a.steps >= 1
    L = M.lib()
    st = Stream()
    rows = {}
    shipped = None
    kf, kt = M.as_int32(KEY_FROM), M.as_int32(KEY_TO)
    for shape in a.shapes.split(","):
        sz, so, eo, of, ot, sn, en = H.table_layout("verify_rekey_table", shape)
        variants = variants_of(shape)
        dirty = shape in DIRTY
        n_bytes, k = int(sz.sum()), sz.size
        sbuf, ebuf = M.DeviceBuffer(sn), M.DeviceBuffer(en)
        H.fill(sbuf, sn)
        t = M.rekey_table(k)
        t["dst"], t["src"], t["n"], t["off_from"], t["off_to"] = ebuf.ptr + eo, sbuf.ptr + so, sz, of, ot
        t["key_from"], t["key_to"] = kf, kt
        M.rekey_table_device(t, check=False)  # the comparand: what the rekey writes
        tb = M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        tw = t.copy()
        tw["key_to"] = M.as_int32(WRONG_KEY)
        tbw = M.DeviceBuffer(tw.nbytes)
        tbw.upload(tw.view(np.uint8))
        ws = M.DeviceBuffer(M.verify_rekey_table_workspace_bytes(k))
        res = M.DeviceBuffer(32 * k)
        own = [sbuf, ebuf, tb, tbw, ws, res]
        if "vt" in variants:  # the twin: the same source and layout, a comparand of its own under one key
            e1buf = M.DeviceBuffer(en)
            t1 = M.table(k)
            t1["dst"], t1["src"], t1["n"], t1["stream_off"], t1["key"] = e1buf.ptr + eo, sbuf.ptr + so, sz, of, kf
            M.cycle_table_device(t1)
            tb1 = M.DeviceBuffer(t1.nbytes)
            tb1.upload(t1.view(np.uint8))
            ws1 = M.DeviceBuffer(M.verify_table_workspace_bytes(k))
            own += [e1buf, tb1, ws1]
        if "batch" in variants:
            ce = (_vp * k)(*[int(x) for x in t["dst"]])
            cs = (_vp * k)(*[int(x) for x in t["src"]])
            cz = (_u64 * k)(*[int(x) for x in sz])
            cf = (_u64 * k)(*[int(x) for x in of])
            ct = (_u64 * k)(*[int(x) for x in ot])
        stv = _vp(st.handle)

        def one_pass(v):
            v = v.rstrip("2")
            if v == "new":
                M.verify_rekey_table_device(tbw if dirty else tb, res, ws, n=k, stream=st.handle)
            elif v == "clean":
                M.verify_rekey_table_device(tb, res, ws, n=k, stream=st.handle)
            elif v == "vt":
                M.verify_table_device(tb1, res, ws1, n=k, stream=st.handle)
            elif v == "one":
                M.verify_rekey_device(int(t["dst"][0]), int(t["src"][0]), KEY_FROM, KEY_TO, int(of[0]), int(ot[0]), result=res, stream=st.handle, n=n_bytes)
            else:
                if L.modgpu_verify_rekey_batch_device(ce, cs, cz, cf, ct, k, kf, kt, _vp(res.ptr), -1, stv):
                    raise RuntimeError(L.modgpu_last_error().decode())
            return M.last_launch()

        summaries = {}

        def checked(v, info):
            nonlocal shipped
            if info["variant"] in (11, 13):
                w = ws if info["variant"] == 13 else ws1
                assert M.table_status(w) is None
                summaries[v] = M.verify_table_summary(w)
                assert (summaries[v]["mismatches"] == 0) == (not (dirty and v.startswith("new"))), (shape, v, summaries[v])
                if info["variant"] == 13:
                    shipped = info["grid"]
            else:
                assert int(M.verify_results(res, k)["mismatches"].sum()) == 0, (shape, v)

        times, info, launches = H.measure(st, variants, one_pass, a.warmup, a.steps, after_warmup=checked)
        row = {"entries": int(k), "bytes": n_bytes, "launch": {v: H.launch_row(info[v], launches[v]) for v in variants}, "summary": summaries}
        for v in variants:
            row[v] = H.stats(times[v], n_bytes, 2, "TBps_2n")
        for v in variants:
            if not v.endswith("2"):
                row[v + "_aa_spread"] = H.aa_spread(row, v)
                if v != "new":
                    row["new_time_over_" + v] = round(row["new"]["median_ms"] / row[v]["median_ms"], 4)
        if shape in STRUCTURAL:
            row["bar"] = {"rule": "batch / new >= 10", "speedup": round(row["batch"]["median_ms"] / row["new"]["median_ms"], 3)}
            row["bar"]["met"] = row["bar"]["speedup"] >= 10
        if shape in LARGE:
            limit = max(1.05, 1 + 2 * row["vt_aa_spread"])
            row["bar"] = {"rule": "new / vt <= max(1.05, 1 + 2 x vt's A/A spread)", "limit": round(limit, 4), "ratio": row["new_time_over_vt"],
                          "met": row["new_time_over_vt"] <= limit}
        rows[shape] = row
        print("%-12s %6d entries  " % (shape, k) + "  ".join("%s %.3f ms %.2f TB/s" % (v, row[v]["median_ms"], row[v]["TBps_2n"]) for v in variants)
              + ("  bar %s" % row["bar"] if "bar" in row else ""), flush=True)
        for b in own:
            b.free()
    st.destroy()
    H.write_profile(a.out, {
        **H.profile_head("bench_verify_rekey_table.py", "TB/s of 2n algorithmic bytes per pass (n of the comparand + n of the source, both read)", a),
        "key_from": KEY_FROM, "key_to": KEY_TO, "wrong_key_to": WRONG_KEY, "shipped_grid": shipped,
        "rekey_verify_table_kernel_source_hash": M.rekey_verify_table_kernel_source_hash(),
        "verify_table_kernel_source_hash": M.verify_table_kernel_source_hash(), "rekey_verify_kernel_source_hash": M.rekey_verify_kernel_source_hash(),
        "kernel_source_hash": M.kernel_source_hash(), "shapes": rows})


if __name__ == "__main__":
    main()
