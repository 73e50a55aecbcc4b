#!/usr/bin/env python3
"""The cycle digest table call (modgpu_cycle_digest_table_device: modgpu_cycle_table_device and one digest record per entry in one pass
and three launches) against what a caller had before: modgpu_cycle_table_device followed by modgpu_digest_table_device on the same table
and stream (3n bytes of traffic, six launches).  One process, one stream, HIP events recorded on that stream around every single pass;
the variants alternate step by step so drift hits all of them alike.  Rate unit: n bytes cycled per pass.  Before anything is timed the
fused call's records are compared with modgpu_digest_table_device's (of the same table for the output side, of the table under the
identity key for the input side) and its destination with modgpu_cycle_table_device's, byte for byte.

    shapes     64k, 1m, 16m 1 entry, launch-bound sizes
               4g           1 x 4 GiB, destination and source chunk-aligned
               4g_p5        the same with the source at phase 5
               16kx64k      16 384 x 64 KiB at random phases
               config4      100 000 entries of [0, 64 KiB] (seeded), packed as in a part
    variants   fused_out    the call at its shipped grid, MODGPU_DIGEST_OUTPUT
               fused_in     the same, MODGPU_DIGEST_INPUT
               g200, g256   fused_out on 200 and on 256 stream workgroups (testing flavour: modgpu_debug_set_cycle_digest_table_grid)
               two_a, two_b modgpu_cycle_table_device + modgpu_digest_table_device, twice per step: their difference is the A/A spread
               cycle_a, _b  modgpu_cycle_table_device alone, twice per step
               parent_a, _b modgpu_cycle_table_device of another build's library (--other-lib) loaded into this process, twice per step
               single, single_to   (one entry) modgpu_digest_device with a destination, and modgpu_cycle_device_to: the single call's own fused cost

    python tools/bench_cycle_digest_table.py [--shapes ...] [--warmup 3] [--steps 20] [--other-lib PATH] [--out profiles/r19_cycle_digest_table.json]
"""
import ctypes
import os

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY = M.KEY_PS3
GRIDS = {"fused_out": 0, "fused_in": 0, "g200": 200, "g256": 256}
_vp = ctypes.c_void_p


def main():
    a = H.arguments("r19_cycle_digest_table.json", shapes="64k,1m,16m,4g,4g_p5,16kx64k,config4", other_lib="").parse_args()
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    M.debug_set_cycle_digest_table_grid(0)
    other = None
    if a.other_lib:
        other = H.other_library(os.path.abspath(a.other_lib), ["modgpu_cycle_table_device", "modgpu_table_kernel_source_hash"], M.lib())
    st = Stream()
    rows = {}
    shipped = None
    for shape in a.shapes.split(","):
        sz, do, so, offs, sn = H.table_layout("cycle_digest_table", shape)
        n_bytes, k = int(sz.sum()), sz.size
        sbuf, dbuf = M.DeviceBuffer(sn + 65536 + 16), M.DeviceBuffer(sn + 65536)
        sbase, dbase = -sbuf.ptr % 65536, -dbuf.ptr % 65536  # the layout's offsets count from a chunk edge
        H.fill(sbuf, sn, offset=sbase)
        t = M.table(k)
        t["dst"], t["src"] = dbuf.ptr + dbase + do, sbuf.ptr + sbase + so
        t["n"], t["stream_off"], t["key"] = sz, offs, M.as_int32(KEY)
        tb, tb_plain = M.DeviceBuffer(t.nbytes), M.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        plain = t.copy()
        plain["key"] = 0
        tb_plain.upload(plain.view(np.uint8))
        ws = M.DeviceBuffer(M.cycle_digest_table_workspace_bytes(k))
        res, res_base = M.DeviceBuffer(32 * k), M.DeviceBuffer(32 * k)
        variants = ["fused_out", "fused_in", "two_a", "two_b", "cycle_a", "cycle_b"]
        if shape in ("4g", "4g_p5"):
            variants += ["g200", "g256", "single", "single_to"]
        if other is not None and shape in ("4g", "config4"):
            variants += ["parent_a", "parent_b"]

        def one_pass(v):
            if v in GRIDS:
                M.debug_set_cycle_digest_table_grid(GRIDS[v])
                M.cycle_digest_table_device(tb, res, M.DIGEST_INPUT if v == "fused_in" else M.DIGEST_OUTPUT, ws, n=k, stream=st.handle)
            elif v.startswith("two"):
                M.cycle_table_device(tb, ws, n=k, stream=st.handle)
                M.digest_table_device(tb, res_base, ws, n=k, stream=st.handle)
            elif v.startswith("cycle"):
                M.cycle_table_device(tb, ws, n=k, stream=st.handle)
            elif v.startswith("parent"):
                if other.modgpu_cycle_table_device(_vp(tb.ptr), k, _vp(ws.ptr), ws.nbytes, -1, _vp(st.handle)):
                    raise RuntimeError("the other library refused the table call")
                return {"kernel": "other library", "variant": 8, "grid": 0}
            elif v == "single":
                M.digest_device(int(t["src"][0]), KEY, int(offs[0]), int(t["dst"][0]), res_base, -1, st.handle, n=n_bytes)
            elif v == "single_to":
                M.cycle_device_to(int(t["dst"][0]), int(t["src"][0]), n_bytes, KEY, int(offs[0]), stream=st.handle)
            return M.last_launch()

        # every value, before anything is timed: the two-call route's destination and records are the reference
        one_pass("two_a")
        st.sync()
        want_out = M.digest_results(res_base, k)[1]
        probe = [(0, min(sn, 1 << 22)), (max(0, sn - (1 << 22)), min(sn, 1 << 22))]
        want_img = [dbuf.download(m, offset=dbase + o) for o, m in probe]
        M.digest_table_device(tb_plain, res_base, ws, n=k, stream=st.handle)
        st.sync()
        want_in = M.digest_results(res_base, k)[1]

        def wipe(v):
            if v in GRIDS:
                for o, m in probe:
                    dbuf.upload(np.zeros(m, np.uint8), offset=dbase + o)

        def checked(v, info):
            nonlocal shipped
            if v in GRIDS:
                assert M.table_status(ws) is None and info["variant"] == 18, (shape, v, info)
                if v == "fused_out" and shipped is None:
                    shipped = info["grid"]
                got = M.digest_results(res, k)[1]
                assert np.array_equal(got, want_in if v == "fused_in" else want_out), (shape, v, "the fused call and the digest table call disagree")
                for (o, m), w in zip(probe, want_img):
                    assert np.array_equal(dbuf.download(m, offset=dbase + o), w), (shape, v, "the fused call and the table call wrote different bytes")

        times, info, launches = H.measure(st, variants, one_pass, a.warmup, a.steps, before_warmup=wipe, after_warmup=checked)
        M.debug_set_cycle_digest_table_grid(0)
        row = {"entries": int(k), "bytes": n_bytes, "launch": {v: H.launch_row(info[v], launches[v]) for v in variants}}
        for v in variants:
            row[v] = H.stats(times[v], n_bytes, 1, "TBps")
        med = {v: row[v]["median_ms"] for v in variants}
        two = min(med["two_a"], med["two_b"])
        row["two_call_aa_spread"] = round(H.spread(med["two_a"], med["two_b"]), 5)
        row["cycle_aa_spread"] = round(H.spread(med["cycle_a"], med["cycle_b"]), 5)
        for v in ("fused_out", "fused_in"):
            row["two_call_over_" + v] = round(two / med[v], 4)
            row[v + "_over_cycle"] = round(med[v] / min(med["cycle_a"], med["cycle_b"]), 4)
        if "single" in variants:
            row["single_fused_over_single_to"] = round(med["single"] / med["single_to"], 4)
            row["g200_over_g256"] = round(med["g200"] / med["g256"], 4)
        if "parent_a" in variants:
            row["cycle_over_parent"] = [round(med["cycle_" + x] / med["parent_" + y], 5) for x in "ab" for y in "ab"]
            row["parent_aa_spread"] = round(H.spread(med["parent_a"], med["parent_b"]), 5)
        rows[shape] = row
        print("%-8s %6d entries  " % (shape, k) + "  ".join("%s %.4f" % (v, med[v]) for v in variants) + " ms", flush=True)
        for b in (sbuf, dbuf, tb, tb_plain, ws, res, res_base):
            b.free()
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_cycle_digest_table.py", "TB/s of n bytes cycled per pass", a), "key": KEY, "shipped_grid": shipped,
                            "table_kernel_source_hash": M.table_kernel_source_hash(),
                            "other_table_kernel_source_hash": other.modgpu_table_kernel_source_hash().decode() if other is not None else None,
                            "shapes": rows})


if __name__ == "__main__":
    main()
