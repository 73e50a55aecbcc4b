#!/usr/bin/env python3
"""The rekey digest table call (modgpu_rekey_digest_table_device: modgpu_rekey_table_device and one digest record per entry in one pass
and three launches) against what a caller had before: modgpu_rekey_table_device followed by modgpu_digest_table_device over a second
table of 40-byte entries built from src, key_from and off_from, on the same stream (3n bytes of traffic, six launches; that table is
built once, outside the timing).  One process, one stream, HIP events recorded on that stream around every single pass; the variants
alternate step by step so drift hits all of them alike.  Rate unit: n bytes rekeyed per pass.  Before anything is timed the fused call's
records are compared with modgpu_digest_table_device's (plain side: the sources under key_from at off_from; input side: under the
identity key; output side: the result under the identity key) and its destination with modgpu_rekey_table_device's, byte for byte.

    shapes     64k, 1m, 16m 1 entry, launch-bound sizes
               4g           1 x 4 GiB, destination and source chunk-aligned
               4g_p5        the same with the source at phase 5
               16kx64k      16 384 x 64 KiB at random phases
               config4      100 000 entries of [0, 64 KiB] (seeded), relocated as in a part (the rekey table tool's table)
    variants   fused_plain  the call at its shipped grid, MODGPU_DIGEST_PLAIN
               fused_out, fused_in   the same, MODGPU_DIGEST_OUTPUT / _INPUT
               g200, g256   fused_plain on 200 and on 256 stream workgroups (testing flavour: modgpu_debug_set_rekey_digest_table_grid)
               two_a, two_b modgpu_rekey_table_device + modgpu_digest_table_device, twice per step: their difference is the A/A spread
               rekey_a, _b  modgpu_rekey_table_device alone, twice per step
               cyc_fused, cyc   modgpu_cycle_digest_table_device (output side) and modgpu_cycle_table_device over the same ranges under
                            key_from: what the sums cost the one-keystream loop, in the same run
               parent_a, _b modgpu_rekey_table_device of another build's library (--other-lib) loaded into this process, twice per step

    python tools/bench_rekey_digest_table.py [--shapes ...] [--warmup 3] [--steps 20] [--other-lib PATH] [--out profiles/r22_rekey_digest_table.json]
"""
import ctypes
import os

import numpy as np

import bench_common as H

M, Stream, hip, _ok = H.setup()

KEY_FROM, KEY_TO = M.KEY_PS3, M.KEY_PS4
GRIDS = {"fused_plain": 0, "fused_out": 0, "fused_in": 0, "g200": 200, "g256": 256}
_vp = ctypes.c_void_p


def layout(shape):
    """(sizes, src offsets, dst offsets, off_from, off_to, src bytes, dst bytes), offsets from chunk-aligned bases: the rekey table tool's
    tables, and the single entries of the digest tools (4g_p5: the source at phase 5)"""
    if shape in H.LAYOUT_SHAPES["rekey_table"]:
        return H.table_layout("rekey_table", shape)
    sz = np.array([H.SINGLE_ENTRY[shape]], np.int64)
    src = np.array([5 if shape == "4g_p5" else 0], np.int64)
    zero = np.zeros(1, np.int64)
    return sz, src, zero, zero + 12345, zero + (1 << 40) + 3, int(sz[0]) + 64 + 5, int(sz[0]) + 64


def main():
    a = H.arguments("r22_rekey_digest_table.json", shapes="64k,1m,16m,4g,4g_p5,16kx64k,config4", other_lib="").parse_args()
    assert a.warmup >= 1 and a.steps >= 1
    M.use_testing_flavour()  # the same device code as libmodgpu.so, plus the switch of the stream grid
    M.debug_set_rekey_digest_table_grid(0)
    other = None
    if a.other_lib:
        other = H.other_library(os.path.abspath(a.other_lib), ["modgpu_rekey_table_device", "modgpu_rekey_table_kernel_source_hash"], M.lib())
    st = Stream()
    rows = {}
    shipped = None
    for shape in a.shapes.split(","):
        sz, so, do, ofr, oto, sn, dn = layout(shape)
        n_bytes, k = int(sz.sum()), sz.size
        sbuf, dbuf = M.DeviceBuffer(sn + 65536 + 16), M.DeviceBuffer(dn + 65536)
        sbase, dbase = -sbuf.ptr % 65536, -dbuf.ptr % 65536  # the layout's offsets count from a chunk edge
        H.fill(sbuf, sn, offset=sbase)
        t = M.rekey_table(k)
        t["dst"], t["src"], t["n"] = dbuf.ptr + dbase + do, sbuf.ptr + sbase + so, sz
        t["off_from"], t["off_to"], t["key_from"], t["key_to"] = ofr, oto, M.as_int32(KEY_FROM), M.as_int32(KEY_TO)
        M.rekey_table_validate(t)
        # the second table of the two-call route, and its kin for the checks: 40-byte entries over the sources (under key_from, or as they
        # are) and over the result (as it is)
        d = M.table(k)
        d["dst"], d["src"], d["n"], d["stream_off"], d["key"] = t["dst"], t["src"], sz, ofr, M.as_int32(KEY_FROM)
        d_in, d_out = d.copy(), d.copy()
        d_in["key"] = 0
        d_out["key"], d_out["src"] = 0, t["dst"]
        tabs = {}
        for name, tab in (("rekey", t), ("plain", d), ("in", d_in), ("out", d_out)):
            tabs[name] = M.DeviceBuffer(tab.nbytes)
            tabs[name].upload(tab.view(np.uint8))
        ws = M.DeviceBuffer(M.rekey_digest_table_workspace_bytes(k))
        res, res_base = M.DeviceBuffer(32 * k), M.DeviceBuffer(32 * k)
        variants = ["fused_plain", "fused_out", "fused_in", "two_a", "two_b", "rekey_a", "rekey_b", "cyc_fused", "cyc"]
        if shape in ("4g", "4g_p5"):
            variants += ["g200", "g256"]
        if other is not None and shape in ("4g", "config4"):
            variants += ["parent_a", "parent_b"]
        sides = {"fused_out": M.DIGEST_OUTPUT, "fused_in": M.DIGEST_INPUT}

        def one_pass(v):
            if v in GRIDS:
                M.debug_set_rekey_digest_table_grid(GRIDS[v])
                M.rekey_digest_table_device(tabs["rekey"], res, sides.get(v, M.DIGEST_PLAIN), ws, n=k, stream=st.handle)
            elif v.startswith("two"):
                M.rekey_table_device(tabs["rekey"], ws, n=k, stream=st.handle)
                M.digest_table_device(tabs["plain"], res_base, ws, n=k, stream=st.handle)
            elif v.startswith("rekey"):
                M.rekey_table_device(tabs["rekey"], ws, n=k, stream=st.handle)
            elif v == "cyc_fused":
                M.cycle_digest_table_device(tabs["plain"], res_base, M.DIGEST_OUTPUT, ws, n=k, stream=st.handle)
            elif v == "cyc":
                M.cycle_table_device(tabs["plain"], ws, n=k, stream=st.handle)
            elif v.startswith("parent"):
                if other.modgpu_rekey_table_device(_vp(tabs["rekey"].ptr), k, _vp(ws.ptr), ws.nbytes, -1, _vp(st.handle)):
                    raise RuntimeError("the other library refused the rekey table call")
                return {"kernel": "other library", "variant": 9, "grid": 0}
            return M.last_launch()

        # every value, before anything is timed: the two-call route's destination and records are the reference
        one_pass("two_a")
        st.sync()
        want = dict.fromkeys(("fused_plain", "g200", "g256"), M.digest_results(res_base, k)[1])
        probe = [(0, min(dn, 1 << 22)), (max(0, dn - (1 << 22)), min(dn, 1 << 22))]
        want_img = [dbuf.download(m, offset=dbase + o) for o, m in probe]
        for v, name in (("fused_in", "in"), ("fused_out", "out")):
            M.digest_table_device(tabs[name], res_base, ws, n=k, stream=st.handle)
            st.sync()
            want[v] = M.digest_results(res_base, k)[1]

        def wipe(v):
            if v in GRIDS:
                for o, m in probe:
                    dbuf.upload(np.zeros(m, np.uint8), offset=dbase + o)

        def checked(v, info):
            nonlocal shipped
            if v in GRIDS:
                assert M.table_status(ws) is None and info["variant"] == 20, (shape, v, info)
                if v == "fused_plain" and shipped is None:
                    shipped = info["grid"]
                assert np.array_equal(M.digest_results(res, k)[1], want[v]), (shape, v, "the fused call and the digest table call disagree")
                for (o, m), w in zip(probe, want_img):
                    assert np.array_equal(dbuf.download(m, offset=dbase + o), w), (shape, v, "the fused call and the rekey table call wrote different bytes")

        times, info, launches = H.measure(st, variants, one_pass, a.warmup, a.steps, before_warmup=wipe, after_warmup=checked)
        M.debug_set_rekey_digest_table_grid(0)
        row = {"entries": int(k), "bytes": n_bytes, "launch": {v: H.launch_row(info[v], launches[v]) for v in variants}}
        for v in variants:
            row[v] = H.stats(times[v], n_bytes, 1, "TBps")
        med = {v: row[v]["median_ms"] for v in variants}
        two, rekey = min(med["two_a"], med["two_b"]), min(med["rekey_a"], med["rekey_b"])
        row["two_call_aa_spread"] = round(H.spread(med["two_a"], med["two_b"]), 5)
        row["rekey_aa_spread"] = round(H.spread(med["rekey_a"], med["rekey_b"]), 5)
        for v in ("fused_plain", "fused_out", "fused_in"):
            row["two_call_over_" + v] = round(two / med[v], 4)
            row[v + "_over_rekey"] = round(med[v] / rekey, 4)
        row["cyc_fused_over_cyc"] = round(med["cyc_fused"] / med["cyc"], 4)
        if "g200" in variants:
            row["g200_over_g256"] = round(med["g200"] / med["g256"], 4)
        if "parent_a" in variants:
            row["rekey_over_parent"] = [round(med["rekey_" + x] / med["parent_" + y], 5) for x in "ab" for y in "ab"]
            row["parent_aa_spread"] = round(H.spread(med["parent_a"], med["parent_b"]), 5)
        rows[shape] = row
        print("%-8s %6d entries  " % (shape, k) + "  ".join("%s %.4f" % (v, med[v]) for v in variants) + " ms", flush=True)
        for b in (sbuf, dbuf, ws, res, res_base, *tabs.values()):
            b.free()
    st.destroy()
    H.write_profile(a.out, {**H.profile_head("bench_rekey_digest_table.py", "TB/s of n bytes rekeyed per pass", a), "key_from": KEY_FROM, "key_to": KEY_TO,
                            "shipped_grid": shipped, "rekey_table_kernel_source_hash": M.rekey_table_kernel_source_hash(),
                            "other_rekey_table_kernel_source_hash": other.modgpu_rekey_table_kernel_source_hash().decode() if other is not None else None,
                            "shapes": rows})


if __name__ == "__main__":
    main()
