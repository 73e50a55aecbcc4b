#!/usr/bin/env python3
"""The rekey verify pass (modgpu_verify_rekey_device: is `expect` what the rekey makes of `src`? -- a read-only pass over 2n bytes under
two keystreams) against the rekey pass on the same buffers (modgpu_rekey_device_to: the same 2n bytes and the same keystream work, plus
stores), which is the yardstick DESIGN 4.12 sets.  tools/bench_verify.py's method: one process, one stream, HIP events recorded on that
stream around every single pass; the variants alternate step by step so drift hits all of them alike.  Rate unit: 2n bytes per pass.

    variants   vr                  clean, expect and src at phase 0, shipped grid (one workgroup per CU)
               rekey, rekey_again  modgpu_rekey_device_to on the same buffers, twice per step: their medians' distance is the A/A spread
               vr_mis              clean, src at phase 5 (the v_alignbyte_b32 funnel);   rekey_mis   the rekey at the same phases
               vr_wrong            the wrong key_to: every byte takes the slow path
    at the largest size also
               vr_batch / rekey_batch   16 equal entries in one call
               route_today         what a caller has without this call: modgpu_rekey_device_to into scratch as large as the data, then
                                   modgpu_verify_device with the identity key between `expect` and the scratch (both passes inside one
                                   pair of events)

    python tools/bench_verify_rekey.py [--sizes-kib 64,1024,16384,4194304] [--warmup 3] [--steps 20] [--out profiles/r13_verify_rekey.json]
"""
import bench_common as H

M, Stream, hip, _ok = H.setup()

SINGLE = ("vr", "rekey", "rekey_again", "vr_mis", "rekey_mis", "vr_wrong")
LARGEST = ("vr_batch", "rekey_batch", "route_today")
KF, KT, WRONG = M.KEY_PS3, M.KEY_PS4, 12345
OF, OT = 3, (1 << 32) + 11


def one_pass(v, B, n, st):
    """B: src (+64 bytes of room), dst (= rekey of src at phase 0), dst_mis (= rekey of src + 5), scratch, res (16 results)"""
    s = st.handle
    if v in ("vr", "vr_wrong"):
        M.verify_rekey_device(B["dst"], B["src"], KF, WRONG if v == "vr_wrong" else KT, OF, OT, result=B["res"], n=n, stream=s)
    elif v == "vr_mis":
        M.verify_rekey_device(B["dst_mis"], B["src"] + 5, KF, KT, OF, OT, result=B["res"], n=n, stream=s)
    elif v in ("rekey", "rekey_again"):
        M.rekey_device_to(B["dst"], B["src"], KF, KT, OF, OT, n=n, stream=s)
    elif v == "rekey_mis":
        M.rekey_device_to(B["dst_mis"], B["src"] + 5, KF, KT, OF, OT, n=n, stream=s)
    elif v == "route_today":
        M.rekey_device_to(B["scratch"], B["src"], KF, KT, OF, OT, n=n, stream=s)
        M.verify_device(B["dst"], B["scratch"], 0, 0, result=B["res"], n=n, stream=s)
    else:
        part = n // 16
        d = [B["dst"] + i * part for i in range(16)]
        sp = [B["src"] + i * part for i in range(16)]
        f, t = [OF + i * part for i in range(16)], [OT + i * part for i in range(16)]
        if v == "vr_batch":
            M.verify_rekey_batch_device(d, sp, [part] * 16, KF, KT, B["res"], offs_from=f, offs_to=t, stream=s)
        else:
            M.rekey_batch_device_to(d, sp, [part] * 16, KF, KT, offs_from=f, offs_to=t, stream=s)
    return M.last_launch()


def main():
    a = H.arguments("r13_verify_rekey.json", sizes_kib="64,1024,16384,4194304").parse_args()
    assert a.warmup >= 3 and a.steps >= 20, "at least 3 warm-ups and 20 timed steps"
    st = Stream()
    rows = {}
    sizes = [int(x) << 10 for x in a.sizes_kib.split(",")]
    for n in sizes:
        largest = n == max(sizes) and n % 16 == 0
        sbuf, dbuf, mbuf, rbuf = M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64), M.DeviceBuffer(32 * 16)
        xbuf = M.DeviceBuffer(n + 64) if largest else None
        H.fill(sbuf, n + 64)
        B = {"src": sbuf.ptr, "dst": dbuf.ptr, "dst_mis": mbuf.ptr, "res": rbuf.ptr, "scratch": xbuf.ptr if xbuf else 0}  # hipMalloc: phase 0
        variants = SINGLE + (LARGEST if largest else ())
        order = [v for v in variants if v.startswith("rekey")] + [v for v in variants if not v.startswith("rekey")]  # the rekey passes make `expect`
        seen = {}

        def checked(v, info):
            if not v.startswith("rekey"):
                r = M.verify_results(rbuf, 16 if v == "vr_batch" else 1)
                seen[v] = {"mismatches": int(r["mismatches"].sum()), "first_mismatch": int(r["first_mismatch"].min()), "n": int(r["n"].sum())}
                assert seen[v]["n"] == n and (seen[v]["mismatches"] == 0) == (v != "vr_wrong"), (v, seen[v])

        times, info, _ = H.measure(st, variants, lambda v: one_pass(v, B, n, st), a.warmup, a.steps, warm_order=order, after_warmup=checked)
        row = {"bytes": n, "launch": {v: H.launch_row(info[v]) for v in order}, "results": seen}
        for v in variants:
            row[v] = H.stats(times[v], n, 2, "TBps_2n")
        med = {v: row[v]["median_ms"] for v in variants}
        spread = H.spread(med["rekey"], med["rekey_again"])
        bound = max(1.05, 1 + 2 * spread)
        row["aa_spread_of_rekey"] = round(spread, 5)
        row["bound"] = round(bound, 5)
        row["vr_over_rekey"] = round(med["vr"] / med["rekey"], 4)
        row["vr_mis_over_rekey_mis"] = round(med["vr_mis"] / med["rekey_mis"], 4)
        row["vr_wrong_over_vr"] = round(med["vr_wrong"] / med["vr"], 4)
        if largest:
            row["vr_batch_over_rekey_batch"] = round(med["vr_batch"] / med["rekey_batch"], 4)
            row["route_today_over_vr"] = round(med["route_today"] / med["vr"], 4)
        rows[str(n)] = row
        print("%8d KiB  " % (n >> 10) + "  ".join("%s %.4f ms" % (v, med[v]) for v in variants) + "  | vr/rekey %.3f mis %.3f bound %.3f"
              % (row["vr_over_rekey"], row["vr_mis_over_rekey_mis"], bound), flush=True)
        for b in (sbuf, dbuf, mbuf, rbuf) + ((xbuf,) if xbuf else ()):
            b.free()
    st.destroy()
    H.write_profile(a.out, {
        **H.profile_head("bench_verify_rekey.py", "TB/s of 2n bytes per pass (rekey verify: 2n read; rekey: n read + n written)", a),
        "key_from": KF, "key_to": KT, "wrong_key_to": WRONG, "off_from": OF, "off_to": OT,
        "rule": "the rekey verify's median <= the rekey median x max(1.05, 1 + 2 x A/A spread of the rekey pass in the same run)",
        "rekey_verify_kernel_source_hash": M.rekey_verify_kernel_source_hash(), "rekey_kernel_source_hash": M.rekey_kernel_source_hash(),
        "verify_kernel_source_hash": M.verify_kernel_source_hash(), "misaligned": "src phase 5, expect / dst phase 0", "sizes": rows})


if __name__ == "__main__":
    main()
