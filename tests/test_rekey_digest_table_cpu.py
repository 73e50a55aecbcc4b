"""CPU checks of the rekey digest table call (modgpu_rekey_digest_table_device & co., include/modgpu.h): the symbols are declared and
exported, the workspace is the rekey table call's, tier 1 comes before any device work, the rekey table TU's code-generation guard
passes the stream kernel with two loops, rejects a digest loop that stores through its source's descriptor, and every rule of the new
loop fires on altered assembly, and the host code runs under ASan + UBSan against the CPU stand-in of the HIP runtime as a stand-alone
program (its own main, run directly, the sanitizer runtimes linked statically)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
MAX_ENTRIES = 1 << 22  # MODGPU_TABLE_MAX_ENTRIES
PUBLIC = {"modgpu_rekey_digest_table_workspace_bytes", "modgpu_rekey_digest_table_device"}
TESTING = {"modgpu_time_rekey_digest_table_device"}
HOOK = "modgpu_debug_set_rekey_digest_table_grid"
BAD_SIDE = "side is neither the output side (0), the input side (1) nor the plaintext between the keystreams (2)"


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_symbols_declared_exported_and_listed(modgpu):
    pub = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    tst = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    for s in PUBLIC:
        assert re.search(r"\b%s\(" % s, pub) and s in modgpu.EXPORTS, s
    for s in TESTING:
        assert re.search(r"\b%s\(" % s, tst) and s in modgpu.TESTING_EXPORTS, s
    assert re.search(r"\b%s\(" % HOOK, tst) and HOOK in modgpu.DEBUG_EXPORTS
    assert re.search(r"#define MODGPU_DIGEST_PLAIN 2u", pub) and modgpu.DIGEST_PLAIN == 2
    assert "20 = the rekey digest table call's stream launch" in tst and "modgpu_rekey_table_kernel_source_hash() for variant 20" in tst
    shipped, hooks = exported(modgpu.lib_path("shipped")), exported(modgpu.lib_path("testing"))
    assert PUBLIC | TESTING <= shipped and PUBLIC | TESTING | {HOOK} <= hooks and HOOK not in shipped
    assert modgpu.lib().modgpu_abi_version() == 8
    for f in ("rekey_digest_table_workspace_bytes", "rekey_digest_table_device", "time_rekey_digest_table_device", "debug_set_rekey_digest_table_grid"):
        assert callable(getattr(modgpu, f)), f
    assert callable(modgpu.DeviceBuffer.convert) and callable(modgpu.DeviceBuffer.convert_checked)
    assert "modgpu_rekey_digest_table_device" in pub[pub.index("DIGEST CHECK"):pub.index("int modgpu_digest_check_device(")]


def test_workspace_is_the_rekey_table_calls(modgpu):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "table_workspace_bytes.json")))
    for n in gold["n_entries"]:
        assert modgpu.rekey_digest_table_workspace_bytes(n) == modgpu.rekey_table_workspace_bytes(n) > 0, n
    assert modgpu.rekey_digest_table_workspace_bytes(0) == 0 and modgpu.rekey_digest_table_workspace_bytes(MAX_ENTRIES + 1) == 0


def test_without_a_gpu_the_call_fails_with_no_device(modgpu):
    """Tier 1 comes first (MODGPU_ERR_INVALID with its text, nothing queued), a bad side among it; a well-formed call gets as far as the
    device and fails there.  The cycle digest table call keeps refusing side 2."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    t, r, ws = np.zeros(64, np.uint64), np.zeros(64, np.uint64), np.zeros(4096, np.uint64)
    tp, rp, wp = t.ctypes.data, r.ctypes.data, ws.ctypes.data
    wb = modgpu.rekey_digest_table_workspace_bytes(3)
    before = modgpu.path_stats()

    def refused(text, *args):
        assert L.modgpu_rekey_digest_table_device(*args, -1, None) == 1, text
        assert text in L.modgpu_last_error().decode(), (text, L.modgpu_last_error().decode())

    refused(BAD_SIDE, tp, 3, rp, 3, wp, wb)
    refused(BAD_SIDE, None, 0, None, 0xFFFFFFFF, None, 0)
    refused("null table or workspace", None, 3, rp, 2, wp, wb)
    refused("null table or workspace", tp, 3, rp, 2, None, wb)
    refused("null results", tp, 3, None, 2, wp, wb)
    refused("table or workspace not 8-byte aligned", tp + 4, 3, rp, 2, wp, wb)
    refused("table or workspace not 8-byte aligned", tp, 3, rp, 2, wp + 4, wb)
    refused("results not 8-byte aligned", tp, 3, rp + 4, 1, wp, wb)
    refused("workspace smaller than modgpu_rekey_digest_table_workspace_bytes(n_entries)", tp, 3, rp, 1, wp, wb - 1)
    refused("workspace smaller than modgpu_rekey_digest_table_workspace_bytes(n_entries)", tp, 3, rp, 1, wp, modgpu.table_workspace_bytes(3))
    refused("more than 4194304 entries", tp, MAX_ENTRIES + 1, None, 0, wp, 1 << 40)
    assert L.modgpu_rekey_digest_table_device(None, 0, None, 0, None, 0, -1, None) == 0
    for side in (0, 1, 2):
        assert L.modgpu_rekey_digest_table_device(tp, 3, rp, side, wp, wb, -1, None) == 2  # MODGPU_ERR_NO_DEVICE
    assert L.modgpu_cycle_digest_table_device(tp, 3, rp, 2, wp, modgpu.cycle_digest_table_workspace_bytes(3), -1, None) == 1
    assert "side is neither the output side (0) nor the input side (1)" in L.modgpu_last_error().decode()
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] and st["scalar_calls"] == before["scalar_calls"]
    assert not ws.any() and not r.any()


def test_the_call_goes_through_the_one_shared_body():
    capi = open(os.path.join(CSRC, "modgpu_capi.cpp")).read()
    impl = capi[capi.index("int rekey_table_impl("):capi.index("int rekey_digest_table_impl(")]
    assert impl.count("return table_call(") == 1 and "kRekeyDigestTable" in impl and "modgpu_launch_rekey_digest_table_stream" in impl
    assert "rekey_table_layout(n)" in impl and "force_table_grid(kRekeyDigestTable, grid)" in capi


def test_codegen_guard_of_the_kernel_with_two_loops():
    """`make isa-check-rekey-table` passes the tree (still 3 kernels); a digest loop that stores through the source's descriptor is
    REJECTED in the new rule's words; the stand-in is wired, and is no row of TABLE."""
    B.isa_check_target("isa-check-rekey-table", 3)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-rekey-table-digest"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a digest loop that stores through its source's descriptor"
    assert "a store of the rekey digest loop is not nt sc1 (24 buffer stores, expected 16 whole words" in broken.stdout, broken.stdout[-3000:]
    B.standin_is_wired("standin_launch_rekey_digest_table.cpp")
    assert "rekey_digest_table" not in B.make_var("TUS").split()


def test_rekey_digest_loop_rules_on_altered_assembly():
    """Every rule of rekey_digest_table_loop on the tree's own assembly with one fault put in by hand, in the new loop"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_rekey_table_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_rekey_table_kernel.s")).read()
    assert ci.check(asm) == []
    stream = next(n for n in ci.kernel_bodies(asm) if "modgpu_cycle_rekey_table_kernel" in n)
    at = asm.index(stream + ":")
    body = ci.kernel_bodies(asm)[stream]
    # 8 sums per word, 4 words, 2 trips; a pair of adds per trip; both loops' stores and blocks; the summed word's own v_bitop3_b32
    assert body.count("v_dot4_u32_u8") == 64 and len(re.findall(r"^\s+global_atomic_add_x2", body, re.M)) == 4
    assert len(ci.code_lines(body, "buffer_store_dwordx4")) == 16 and len(ci.carry_blocks(body)) == 16
    assert len(re.findall(r"v_bitop3_b32 .*bitop3:0x96", body)) == 64 and len(re.findall(r"v_bitop3_b32 .*bitop3:0x78", body)) == 64
    dot = asm.index("v_dot4_u32_u8", at)  # the new loop: where the first sum is taken
    add = asm.index("global_atomic_add_x2", dot)  # ... the first pair of adds behind it
    add_end = asm.index("\n", add)
    store = asm.index(" nt sc1\n", dot)  # ... and the first store behind it
    ticket = asm.index("global_atomic_add ", dot)  # ... and the first ticket fetch behind it
    ticket_end = asm.index(" sc0", ticket)
    cases = {
        "no v_dot4_u32_u8": asm[:at] + asm[at:].replace("v_dot4_u32_u8", "v_dot2_u32_u16"),
        "a 64-bit atomic returns its value": asm[:add_end] + " sc0" + asm[add_end:],
        "expected 4 global_atomic_add_x2": asm[:add] + "global_atomic_umin_x2" + asm[add + len("global_atomic_add_x2"):],
        "expected the ticket fetch of each unrolled trip of both loops (4)": asm[:ticket_end] + asm[ticket_end + len(" sc0"):],
        "no ds_add_u32": asm[:at] + asm[at:].replace("ds_add_u32", "ds_max_u32"),
        "a store of the rekey digest loop is not nt sc1": asm[:store] + " sc1\n" + asm[store + len(" nt sc1\n"):],
        "a store through a pointer in the kernel of the rekey digest loop": asm[:add] + "global_store_dwordx2 v1, v[2:3], s[2:3]\n\t" + asm[add:],
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])
    # the block count says both loops: a kernel with the plain loop's 8 blocks alone is not this TU's stream kernel
    k = ci.Kernel(stream, "modgpu_cycle_rekey_table_kernel", body, ci.metadata(asm, stream))
    assert ci.block_count(k, ci.TWO_KEYSTREAM, 16, "") == [] and ci.block_count(k, ci.TWO_KEYSTREAM, 8, "") != []


def test_rekey_digest_table_on_the_standin_under_asan_ubsan():
    """tests/rekey_digest_table_main.cpp: every edge size at four destination phases and three source shifts on all three sides, every
    degenerate key pair, table lengths across the level and record edges with empty entries, empty entries only, dst == src, every
    device refusal (nothing written) and every host refusal with its text, every byte of both arenas and every record against a model
    written from lcg.h and the closed form."""
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "rekey-digest-table-main"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", MODGPU_REQUIRE_GPU="0")
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "rekey_digest_table_main")], env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1] == f"{len(lines) - 1} passed, 0 failed" and len(lines) - 1 == 99, lines[-1]
    sized = [f"sizes at dst phase {p} src +{d} side={s}" for p in (0, 1, 15, 65535) for d in (0, 1, 3) for s in (0, 1, 2)]
    pairs = [f"key pair {p} side={s}" for p in range(8) for s in (0, 2)]
    for what in sized + pairs + ["length 1 ", "length 16 ", "length 17 ", "length 1024 ", "length 1025 ", "empty entries only side=0",
                                 "empty entries only side=1", "empty entries only side=2", "dst == src at phase 0 side=0",
                                 "dst == src at phase 5 side=1", "dst == src at phase 65535 side=2", "device refusal: a null source",
                                 "device refusal: a null destination", "device refusal: nonzero flags", "device refusal: nonzero reserved",
                                 "device refusal: an entry of 1 TiB", "refusal: a side that is none of the three", "refusal: too many entries",
                                 "refusal: null table", "refusal: null workspace", "refusal: misaligned table", "refusal: misaligned workspace",
                                 "refusal: short workspace", "refusal: the out-of-place table's workspace size",
                                 "refusal: table that is not device memory", "refusal: workspace that is not device memory", "refusal: null results",
                                 "refusal: misaligned results", "refusal: results that are not device memory",
                                 "refusal: the cycle digest table call still refuses side 2", "refusal: timing without iterations",
                                 "refusals queued nothing"]:
        assert any(ln.startswith(f"ok   rekey digest table: {what}") for ln in lines), what
    assert lines[0] == "ok   workspace sizes" and lines[-2].startswith("ok   launches: ") and lines[-2].endswith(", 0 plan errors")
