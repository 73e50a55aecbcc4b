"""CPU checks of the cycle digest table call (modgpu_cycle_digest_table_device & co., include/modgpu.h): the symbols are declared and
exported, the workspace is the out-of-place table call's, tier 1 comes before any device work, the table TU's code-generation guard
passes the stream kernel with two loops and every rule of the new loop fires on altered assembly, and the host code runs under ASan +
UBSan against the CPU stand-in of the HIP runtime as a stand-alone program (its own main, run directly, the sanitizer runtimes linked
statically)."""
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
PUBLIC = {"modgpu_cycle_digest_table_workspace_bytes", "modgpu_cycle_digest_table_device"}
TESTING = {"modgpu_time_cycle_digest_table_device"}
HOOK = "modgpu_debug_set_cycle_digest_table_grid"


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
    assert re.search(r"#define MODGPU_DIGEST_OUTPUT 0u", pub) and re.search(r"#define MODGPU_DIGEST_INPUT 1u", pub)
    assert (modgpu.DIGEST_OUTPUT, modgpu.DIGEST_INPUT) == (0, 1)
    assert "18 = the cycle digest table call's stream launch" in tst and "modgpu_table_kernel_source_hash() for variant 18" in tst
    shipped, hooks = exported(modgpu.lib_path("shipped")), exported(modgpu.lib_path("testing"))
    assert PUBLIC | TESTING <= shipped and PUBLIC | TESTING | {HOOK} <= hooks and HOOK not in shipped
    assert modgpu.lib().modgpu_abi_version() == 8
    for f in ("cycle_digest_table_workspace_bytes", "cycle_digest_table_device", "time_cycle_digest_table_device", "debug_set_cycle_digest_table_grid"):
        assert callable(getattr(modgpu, f)), f
    assert callable(modgpu.DeviceBuffer.extract)


def test_workspace_is_the_table_calls(modgpu):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "table_workspace_bytes.json")))
    assert len(gold["n_entries"]) == 16
    for n in gold["n_entries"]:
        assert modgpu.cycle_digest_table_workspace_bytes(n) == modgpu.table_workspace_bytes(n) == gold["table"][str(n)], n
    assert modgpu.cycle_digest_table_workspace_bytes(0) == 0 and modgpu.cycle_digest_table_workspace_bytes(MAX_ENTRIES + 1) == 0


def test_without_a_gpu_the_call_fails_with_no_device(modgpu):
    """Tier 1 comes first (MODGPU_ERR_INVALID, nothing queued), a bad side among it; a well-formed call gets as far as the device and
    fails there."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    t, r, ws = np.zeros(64, np.uint64), np.zeros(64, np.uint64), np.zeros(4096, np.uint64)
    wb = modgpu.cycle_digest_table_workspace_bytes(3)
    before = modgpu.path_stats()
    assert L.modgpu_cycle_digest_table_device(t.ctypes.data, 3, r.ctypes.data, 2, ws.ctypes.data, wb, -1, None) == 1
    assert "side is neither the output side (0) nor the input side (1)" in L.modgpu_last_error().decode()
    assert L.modgpu_cycle_digest_table_device(None, 0, None, 0xFFFFFFFF, None, 0, -1, None) == 1
    assert L.modgpu_cycle_digest_table_device(t.ctypes.data, 3, None, 0, ws.ctypes.data, wb, -1, None) == 1
    assert "null results" in L.modgpu_last_error().decode()
    assert L.modgpu_cycle_digest_table_device(t.ctypes.data, 3, r.ctypes.data + 4, 1, ws.ctypes.data, wb, -1, None) == 1
    assert L.modgpu_cycle_digest_table_device(t.ctypes.data, 3, r.ctypes.data, 1, ws.ctypes.data, wb - 1, -1, None) == 1
    assert "modgpu_cycle_digest_table_workspace_bytes" in L.modgpu_last_error().decode()
    assert L.modgpu_cycle_digest_table_device(t.ctypes.data, MAX_ENTRIES + 1, None, 0, ws.ctypes.data, 1 << 40, -1, None) == 1
    assert "more than 4194304 entries" in L.modgpu_last_error().decode()
    assert L.modgpu_cycle_digest_table_device(None, 0, None, 0, None, 0, -1, None) == 0
    for side in (0, 1):
        assert L.modgpu_cycle_digest_table_device(t.ctypes.data, 3, r.ctypes.data, side, ws.ctypes.data, wb, -1, None) == 2  # MODGPU_ERR_NO_DEVICE
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] and st["scalar_calls"] == before["scalar_calls"]
    assert not ws.any() and not r.any()


def test_a_null_device_table_is_refused_not_taken_for_an_empty_one(modgpu):
    freed = object.__new__(modgpu.DeviceBuffer)  # as DeviceBuffer.free() leaves one (made without a device)
    freed.nbytes, freed.device, freed.ptr = 4096, -1, None
    ws, res = np.zeros(1 << 16, np.uint64), np.zeros(4 * 3, np.uint64)
    before = modgpu.path_stats()["gpu_launches"]
    for table in (freed, None):
        with pytest.raises(modgpu.ModGpuError, match="null table or workspace"):
            modgpu.cycle_digest_table_device(table, res.ctypes.data, modgpu.DIGEST_INPUT, ws.ctypes.data, n=3)
    assert modgpu.path_stats()["gpu_launches"] == before and not ws.any() and not res.any()
    rec, adler = modgpu.cycle_digest_table_device(modgpu.table(0))
    assert rec.size == 0 and adler.size == 0 and rec.dtype == modgpu.DIGEST_RESULT_DTYPE and adler.dtype == np.uint32


def test_the_call_goes_through_the_one_shared_body():
    capi = open(os.path.join(CSRC, "modgpu_capi.cpp")).read()
    impl = capi[capi.index("int table_impl("):capi.index("int cycle_digest_table_impl(")]
    assert impl.count("return table_call(") == 1 and "kCycleDigestTable" in impl and "modgpu_launch_cycle_digest_table_stream" in impl
    assert capi.count("int table_call(") == 1 and capi.count("return table_call(") == 6 and capi.count("hipEventElapsedTime(") == 1
    assert capi.count('"null table or workspace"') == 1 and capi.count('"more than 4194304 entries') == 3
    assert "force_table_grid(kCycleDigestTable, grid)" in capi


def test_codegen_guard_of_the_kernel_with_two_loops():
    """`make isa-check-table` passes the tree (still 3 kernels); the stand-in is wired, and is no row of TABLE."""
    B.isa_check_target("isa-check-table", 3)
    B.standin_is_wired("standin_launch_cycle_digest_table.cpp")
    assert "cycle_digest_table" not in B.make_var("TUS").split()


def test_cycle_digest_loop_rules_on_altered_assembly():
    """The new rules of check_isa.check() on the tree's own assembly with one fault put in by hand, in the new loop"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_table_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_table_kernel.s")).read()
    assert ci.check(asm) == []
    stream = next(n for n in ci.kernel_bodies(asm) if "modgpu_cycle_table_kernel" in n)
    at = asm.index(stream + ":")
    body = ci.kernel_bodies(asm)[stream]
    # 8 per word, 4 words, 2 trips, in the keyed and in the copying branch (the compiler merges some of the latter); a pair of adds per trip
    assert 64 <= body.count("v_dot4_u32_u8") <= 128 and len(re.findall(r"^\s+global_atomic_add_x2", body, re.M)) == 4
    assert len(ci.code_lines(body, "buffer_store_dwordx4")) == 16 and len(ci.carry_blocks(body)) == 16  # both loops
    dot = asm.index("v_dot4_u32_u8", at)  # the new loop: where the first sum is taken
    add = asm.index("global_atomic_add_x2", dot)  # ... the first pair of adds behind it
    add_end = asm.index("\n", add)
    store = asm.index(" nt sc1\n", dot)  # ... and the first store behind it
    cases = {
        "no v_dot4_u32_u8": asm[:at] + asm[at:].replace("v_dot4_u32_u8", "v_dot2_u32_u16"),
        "a 64-bit atomic returns its value": asm[:add_end] + " sc0" + asm[add_end:],
        "no ds_add_u32": asm[:at] + asm[at:].replace("ds_add_u32", "ds_max_u32"),
        "a store of the cycle digest loop is not nt sc1": asm[:store] + " sc1\n" + asm[store + len(" nt sc1\n"):],
        "a store through a pointer in the kernel of the cycle digest loop": asm[:add] + "global_store_dwordx2 v1, v[2:3], s[2:3]\n\t" + asm[add:],
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_cycle_digest_table_on_the_standin_under_asan_ubsan():
    """tests/cycle_digest_table_main.cpp: every edge size at five destination phases and four source phase differences on both sides,
    table lengths across the level and record edges, empty entries only, dst == src, every device refusal and every host refusal with
    its text, every destination byte, every guard byte and every record against a model."""
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle-digest-table-main"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", MODGPU_REQUIRE_GPU="0")
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "cycle_digest_table_main")], env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1] == f"{len(lines) - 1} passed, 0 failed" and len(lines) - 1 == 81, lines[-1]
    sized = [f"sizes at dst phase {p} src +{d} side={s}" for p in (0, 1, 5, 15, 65535) for d in (0, 1, 3, 5) for s in (0, 1)]
    for what in sized + ["length 1 ", "length 16 ", "length 17 ", "length 1024 ", "length 1025 ", "length 4097 ", "empty entries only side=0",
                         "empty entries only side=1", "dst == src at phase 0 side=0", "dst == src at phase 65535 side=1",
                         "device refusal: a null source", "device refusal: a null destination", "device refusal: nonzero flags",
                         "device refusal: an entry of 1 TiB", "refusal: a side that is neither", "refusal: too many entries", "refusal: null table",
                         "refusal: null workspace", "refusal: misaligned table", "refusal: misaligned workspace", "refusal: short workspace",
                         "refusal: table that is not device memory", "refusal: workspace that is not device memory", "refusal: null results",
                         "refusal: misaligned results", "refusal: results that are not device memory", "refusal: timing without iterations",
                         "refusals queued nothing"]:
        assert any(ln.startswith(f"ok   cycle digest table: {what}") for ln in lines), what
    assert lines[0] == "ok   workspace sizes" and lines[-2].startswith("ok   launches: ") and lines[-2].endswith(", 0 plan errors")
