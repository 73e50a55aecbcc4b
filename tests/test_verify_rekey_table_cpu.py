"""CPU checks of the rekey verify table call (modgpu_verify_rekey_table_device & co., include/modgpu.h): the symbols are declared,
exported and listed, the new TU has a source list and hash of its own, the workspace is the rekey table call's plus one line, tier 1
comes before the device, and the TU's code-generation guard passes the tree and rejects a broken build and hand-made faults.  The CPU
stand-in of the three launches is wired into the sanitizer builds of the library; no case file runs it under a sanitizer yet."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
PUBLIC = ("modgpu_verify_rekey_table_workspace_bytes", "modgpu_verify_rekey_table_device")
TESTING = ("modgpu_time_verify_rekey_table_device", "modgpu_rekey_verify_table_kernel_source_hash")
DEBUG = ("modgpu_debug_set_rekey_verify_table_grid",)
REKEY_VERIFY_TABLE_SRC = ("cycle_rekey_verify_table_kernel.hip", "cycle_table_impl.h", "cycle_rekey_verify_table_kernel.h", "cycle_rekey_table_kernel.h",
                          "cycle_verify_table_kernel.h", "cycle_table_kernel.h", "cycle_verify_kernel.h", "cycle_rekey_impl.h",
                          "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h")
MAX_ENTRIES = 1 << 22  # MODGPU_TABLE_MAX_ENTRIES


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_new_symbols_declared_exported_and_listed(modgpu):
    public = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    testing = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    assert re.search(r"\buint64_t modgpu_verify_rekey_table_workspace_bytes\(uint64_t n_entries\);", public)
    assert re.search(r"\bint modgpu_verify_rekey_table_device\(const modgpu_rekey_table_entry_t \*dev_entries,", public)
    assert re.search(r"\bint modgpu_time_verify_rekey_table_device\(", testing) and "modgpu_rekey_verify_table_kernel_source_hash(void);" in testing
    assert "void modgpu_debug_set_rekey_verify_table_grid(uint32_t grid);" in testing
    assert re.search(r"\b13 = the rekey verify table call's stream kernel", testing)
    assert "modgpu_rekey_verify_table_kernel_source_hash() for variant 13" in testing
    assert "#define MODGPU_ABI_VERSION 8\n" in public
    shipped, hooks = exported(modgpu.lib_path("shipped")), exported(modgpu.lib_path("testing"))
    assert set(PUBLIC + TESTING) <= shipped and set(PUBLIC + TESTING + DEBUG) <= hooks
    assert not set(DEBUG) & shipped, "the debug hook is in the shipped flavour"
    assert set(PUBLIC) <= set(modgpu.EXPORTS) and set(TESTING) <= set(modgpu.TESTING_EXPORTS) and set(DEBUG) <= set(modgpu.DEBUG_EXPORTS)
    for name in ("verify_rekey_table_workspace_bytes", "verify_rekey_table_device", "time_verify_rekey_table_device",
                 "rekey_verify_table_kernel_source_hash", "debug_set_rekey_verify_table_grid"):
        assert callable(getattr(modgpu, name)), name
    assert modgpu.lib().modgpu_abi_version() == 8


def test_source_list_and_hash(modgpu):
    assert tuple(B.make_var("REKEY_VERIFY_TABLE_SRC").split()) == REKEY_VERIFY_TABLE_SRC
    assert "cycle_rekey_verify_table_kernel.h" in B.make_var("CAPI_HDR").split()
    h = hashlib.sha256()
    for f in REKEY_VERIFY_TABLE_SRC:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    assert modgpu.rekey_verify_table_kernel_source_hash() == h.hexdigest()
    others = {modgpu.kernel_source_hash(), modgpu.feed_kernel_source_hash(), modgpu.to_kernel_source_hash(), modgpu.xfer_kernel_source_hash(),
              modgpu.rekey_kernel_source_hash(), modgpu.table_kernel_source_hash(), modgpu.rekey_table_kernel_source_hash(),
              modgpu.verify_kernel_source_hash(), modgpu.verify_table_kernel_source_hash(), modgpu.rekey_verify_kernel_source_hash(),
              modgpu.keep_kernel_source_hash()}
    assert len(others) == 11 and modgpu.rekey_verify_table_kernel_source_hash() not in others
    assert modgpu.kernel_source_hash().startswith("d2832a17dddf0901")


def test_workspace_is_the_rekey_table_calls_plus_one_line(modgpu):
    w = modgpu.verify_rekey_table_workspace_bytes
    for n in (1, 16, 17, 1000, MAX_ENTRIES):
        assert w(n) == modgpu.rekey_table_workspace_bytes(n) + 64, n
    assert w(0) == 0 and w(MAX_ENTRIES + 1) == 0


def test_tier_1_comes_before_the_device(modgpu):
    """Tier 1 comes first (MODGPU_ERR_INVALID, nothing queued); a well-formed call gets as far as the device and fails there."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    t, r, ws = np.zeros(64, np.uint64), np.zeros(64, np.uint64), np.zeros(4096, np.uint64)
    wb = modgpu.verify_rekey_table_workspace_bytes(3)
    before = modgpu.path_stats()
    assert L.modgpu_verify_rekey_table_device(t.ctypes.data, 3, None, ws.ctypes.data, wb, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(t.ctypes.data, 3, r.ctypes.data + 4, ws.ctypes.data, wb, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(t.ctypes.data + 4, 3, r.ctypes.data, ws.ctypes.data, wb, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(None, 3, r.ctypes.data, ws.ctypes.data, wb, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(t.ctypes.data, 3, r.ctypes.data, None, wb, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(t.ctypes.data, 3, r.ctypes.data, ws.ctypes.data, wb - 1, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(t.ctypes.data, 3, r.ctypes.data, ws.ctypes.data, modgpu.rekey_table_workspace_bytes(3), -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(t.ctypes.data, MAX_ENTRIES + 1, r.ctypes.data, ws.ctypes.data, 1 << 40, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(None, 0, None, None, 0, -1, None) == 0
    assert L.modgpu_verify_rekey_table_device(t.ctypes.data, 3, r.ctypes.data, ws.ctypes.data, wb, -1, None) == 2  # MODGPU_ERR_NO_DEVICE
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] and st["scalar_calls"] == before["scalar_calls"]
    assert not r.any() and not ws.any()


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-rekey-verify-table` passes the tree (3 kernels); the TU with a store of the difference in the stream loop is
    REJECTED by name; the object waits for its own guard run, which ISA_CHECK=0 leaves out; the TU is built with the atomic-optimizer
    flag; the object is on both link lines; the stand-in is wired."""
    B.isa_check_target("isa-check-rekey-verify-table", 3)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-rekey-verify-table"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a rekey verify table stream kernel that stores"
    assert "modgpu_cycle_rekey_verify_table_kernel" in broken.stdout and "a rekey verify kernel stores through a buffer descriptor" in broken.stdout, \
        broken.stdout[-3000:]
    B.standin_is_wired("standin_launch_rekey_verify_table.cpp")
    plan = B.dry_run("all")
    flag = "-amdgpu-atomic-optimizer-strategy=None"
    for step in ("-S --cuda-device-only", "-c"):
        lines = [ln for ln in plan if f" {step} cycle_rekey_verify_table_kernel.hip " in ln]
        assert len(lines) == 1 and f" -mllvm {flag} " in lines[0], (step, lines)
    assert sum(" cycle_rekey_verify_table_kernel.o " in ln for ln in plan if " -shared " in ln and "libmodgpu" in ln and "libmodulate_host" not in ln) == 2
    B.guard_then_compile("cycle_rekey_verify_table_kernel")
    B.unguarded_plan("cycle_rekey_verify_table_kernel")


def test_codegen_guard_rules_on_altered_assembly():
    """Each rule of the rekey verify table branch of check_isa.check() on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_rekey_verify_table_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_rekey_verify_table_kernel.s")).read()
    assert ci.check(asm) == []
    names = list(ci.kernel_bodies(asm))
    assert len(names) == 3
    stream = next(n for n in names if "modgpu_cycle_rekey_verify_table_kernel" in n)
    plan = next(n for n in names if "modgpu_cycle_rekey_verify_table_plan" in n)
    at = asm.index(stream + ":")

    def in_stream(old, new):
        i = asm.index(old, at)
        return asm[:i] + new + asm[i + len(old):]

    def meta(name, field, value):
        m = asm.index("amdhsa.kernels")
        rec = asm.index(".name:           " + name + "\n", m)
        start = asm.rfind("  - .agpr_count", m, rec)
        i = asm.index("." + field + ":", start)
        j = asm.index("\n", i)
        return asm[:i] + "." + field + ":" + " " * 6 + str(value) + asm[j:]

    def in_plan(new):  # right behind the plan kernel's label line
        i = asm.index("\n", asm.index("\n" + plan + ":")) + 1
        i = asm.index("\n", i) + 1
        return asm[:i] + new + asm[i:]

    one_block = next(x for x in ci.BLOCK.findall(asm[at:]) if "s[94:95]" in x)  # a ninth one, as the compiler wrote it
    cases = {
        "register counts beyond the budget": meta(stream, "vgpr_count", 129),
        "spills, scratch or a private segment": meta(stream, "vgpr_spill_count", 2),
        "private segment": meta(stream, "private_segment_fixed_size", 40),
        "holds another kernel": asm.replace(plan, plan.replace("table_plan", "table_other")),
        "holds 0 modgpu_cycle_rekey_verify_table_plan, expected 1": asm.replace("\n" + plan + ":", "\nno" + plan + ":"),
        "a planning kernel carries a keystream block": in_plan("\t;;#ASMSTART\n" + one_block + ";;#ASMEND\n"),
        "a data load is not nt": in_stream(" offen nt\n", " offen\n"),
        "the atomic optimizer rewrote": in_stream("\ts_barrier\n", "\tv_mbcnt_lo_u32_b32 v1, -1, 0\n\ts_barrier\n"),
        "touched OUTSIDE the blocks": in_stream("\ts_barrier\n", "\tv_mov_b32_e32 v113, 0\n\ts_barrier\n"),
        "gave a two-keystream block operand a fixed temporary": in_stream("v_addc_co_u32_sdwa v", "v_addc_co_u32_sdwa v119, vcc, v125, v"),
        "a two-keystream block does not end with s_nop 0": in_stream("\ts_nop 0\n\t\n\t;;#ASMEND", "\t\n\t;;#ASMEND"),
        "is not 60 mads + 30 addc": in_stream("\tv_addc_co_u32_sdwa", "\tv_add_co_u32_sdwa"),
        "three-input XORs": in_stream(" bitop3:0x96", " bitop3:0x69"),
        "two-keystream blocks, expected 8": in_stream("\ts_barrier\n", "\t;;#ASMSTART\n" + one_block + ";;#ASMEND\n\ts_barrier\n"),
        "the entry search is not scalar": in_stream("\ts_barrier\n", "\tglobal_load_dword v1, v[2:3], off\n\tglobal_load_dword v1, v[2:3], off\n"
                                                   "\tglobal_load_dword v1, v[2:3], off\n\ts_barrier\n"),
        "a rekey verify kernel stores": in_stream("\ts_barrier\n", "\tglobal_store_dword v1, v2, s[2:3]\n\ts_barrier\n"),
        "stores through a buffer descriptor or a pointer": in_stream("\ts_barrier\n", "\tbuffer_store_dwordx4 v[0:3], v4, s[8:11], 0 offen nt sc1\n\ts_barrier\n"),
        "buffer atomics or flat_ accesses": in_stream("\ts_barrier\n", "\tbuffer_atomic_add_x2 v[0:1], v4, s[8:11], 0 offen\n\ts_barrier\n"),
        "flat_ accesses": in_stream("\ts_barrier\n", "\tflat_load_dword v1, v[2:3]\n\ts_barrier\n"),
        "32-bit global_atomic_add": in_stream(" sc0\n", "\n"),
        "result atomics": in_stream("global_atomic_umin_x2", "global_atomic_umax_x2"),
        "can be reached with part of the wave masked off": in_stream("\ts_barrier\n", "\ts_and_saveexec_b64 s[90:91], vcc\n\ts_barrier\n"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])
