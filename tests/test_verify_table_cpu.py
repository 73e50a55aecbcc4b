"""CPU checks of the verify table call (modgpu_verify_table_device & co., include/modgpu.h): the workspace size, the refusal without a
device, the new TU's source list and hash, its code-generation guard, a broken build the guard must reject, the stand-in's wiring, and
the host code under ASan/UBSan and TSan against the CPU stand-in of the HIP runtime."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
VERIFY_TABLE_SRC = ("cycle_verify_table_kernel.hip", "cycle_table_impl.h", "cycle_verify_table_kernel.h", "cycle_table_kernel.h", "cycle_verify_kernel.h",
                    "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h")
MAX_ENTRIES = 1 << 22  # MODGPU_TABLE_MAX_ENTRIES


def test_workspace_size(modgpu):
    w = modgpu.verify_table_workspace_bytes
    assert w(0) == 0 and w(MAX_ENTRIES + 1) == 0 and w(MAX_ENTRIES) > 0
    sizes = [w(n) for n in (1, 2, 15, 16, 17, 255, 256, 257, 1000, 1024, 1025, 4096, 65536, 100000, MAX_ENTRIES)]
    assert sizes == sorted(sizes)
    for n in (1, 16, 17, 1000, 100000, MAX_ENTRIES):
        assert w(n) >= modgpu.table_workspace_bytes(n) + 64 and w(n) % 64 == 0, n


def test_without_a_gpu_the_call_fails_with_no_device(modgpu):
    """Tier 1 comes first (MODGPU_ERR_INVALID, nothing queued); a well-formed call gets as far as the device and fails there."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    t, r, ws = np.zeros(64, np.uint64), np.zeros(64, np.uint64), np.zeros(4096, np.uint64)
    wb = modgpu.verify_table_workspace_bytes(3)
    before = modgpu.path_stats()
    assert L.modgpu_verify_table_device(t.ctypes.data, 3, None, ws.ctypes.data, wb, -1, None) == 1
    assert L.modgpu_verify_table_device(t.ctypes.data, 3, r.ctypes.data + 4, ws.ctypes.data, wb, -1, None) == 1
    assert L.modgpu_verify_table_device(t.ctypes.data, 3, r.ctypes.data, ws.ctypes.data, wb - 1, -1, None) == 1
    assert L.modgpu_verify_table_device(None, 0, None, None, 0, -1, None) == 0
    assert L.modgpu_verify_table_device(t.ctypes.data, 3, r.ctypes.data, ws.ctypes.data, wb, -1, None) == 2  # MODGPU_ERR_NO_DEVICE
    out = np.zeros(4, np.uint64)
    assert L.modgpu_verify_table_summary(ws.ctypes.data, -1, out.ctypes.data) == 2
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] and st["scalar_calls"] == before["scalar_calls"]


def test_source_list_and_hash(modgpu):
    assert tuple(B.make_var("VERIFY_TABLE_SRC").split()) == VERIFY_TABLE_SRC
    h = hashlib.sha256()
    for f in VERIFY_TABLE_SRC:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    assert modgpu.verify_table_kernel_source_hash() == h.hexdigest()
    assert len({modgpu.verify_table_kernel_source_hash(), modgpu.verify_kernel_source_hash(), modgpu.table_kernel_source_hash()}) == 3


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-verify-table` passes the tree (3 kernels); the TU with a store of the difference in the stream loop is REJECTED;
    the object waits for its own guard run, which ISA_CHECK=0 leaves out; the TU is built with the atomic-optimizer flag; the stand-in
    is wired."""
    B.isa_check_target("isa-check-verify-table", 3)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-verify-table"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a verify table stream kernel that stores"
    assert "a verify kernel stores through a buffer descriptor" in broken.stdout, broken.stdout[-3000:]
    B.standin_is_wired("standin_launch_verify_table.cpp")
    plan = B.dry_run("all")
    flag = "-amdgpu-atomic-optimizer-strategy=None"
    for step in ("-S --cuda-device-only", "-c"):
        lines = [ln for ln in plan if f" {step} cycle_verify_table_kernel.hip " in ln]
        assert len(lines) == 1 and f" -mllvm {flag} " in lines[0], (step, lines)
    for link in [ln for ln in plan if " -shared " in ln and "libmodgpu" in ln and "libmodulate_host" not in ln]:
        assert " cycle_verify_table_kernel.o " in link, link
    B.guard_then_compile("cycle_verify_table_kernel")
    B.unguarded_plan("cycle_verify_table_kernel")


def test_codegen_guard_rules_on_altered_assembly():
    """Rules of the verify table branch of check_isa.check() on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_verify_table_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_verify_table_kernel.s")).read()
    assert ci.check(asm) == []
    names = list(ci.kernel_bodies(asm))
    assert len(names) == 3
    stream = next(n for n in names if "modgpu_cycle_verify_table_kernel" in n)
    at = asm.index(stream + ":")

    def in_stream(old, new):
        i = asm.index(old, at)
        return asm[:i] + new + asm[i + len(old):]

    cases = {
        "a data load is not nt": in_stream(" offen nt\n", " offen\n"),
        "the atomic optimizer rewrote": in_stream("\ts_barrier\n", "\tv_mbcnt_lo_u32_b32 v1, -1, 0\n\ts_barrier\n"),
        "touched OUTSIDE the keystream blocks": in_stream("\ts_barrier\n", "\tv_mov_b32_e32 v121, 0\n\ts_barrier\n"),
        "the entry search is not scalar": in_stream("\ts_barrier\n", "\tglobal_load_dword v1, v[2:3], off\n\tglobal_load_dword v1, v[2:3], off\n"
                                                   "\tglobal_load_dword v1, v[2:3], off\n\ts_barrier\n"),
        "a verify kernel stores": in_stream("\ts_barrier\n", "\tglobal_store_dword v1, v2, s[2:3]\n\ts_barrier\n"),
        "32-bit global_atomic_add": in_stream(" sc0\n", "\n"),
        "result atomics": in_stream("global_atomic_umin_x2", "global_atomic_umax_x2"),
        "does not end with s_nop 0": in_stream("\ts_nop 0\n\t\n\t;;#ASMEND", "\t\n\t;;#ASMEND"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_verify_table_host_code_under_asan_ubsan():
    B.run_sanitized_cases("san_verify_table_cases.py", "asan", "5 passed")


def test_verify_table_host_code_under_tsan():
    B.run_sanitized_cases("san_verify_table_cases.py", "tsan", "5 passed")
