"""CPU checks of the rekey entry points (modgpu_rekey_device_to / modgpu_rekey_batch_device_to, include/modgpu.h): the symbols are
declared, exported and listed, the new TU has a source hash of its own, argument validation happens before any device work, the
TU's code-generation guard passes the tree and rejects a broken build and hand-made faults, and the host code runs clean under
ASan/UBSan and TSan against the CPU stand-in of the HIP runtime."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
NEW = ("modgpu_rekey_device_to", "modgpu_rekey_batch_device_to", "modgpu_time_rekey_device_to", "modgpu_rekey_kernel_source_hash")
REKEY_SRC = ("cycle_rekey_kernel.hip", "cycle_rekey_kernel.h", "cycle_rekey_impl.h", "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h")


def test_new_symbols_declared_exported_and_listed(modgpu):
    public = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    testing = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    for name in NEW[:2]:
        assert re.search(r"\bint %s\(" % name, public), name
    assert re.search(r"\bint modgpu_time_rekey_device_to\(", testing) and "modgpu_rekey_kernel_source_hash(void);" in testing
    assert "void modgpu_debug_set_rekey_form(int shape);" in testing
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
        assert ("modgpu_debug_set_rekey_form" in names) == (flavour == "testing")
    assert set(NEW[:2]) <= set(modgpu.EXPORTS) and set(NEW[2:]) <= set(modgpu.TESTING_EXPORTS)
    assert "modgpu_debug_set_rekey_form" in modgpu.DEBUG_EXPORTS
    assert modgpu.lib().modgpu_abi_version() == 8


def test_rekey_kernel_source_hash_matches_its_sources(modgpu):
    h = hashlib.sha256()
    for f in REKEY_SRC:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    assert modgpu.rekey_kernel_source_hash() == h.hexdigest()
    assert len({modgpu.rekey_kernel_source_hash(), modgpu.kernel_source_hash(), modgpu.feed_kernel_source_hash(),
                modgpu.to_kernel_source_hash(), modgpu.xfer_kernel_source_hash()}) == 5


def test_validation_comes_before_the_device(modgpu):
    """Without a GPU: NULL with n > 0, a partial overlap and a batch overlap are MODGPU_ERR_INVALID (checked before any device work);
    n == 0 does nothing; every valid call -- degenerate keys included -- is MODGPU_ERR_NO_DEVICE: nothing is computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    b = np.arange(256, dtype=np.uint8)
    keep = b.copy()
    before = modgpu.path_stats()
    p = b.ctypes.data
    K3, K4 = modgpu.KEY_PS3, modgpu.KEY_PS4

    def code(fn, *args, **kw):
        with pytest.raises(modgpu.ModGpuError) as e:
            fn(*args, **kw)
        return e.value.code

    rk, rkb = modgpu.rekey_device_to, modgpu.rekey_batch_device_to
    assert code(rk, 0, p, K3, K4, n=10) == 1
    assert code(rk, p, 0, K3, K4, n=10) == 1
    for d, s in ((p + 1, p), (p, p + 1), (p + 9, p), (p, p + 9)):  # partial overlaps, down to one byte
        assert code(rk, d, s, K3, K4, 3, 5, n=10) == 1
    assert code(rkb, [p, p + 20], [p + 100, p + 25], [10, 10], K3, K4) == 1   # entry 1 partly overlaps its own source
    assert code(rkb, [p, p + 5], [p + 100, p + 120], [10, 10], K3, K4) == 1   # two destinations meet
    assert code(rkb, [p, p + 20], [p + 20, p + 40], [10, 10], K3, K4) == 1    # dst 1 == src 0 of another entry
    assert code(rkb, [p, 0], [p + 100, p + 120], [10, 10], K3, K4) == 1
    L = modgpu.lib()
    assert L.modgpu_rekey_batch_device_to(None, None, None, None, None, 2, 1, 2, -1, None) == 1
    assert L.modgpu_rekey_batch_device_to(None, None, None, None, None, -1, 1, 2, -1, None) == 1
    # valid: exact alias, disjoint, n == 0, null with n == 0, overlapping SOURCES, empty entries, degenerate keys, NULL offsets
    assert code(rk, p, p, K3, K4, n=10) == 2
    assert code(rk, p + 100, p, K3, K4, 1 << 40, 7, n=10) == 2
    assert code(rk, p + 100, p, K3, K4, n=0) == 2
    assert code(rk, 0, 0, K3, K4, n=0) == 2
    for kf, kt in ((0, K4), (K3, 0x7FFFFFFF), (0, 0x80000001), (K3, K3)):
        assert code(rk, p + 100, p, kf, kt, 4, 4, n=10) == 2
    assert code(rkb, [p + 100, p + 120, p + 140], [p, p + 5, p + 5], [10, 10, 0], K3, K4, offs_from=[0, 5, 7], offs_to=[1, 2, 3]) == 2
    assert code(rkb, [p + 100, 0], [p, 0], [10, 0], K3, K4) == 2
    assert code(modgpu.time_rekey_device_to, p + 100, p, 10, K3, K4) == 2
    assert np.array_equal(b, keep)
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] == 0 and st["scalar_calls"] == before["scalar_calls"]


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-rekey` is the guard's pass over the rekey TU (2 kernels); the TU with a block operand pinned into a fixed
    temporary is REJECTED by name; the object waits for its own guard run, which ISA_CHECK=0 leaves out; the stand-in is wired.
    (`make isa-check` as a whole: tests/test_capi_cpu.py.)"""
    B.isa_check_target("isa-check-rekey", 2)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-rekey"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a two-keystream block whose input sits in a fixed temporary"
    assert "the compiler gave a two-keystream block operand a fixed temporary" in broken.stdout, broken.stdout[-3000:]
    B.guard_then_compile("cycle_rekey_kernel")
    B.unguarded_plan("cycle_rekey_kernel")
    B.standin_is_wired("standin_launch_rekey.cpp")
    assert tuple(B.make_var("REKEY_SRC").split()) == REKEY_SRC


def test_codegen_guard_rules_on_altered_assembly():
    """Each rule of the rekey branch of check_isa.check() on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_rekey_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_rekey_kernel.s")).read()
    assert ci.check(asm) == []
    names = list(ci.kernel_bodies(asm))
    assert len(names) == 2 and all(n.startswith("_Z25modgpu_cycle_rekey_kernel") for n in names)
    first = names[0]
    at = asm.index(first + ":")

    def in_first(old, new):
        i = asm.index(old, at)
        return asm[:i] + new + asm[i + len(old):]

    def meta(field, value):
        m = asm.index("amdhsa.kernels")
        rec = asm.index(".name:           " + first + "\n", m)
        start = asm.rfind("  - .agpr_count", m, rec)
        i = asm.index("." + field + ":", start)
        j = asm.index("\n", i)
        return asm[:i] + "." + field + ":" + " " * 6 + str(value) + asm[j:]

    cases = {
        "register counts beyond the budget": meta("vgpr_count", 129),
        "spills, scratch or a private segment": meta("vgpr_spill_count", 2),
        "the atomic optimizer rewrote the ticket atomic": in_first("\ts_barrier\n", "\tv_mbcnt_lo_u32_b32 v1, -1, 0\n\ts_barrier\n"),
        "a data load is not nt": in_first(" offen nt\n", " offen\n"),
        "a data store is not nt sc1": in_first(" offen nt sc1\n", " offen sc1\n"),
        "a two-keystream block does not end with s_nop 0": in_first("\ts_nop 0\n\t\n\t;;#ASMEND", "\t\n\t;;#ASMEND"),
        "is not 60 mads + 30 addc": in_first("\tv_addc_co_u32_sdwa", "\tv_add_co_u32_sdwa"),
        "touched OUTSIDE the blocks": in_first("\ts_barrier\n", "\tv_mov_b32_e32 v113, 0\n\ts_barrier\n"),
        "three-input XORs": in_first("bitop3:0x96", "bitop3:0x69"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_rekey_host_code_under_asan_ubsan():
    B.run_sanitized_cases("san_rekey_cases.py", "asan", "6 passed")


def test_rekey_host_code_under_tsan():
    B.run_sanitized_cases("san_rekey_cases.py", "tsan", "6 passed")
