"""CPU checks of the out-of-place entry points (modgpu_cycle_device_to / modgpu_cycle_batch_device_to, include/modgpu.h): the
symbols are in both library flavours, argument validation happens before any device work, the new TU's code-generation guard
passes the tree and rejects a broken build and hand-made faults, and the host code runs clean under ASan/UBSan and TSan against
the CPU stand-in of the HIP runtime."""
import os
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
NEW = ("modgpu_cycle_device_to", "modgpu_cycle_batch_device_to", "modgpu_time_cycle_device_to", "modgpu_to_kernel_source_hash")


def test_new_symbols_in_both_flavours(modgpu):
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
        assert ("modgpu_debug_set_to_form" in names) == (flavour == "testing")
    assert set(NEW[:2]) <= set(modgpu.EXPORTS) and set(NEW[2:]) <= set(modgpu.TESTING_EXPORTS)
    assert modgpu.lib().modgpu_abi_version() == 8


def test_to_kernel_source_hash_matches_its_sources(modgpu):
    import hashlib
    h = hashlib.sha256()
    for f in ("cycle_to_kernel.hip", "cycle_to_kernel.h", "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    assert modgpu.to_kernel_source_hash() == h.hexdigest()
    assert len({modgpu.to_kernel_source_hash(), modgpu.kernel_source_hash(), modgpu.feed_kernel_source_hash()}) == 3


def test_validation_comes_before_the_device(modgpu):
    """Without a GPU: a null pointer with bytes to move, a partial overlap and a batch overlap are MODGPU_ERR_INVALID (checked
    before any device work); every valid call is MODGPU_ERR_NO_DEVICE -- nothing is computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    b = np.arange(256, dtype=np.uint8)
    keep = b.copy()
    before = modgpu.path_stats()
    p = b.ctypes.data

    def code(fn, *args, **kw):
        with pytest.raises(modgpu.ModGpuError) as e:
            fn(*args, **kw)
        return e.value.code

    assert code(modgpu.cycle_device_to, 0, p, 10, 1) == 1
    assert code(modgpu.cycle_device_to, p, 0, 10, 1) == 1
    for d, s in ((p + 1, p), (p, p + 1), (p + 9, p), (p, p + 9)):  # partial overlaps, down to one byte
        assert code(modgpu.cycle_device_to, d, s, 10, 1) == 1
    assert code(modgpu.cycle_batch_device_to, [p, p + 20], [p + 100, p + 25], [10, 10], 1) == 1   # entry 1 partly overlaps its own source
    assert code(modgpu.cycle_batch_device_to, [p, p + 5], [p + 100, p + 120], [10, 10], 1) == 1   # two destinations meet
    assert code(modgpu.cycle_batch_device_to, [p, p + 20], [p + 20, p + 40], [10, 10], 1) == 1    # dst 1 == src 0 of another entry
    assert code(modgpu.cycle_batch_device_to, [p, 0], [p + 100, p + 120], [10, 10], 1) == 1
    # valid: exact alias, disjoint, n == 0, null with n == 0, overlapping SOURCES, empty batch entries, zero-residue key
    assert code(modgpu.cycle_device_to, p, p, 10, 1) == 2
    assert code(modgpu.cycle_device_to, p + 100, p, 10, 1) == 2
    assert code(modgpu.cycle_device_to, p + 100, p, 0, 1) == 2
    assert code(modgpu.cycle_device_to, 0, 0, 0, 1) == 2
    assert code(modgpu.cycle_device_to, p + 100, p, 10, 0x7FFFFFFF) == 2
    assert code(modgpu.cycle_batch_device_to, [p + 100, p + 120, p + 140], [p, p + 5, p + 5], [10, 10, 0], 1, stream_offs=[0, 5, 7]) == 2
    assert code(modgpu.cycle_batch_device_to, [p + 100, 0], [p, 0], [10, 0], 1) == 2
    assert code(modgpu.time_cycle_device_to, p + 100, p, 10, 1) == 2
    assert np.array_equal(b, keep)
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] == 0 and st["scalar_calls"] == before["scalar_calls"]


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-to` is the guard's pass over the out-of-place TU (2 kernels); the same TU built without
    -amdgpu-atomic-optimizer-strategy=None is REJECTED; the object waits for its own guard run, which ISA_CHECK=0 leaves out.
    (`make isa-check` as a whole: tests/test_capi_cpu.py.)"""
    B.isa_check_target("isa-check-to", 2)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-to"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted an out-of-place kernel whose ticket atomic is wave-aggregated"
    assert "the atomic optimizer rewrote the ticket atomic" in broken.stdout, broken.stdout[-3000:]
    B.guard_then_compile("cycle_to_kernel")
    B.unguarded_plan("cycle_to_kernel")


def test_codegen_guard_rules_on_altered_assembly():
    """Each rule of the out-of-place branch of check_isa.check() on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_to_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_to_kernel.s")).read()
    assert ci.check(asm) == []
    names = list(ci.kernel_bodies(asm))
    assert len(names) == 2 and all(n.startswith("_Z22modgpu_cycle_to_kernel") for n in names)
    assert not any(s in n for n in names for s in ("modgpu_cycle_feed_kernel", "modgpu_cycle_queue_kernel", "modgpu_cycle_kernelILi1ELi256E"))
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
        "does not end with s_nop 0": in_first("\ts_nop 0\n\t\n\t;;#ASMEND", "\t\n\t;;#ASMEND"),
        "is not 30 mads + 15 addc": in_first("\tv_addc_co_u32_sdwa", "\tv_add_co_u32_sdwa"),
        "a fixed temporary is touched OUTSIDE the keystream blocks": in_first("\ts_barrier\n", "\tv_mov_b32_e32 v121, 0\n\ts_barrier\n"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_out_of_place_host_code_under_asan_ubsan():
    B.run_sanitized_cases("san_to_cases.py", "asan", "6 passed")


def test_out_of_place_host_code_under_tsan():
    B.run_sanitized_cases("san_to_cases.py", "tsan", "6 passed")
