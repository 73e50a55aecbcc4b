"""CPU checks of the verify entry points (modgpu_verify_device / modgpu_verify_batch_device / modgpu_verify_results,
include/modgpu.h): the symbols are declared, exported and listed, the new TU has a source hash of its own, argument validation happens
before any device work, the TU's code-generation guard passes the tree and rejects a broken build and hand-made faults, and the host
code runs clean under ASan/UBSan and TSan against the CPU stand-in of the HIP runtime."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
PUBLIC = ("modgpu_verify_device", "modgpu_verify_batch_device", "modgpu_verify_results")
TESTING = ("modgpu_time_verify_device", "modgpu_verify_kernel_source_hash")
VERIFY_SRC = ("cycle_verify_kernel.hip", "cycle_verify_kernel.h", "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h")


def test_new_symbols_declared_exported_and_listed(modgpu):
    public = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    testing = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    for name in PUBLIC:
        assert re.search(r"\bint %s\(" % name, public), name
    assert re.search(r"typedef struct modgpu_verify_result \{\s*uint64_t mismatches;[^}]*uint64_t first_mismatch;[^}]*uint64_t n;[^}]*"
                     r"uint64_t reserved;[^}]*\} modgpu_verify_result_t;", public)
    assert re.search(r"\bint modgpu_time_verify_device\(", testing) and "modgpu_verify_kernel_source_hash(void);" in testing
    assert "void modgpu_debug_set_verify_form(int grid);" in testing
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(PUBLIC + TESTING) <= names, (flavour, set(PUBLIC + TESTING) - names)
        assert ("modgpu_debug_set_verify_form" in names) == (flavour == "testing")
    assert set(PUBLIC) <= set(modgpu.EXPORTS) and set(TESTING) <= set(modgpu.TESTING_EXPORTS)
    assert "modgpu_debug_set_verify_form" in modgpu.DEBUG_EXPORTS
    assert modgpu.VERIFY_RESULT_DTYPE.itemsize == 32 and modgpu.VERIFY_RESULT_DTYPE.names == ("mismatches", "first_mismatch", "n", "reserved")
    assert modgpu.lib().modgpu_abi_version() == 8


def test_verify_kernel_source_hash_matches_its_sources(modgpu):
    h = hashlib.sha256()
    for f in VERIFY_SRC:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    assert modgpu.verify_kernel_source_hash() == h.hexdigest()
    assert len({modgpu.verify_kernel_source_hash(), modgpu.kernel_source_hash(), modgpu.feed_kernel_source_hash(),
                modgpu.to_kernel_source_hash(), modgpu.xfer_kernel_source_hash(), modgpu.rekey_kernel_source_hash(),
                modgpu.table_kernel_source_hash(), modgpu.rekey_table_kernel_source_hash()}) == 8


def test_validation_comes_before_the_device(modgpu):
    """Without a GPU: a NULL expect / src with n > 0, a NULL or misaligned result, a negative count and NULL arrays are
    MODGPU_ERR_INVALID (checked before any device work); every valid call -- n == 0, aliased and overlapping inputs, degenerate keys --
    is MODGPU_ERR_NO_DEVICE: nothing is computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    b = np.arange(256, dtype=np.uint8)
    keep = b.copy()
    r = np.zeros(8, dtype=modgpu.VERIFY_RESULT_DTYPE)
    before = modgpu.path_stats()
    p, q = b.ctypes.data, r.ctypes.data
    K3, K4 = modgpu.KEY_PS3, modgpu.KEY_PS4

    def code(fn, *args, **kw):
        with pytest.raises(modgpu.ModGpuError) as e:
            fn(*args, **kw)
        return e.value.code

    vd, vb = modgpu.verify_device, modgpu.verify_batch_device
    assert code(vd, 0, p, K3, result=q, n=10) == 1
    assert code(vd, p, 0, K3, result=q, n=10) == 1
    assert code(vd, p, p + 100, K3, result=q + 4, n=10) == 1   # misaligned result
    assert code(vd, p, p + 100, K3, result=q + 1, n=0) == 1    # ... with nothing to compare, too
    L = modgpu.lib()
    assert L.modgpu_verify_device(p, p + 100, 10, 1, 0, None, -1, None) == 1   # NULL result
    assert L.modgpu_verify_device(p, p + 100, 0, 1, 0, None, -1, None) == 1
    assert code(vb, [p, 0], [p + 100, p + 120], [10, 10], K3, q) == 1
    assert code(vb, [p, p], [p + 100, 0], [10, 10], K3, q) == 1
    assert code(vb, [p, p], [p + 100, p], [10, 10], K3, 0) == 1                # NULL results
    assert L.modgpu_verify_batch_device(None, None, None, None, 2, 1, q, -1, None) == 1
    assert L.modgpu_verify_batch_device(None, None, None, None, -1, 1, q, -1, None) == 1
    assert code(modgpu.time_verify_device, p, p + 100, 10, K3, q + 4) == 1
    assert L.modgpu_verify_results(None, 1, -1, q) == 1 and L.modgpu_verify_results(q, 1, -1, None) == 1
    # valid: disjoint, exact alias, partial overlap, n == 0, NULL buffers with n == 0, overlapping entries, empty entries, degenerate
    # keys, NULL offsets, an empty batch
    assert code(vd, p, p + 100, K3, 1 << 40, result=q, n=10) == 2
    assert code(vd, p, p, K3, result=q, n=10) == 2
    assert code(vd, p + 1, p, K3, result=q, n=10) == 2
    assert code(vd, p, p + 9, K3, 3, result=q, n=10) == 2
    assert code(vd, p, p + 100, K3, result=q, n=0) == 2
    assert code(vd, 0, 0, K3, result=q, n=0) == 2
    for k in (0, 0x7FFFFFFF, 0x80000001):
        assert code(vd, p, p + 100, k, 4, result=q, n=10) == 2
    assert code(vb, [p, p + 5, p + 5], [p + 100, p + 5, p], [10, 10, 0], K4, q, stream_offs=[0, 5, 7]) == 2
    assert code(vb, [p, 0], [p + 100, 0], [10, 0], K3, q) == 2
    assert code(vb, [], [], [], K3, 0) == 2
    assert code(modgpu.time_verify_device, p, p + 100, 10, K3, q) == 2
    assert code(modgpu.verify_results, q, 1) == 2
    assert np.array_equal(b, keep) and not r.view(np.uint8).any()
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] == 0 and st["scalar_calls"] == before["scalar_calls"]


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-verify` is the TU's own pass (5 kernels: the init kernel and four forms); the TU with a store in its stream
    loop is REJECTED by name; the object waits for its own guard run, which ISA_CHECK=0 leaves out; the stand-in is wired.
    (`make isa-check` as a whole: tests/test_capi_cpu.py.)"""
    B.isa_check_target("isa-check-verify", 5)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-verify"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a verify kernel that stores in its stream loop"
    assert "a verify kernel stores through a buffer descriptor" in broken.stdout, broken.stdout[-3000:]
    B.guard_then_compile("cycle_verify_kernel")
    B.unguarded_plan("cycle_verify_kernel")
    B.standin_is_wired("standin_launch_verify.cpp")
    assert tuple(B.make_var("VERIFY_SRC").split()) == VERIFY_SRC


def test_codegen_guard_rules_on_altered_assembly():
    """Each rule of the verify branch of check_isa.check() on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_verify_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_verify_kernel.s")).read()
    assert ci.check(asm) == []
    names = list(ci.kernel_bodies(asm))
    assert len(names) == 5 and sum(n.startswith("_Z26modgpu_cycle_verify_kernel") for n in names) == 4
    keyed = next(n for n in names if n.endswith("Lb0ELb1EEv15CycleVerifyArgs"))
    ident = next(n for n in names if n.endswith("Lb0ELb0EEv15CycleVerifyArgs"))
    init = next(n for n in names if "modgpu_cycle_verify_init" in n)

    def in_kernel(name, old, new):
        i = asm.index(old, asm.index(name + ":"))
        assert i < asm.index("s_endpgm", asm.index(name + ":")), (name, old)
        return asm[:i] + new + asm[i + len(old):]

    def meta(name, field, value):
        m = asm.index("amdhsa.kernels")
        rec = asm.index(".name:           " + name + "\n", m)
        start = asm.rfind("  - .agpr_count", m, rec)
        i = asm.index("." + field + ":", start)
        j = asm.index("\n", i)
        return asm[:i] + "." + field + ":" + " " * 6 + str(value) + asm[j:]

    one_block = next(x for x in ci.BLOCK.findall(asm[asm.index(keyed + ":"):]) if "s[94:95]" in x)  # a tenth one, as the compiler wrote it
    store = "\tbuffer_store_dwordx4 v[0:3], v4, s[8:11], 0 offen nt sc1\n\ts_barrier\n"
    cases = {
        "register counts beyond the budget": meta(keyed, "vgpr_count", 129),
        "spills, scratch or a private segment": meta(keyed, "vgpr_spill_count", 2),
        "a verify kernel stores through a buffer descriptor": in_kernel(keyed, "\ts_barrier\n", store),
        "flat_ accesses": in_kernel(keyed, "\ts_barrier\n", "\tflat_load_dword v1, v[2:3]\n\ts_barrier\n"),
        "a data load is not nt": in_kernel(keyed, " offen nt\n", " offen\n"),
        "a keystream block does not end with s_nop 0": in_kernel(keyed, "\ts_nop 0\n\t\n\t;;#ASMEND", "\t\n\t;;#ASMEND"),
        "is not 30 mads + 15 addc": in_kernel(keyed, "\tv_addc_co_u32_sdwa", "\tv_add_co_u32_sdwa"),
        "touched OUTSIDE the keystream blocks": in_kernel(keyed, "\ts_barrier\n", "\tv_mov_b32_e32 v121, 0\n\ts_barrier\n"),
        "keystream blocks, expected 9": in_kernel(keyed, "\ts_barrier\n", "\t;;#ASMSTART\n" + one_block + ";;#ASMEND\n\ts_barrier\n"),
        "expected the one global_store_dwordx2": in_kernel(keyed, "\ts_barrier\n", "\tglobal_store_dword v1, v2, s[0:1]\n\ts_barrier\n"),
        "result atomics": in_kernel(keyed, "\tglobal_atomic_umin_x2", "\tglobal_atomic_smin_x2"),
        "LDS is 24 bytes": meta(keyed, "group_segment_fixed_size", 24),
        "an identity form carries a keystream block": in_kernel(
            ident, "\ts_barrier\n", "\t;;#ASMSTART\n\tv_mad_u64_u32 v[120:121], s[94:95], v1, s4, v[2:3]\n\ts_nop 0\n\t;;#ASMEND\n\ts_barrier\n"),
        "the init kernel does something other than store": in_kernel(init, "\tglobal_store_dword", "\tglobal_load_dword v1, v2, s[0:1]\n\tglobal_store_dword"),
        "expected 1 and 4": asm.replace(init, init.replace("verify_init", "verify_kernel")),
        "can be reached with part of the wave masked off": in_kernel(keyed, "\ts_barrier\n", "\ts_and_saveexec_b64 s[90:91], vcc\n\ts_barrier\n"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_verify_host_code_under_asan_ubsan():
    B.run_sanitized_cases("san_verify_cases.py", "asan", "5 passed")


def test_verify_host_code_under_tsan():
    B.run_sanitized_cases("san_verify_cases.py", "tsan", "5 passed")
