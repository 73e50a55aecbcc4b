"""CPU checks of the rekey verify entry points (modgpu_verify_rekey_device / modgpu_verify_rekey_batch_device, include/modgpu.h): the
symbols are declared, exported and listed, the new TU has a source hash of its own, argument validation happens before any device work,
the TU's code-generation guard passes the tree and rejects a broken build and hand-made faults, and the host code runs clean under
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
PUBLIC = ("modgpu_verify_rekey_device", "modgpu_verify_rekey_batch_device")
TESTING = ("modgpu_time_verify_rekey_device", "modgpu_rekey_verify_kernel_source_hash")
REKEY_VERIFY_SRC = ("cycle_rekey_verify_kernel.hip", "cycle_rekey_verify_kernel.h", "cycle_verify_kernel.h", "cycle_rekey_impl.h",
                    "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h")


def test_new_symbols_declared_exported_and_listed(modgpu):
    public = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    testing = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    for name in PUBLIC:
        assert re.search(r"\bint %s\(" % name, public), name
    assert re.search(r"\bint modgpu_time_verify_rekey_device\(", testing) and "modgpu_rekey_verify_kernel_source_hash(void);" in testing
    assert re.search(r"\b12 = the rekey verify call's", testing) and "modgpu_rekey_verify_kernel_source_hash() for variant 12" in testing
    assert "#define MODGPU_ABI_VERSION 8\n" in public
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(PUBLIC + TESTING) <= names, (flavour, set(PUBLIC + TESTING) - names)
    assert set(PUBLIC) <= set(modgpu.EXPORTS) and set(TESTING) <= set(modgpu.TESTING_EXPORTS)
    for name in ("verify_rekey_device", "verify_rekey_batch_device", "time_verify_rekey_device", "rekey_verify_kernel_source_hash"):
        assert callable(getattr(modgpu, name)), name
    assert modgpu.lib().modgpu_abi_version() == 8


def test_rekey_verify_kernel_source_hash_matches_its_sources(modgpu):
    h = hashlib.sha256()
    for f in REKEY_VERIFY_SRC:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    assert modgpu.rekey_verify_kernel_source_hash() == h.hexdigest()
    assert len({modgpu.rekey_verify_kernel_source_hash(), modgpu.verify_kernel_source_hash(), modgpu.kernel_source_hash(),
                modgpu.feed_kernel_source_hash(), modgpu.to_kernel_source_hash(), modgpu.xfer_kernel_source_hash(),
                modgpu.rekey_kernel_source_hash(), modgpu.table_kernel_source_hash(), modgpu.rekey_table_kernel_source_hash(),
                modgpu.verify_table_kernel_source_hash()}) == 10


def test_validation_comes_before_the_device(modgpu):
    """Without a GPU: a NULL expect / src with n > 0, a NULL or misaligned result, an entry of 2^24 chunks or more, a negative count and
    NULL arrays are MODGPU_ERR_INVALID (checked before any device work); every valid call -- n == 0, aliased and overlapping inputs,
    degenerate keys, NULL offset arrays, an empty batch -- is MODGPU_ERR_NO_DEVICE: nothing is computed on the host."""
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

    vd, vb = modgpu.verify_rekey_device, modgpu.verify_rekey_batch_device
    assert code(vd, 0, p, K3, K4, result=q, n=10) == 1
    assert code(vd, p, 0, K3, K4, result=q, n=10) == 1
    assert code(vd, p, p + 100, K3, K4, result=q + 4, n=10) == 1   # misaligned result
    assert code(vd, p, p + 100, K3, K4, result=q + 1, n=0) == 1    # ... with nothing to compare, too
    assert code(vd, p, p + 100, 0, 0, result=q + 4, n=10) == 1     # ... and whatever the keys
    assert code(vd, p, p, K3, K4, result=q, n=1 << 40) == 1        # 2^24 chunks of 64 KiB
    L = modgpu.lib()
    assert L.modgpu_verify_rekey_device(p, p + 100, 10, 1, 0, 2, 0, None, -1, None) == 1   # NULL result
    assert L.modgpu_verify_rekey_device(p, p + 100, 0, 1, 0, 2, 0, None, -1, None) == 1
    assert code(vb, [p, 0], [p + 100, p + 120], [10, 10], K3, K4, q) == 1
    assert code(vb, [p, p], [p + 100, 0], [10, 10], K3, K4, q) == 1
    assert code(vb, [p, p], [p + 100, p], [10, 10], K3, K4, 0) == 1                # NULL results
    assert code(vb, [p, p], [p + 100, p], [10, 1 << 40], K3, K4, q) == 1
    assert L.modgpu_verify_rekey_batch_device(None, None, None, None, None, 2, 1, 2, q, -1, None) == 1
    assert L.modgpu_verify_rekey_batch_device(None, None, None, None, None, -1, 1, 2, q, -1, None) == 1
    assert code(modgpu.time_verify_rekey_device, p, p + 100, 10, K3, K4, q + 4) == 1
    assert code(modgpu.time_verify_rekey_device, p, p + 100, 10, K3, K4, q, iters=0) == 1
    # valid: disjoint, exact alias, partial overlap, n == 0, NULL buffers with n == 0, overlapping entries, empty entries, degenerate
    # keys and coinciding streams, NULL offsets, an empty batch
    assert code(vd, p, p + 100, K3, K4, 1 << 40, (1 << 64) - 1, result=q, n=10) == 2
    assert code(vd, p, p, K3, K4, result=q, n=10) == 2
    assert code(vd, p + 1, p, K3, K4, result=q, n=10) == 2
    assert code(vd, p, p + 9, K3, K4, 3, 4, result=q, n=10) == 2
    assert code(vd, p, p + 100, K3, K4, result=q, n=0) == 2
    assert code(vd, 0, 0, K3, K4, result=q, n=0) == 2
    for k in (0, 0x7FFFFFFF, 0x80000001):
        assert code(vd, p, p + 100, k, K4, 4, 5, result=q, n=10) == 2
        assert code(vd, p, p + 100, K3, k, 4, 5, result=q, n=10) == 2
        assert code(vd, p, p + 100, k, 0, 4, 5, result=q, n=10) == 2
    assert code(vd, p, p + 100, K4, K4, 7, 7 + (1 << 31) - 2, result=q, n=10) == 2
    assert code(vb, [p, p + 5, p + 5], [p + 100, p + 5, p], [10, 10, 0], K4, K4, q, offs_from=[0, 5, 7], offs_to=[0, 6, 7]) == 2
    assert code(vb, [p, p + 5], [p + 100, p + 5], [10, 10], K3, K4, q, offs_from=[0, 5]) == 2
    assert code(vb, [p, 0], [p + 100, 0], [10, 0], K3, K4, q) == 2
    assert code(vb, [], [], [], K3, K4, 0) == 2
    assert code(modgpu.time_verify_rekey_device, p, p + 100, 10, K3, K4, q) == 2
    assert np.array_equal(b, keep) and not r.view(np.uint8).any()
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] == 0 and st["scalar_calls"] == before["scalar_calls"]


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-rekey-verify` is the TU's own pass (2 kernels: plain and funnel); the TU with a store in its stream loop is
    REJECTED by name; the object waits for its own guard run, which ISA_CHECK=0 leaves out; the stand-in is wired; the TU is built
    without the atomic-optimizer flag (it has no ticket)."""
    B.isa_check_target("isa-check-rekey-verify", 2)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-rekey-verify"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a rekey verify kernel that stores in its stream loop"
    assert "a rekey verify kernel stores through a buffer descriptor" in broken.stdout, broken.stdout[-3000:]
    B.guard_then_compile("cycle_rekey_verify_kernel")
    B.unguarded_plan("cycle_rekey_verify_kernel")
    B.standin_is_wired("standin_launch_rekey_verify.cpp")
    assert tuple(B.make_var("REKEY_VERIFY_SRC").split()) == REKEY_VERIFY_SRC
    assert "cycle_rekey_verify_kernel.h" in B.make_var("CAPI_HDR").split()
    plan = B.dry_run("all")
    for step in ("-S --cuda-device-only", "-c"):
        lines = [ln for ln in plan if f" {step} cycle_rekey_verify_kernel.hip " in ln]
        assert len(lines) == 1 and "-amdgpu-atomic-optimizer-strategy" not in lines[0], (step, lines)
    assert sum("cycle_rekey_verify_kernel.o" in ln for ln in plan if " -shared " in ln and "libmodgpu" in ln) == 2  # both link lines


def test_codegen_guard_rules_on_altered_assembly():
    """Each rule of the rekey verify branch of check_isa.check() on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_rekey_verify_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_rekey_verify_kernel.s")).read()
    assert ci.check(asm) == []
    names = list(ci.kernel_bodies(asm))
    assert len(names) == 2 and all(n.startswith("_Z32modgpu_cycle_rekey_verify_kernel") for n in names)
    plain = next(n for n in names if n.endswith("Lb0EEv20CycleRekeyVerifyArgs"))
    funnel = next(n for n in names if n.endswith("Lb1EEv20CycleRekeyVerifyArgs"))

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

    one_block = next(x for x in ci.BLOCK.findall(asm[asm.index(plain + ":"):]) if "s[94:95]" in x)  # a tenth one, as the compiler wrote it
    store = "\tbuffer_store_dwordx4 v[0:3], v4, s[8:11], 0 offen nt sc1\n\ts_barrier\n"
    cases = {
        "register counts beyond the budget": meta(plain, "vgpr_count", 129),
        "spills, scratch or a private segment": meta(funnel, "vgpr_spill_count", 2),
        "private segment": meta(plain, "private_segment_fixed_size", 40),
        "a rekey verify kernel stores through a buffer descriptor": in_kernel(plain, "\ts_barrier\n", store),
        "stores through a buffer descriptor (": in_kernel(funnel, "\ts_barrier\n", "\tbuffer_atomic_add_x2 v[0:1], v4, s[8:11], 0 offen\n\ts_barrier\n"),
        "flat_ accesses": in_kernel(plain, "\ts_barrier\n", "\tflat_load_dword v1, v[2:3]\n\ts_barrier\n"),
        "a data load is not nt": in_kernel(funnel, " offen nt\n", " offen\n"),
        "a two-keystream block does not end with s_nop 0": in_kernel(plain, "\ts_nop 0\n\t\n\t;;#ASMEND", "\t\n\t;;#ASMEND"),
        "is not 60 mads + 30 addc": in_kernel(plain, "\tv_addc_co_u32_sdwa", "\tv_add_co_u32_sdwa"),
        "touched OUTSIDE the blocks": in_kernel(plain, "\ts_barrier\n", "\tv_mov_b32_e32 v113, 0\n\ts_barrier\n"),
        "gave a two-keystream block operand a fixed temporary": in_kernel(plain, "v_addc_co_u32_sdwa v", "v_addc_co_u32_sdwa v119, vcc, v125, v"),
        "three-input XORs": in_kernel(plain, " bitop3:0x96", " bitop3:0x69"),
        "two-keystream blocks, expected 9": in_kernel(plain, "\ts_barrier\n", "\t;;#ASMSTART\n" + one_block + ";;#ASMEND\n\ts_barrier\n"),
        "expected the one global_store_dwordx2": in_kernel(plain, "\ts_barrier\n", "\tglobal_store_dword v1, v2, s[0:1]\n\ts_barrier\n"),
        "result atomics": in_kernel(funnel, "\tglobal_atomic_umin_x2", "\tglobal_atomic_smin_x2"),
        "LDS is 24 bytes": meta(plain, "group_segment_fixed_size", 24),
        "holds another kernel": asm.replace(funnel, funnel.replace("rekey_verify_kernel", "rekey_verify_other0")),
        "holds 1 kernels, expected 2": asm.replace("\n" + funnel + ":", "\nno" + funnel + ":"),
        "can be reached with part of the wave masked off": in_kernel(plain, "\ts_barrier\n", "\ts_and_saveexec_b64 s[90:91], vcc\n\ts_barrier\n"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_rekey_verify_host_code_under_asan_ubsan():
    B.run_sanitized_cases("san_rekey_verify_cases.py", "asan", "5 passed")


def test_rekey_verify_host_code_under_tsan():
    B.run_sanitized_cases("san_rekey_verify_cases.py", "tsan", "5 passed")
