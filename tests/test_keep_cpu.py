"""CPU checks of the keep kernel's TU and route (cycle_keep_kernel.hip: the work-queue kernel with a resident slice, what a single in-place
buffer of 1 GiB or more is launched on): the TU has a source hash of its own and leaves the main TU's alone, the symbols are declared,
exported and listed, the host's policy for a call's size is the stated arithmetic, the TU's code-generation guard passes the tree and
rejects a broken build and hand-made faults, and the host code runs clean under
ASan/UBSan and TSan against the CPU stand-in of the HIP runtime."""
import hashlib
import os
import re
import subprocess

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
KEEP_SRC = ("cycle_keep_kernel.hip", "cycle_keep_kernel.h", "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h")
MAIN_HASH = "d2832a17dddf0901"
S = 192 << 20  # kKeepBytes: the resident bytes the shipped policy aims at (profiles/r13_keep.json)


def sha(files):
    h = hashlib.sha256()
    for f in files:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()


def test_keep_kernel_source_hash_matches_its_sources_and_the_main_one_is_unchanged(modgpu):
    assert modgpu.keep_kernel_source_hash() == sha(KEEP_SRC)
    assert tuple(B.make_var("KEEP_SRC").split()) == KEEP_SRC
    others = {modgpu.kernel_source_hash(), modgpu.feed_kernel_source_hash(), modgpu.to_kernel_source_hash(), modgpu.xfer_kernel_source_hash(),
              modgpu.rekey_kernel_source_hash(), modgpu.table_kernel_source_hash(), modgpu.rekey_table_kernel_source_hash(),
              modgpu.verify_kernel_source_hash(), modgpu.verify_table_kernel_source_hash(), modgpu.rekey_verify_kernel_source_hash()}
    assert len(others) == 10 and modgpu.keep_kernel_source_hash() not in others
    assert modgpu.kernel_source_hash() == sha(("cycle_kernel_impl.h", "cycle_kernel.hip", "cycle_kernel.h", "lcg.h"))
    assert modgpu.kernel_source_hash().startswith(MAIN_HASH)


def test_new_symbols_declared_exported_and_listed(modgpu):
    testing = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    assert "const char *modgpu_keep_kernel_source_hash(void);" in testing
    assert re.search(r"\bint modgpu_keep_policy\(uint64_t bytes, uint32_t \*mask, uint32_t \*run\);", testing)
    assert re.search(r"\bvoid modgpu_debug_set_keep\(uint64_t min_bytes, uint32_t mask, uint32_t run\);", testing)
    reporting = {"modgpu_keep_kernel_source_hash", "modgpu_keep_policy"}
    assert reporting <= set(modgpu.TESTING_EXPORTS) and "modgpu_debug_set_keep" in modgpu.DEBUG_EXPORTS

    def exported(flavour):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert reporting <= exported("shipped") and "modgpu_debug_set_keep" not in exported("shipped")
    assert reporting | {"modgpu_debug_set_keep"} <= exported("testing")
    for name in ("keep_kernel_source_hash", "keep_policy", "debug_set_keep"):
        assert callable(getattr(modgpu, name)), name
    assert modgpu.lib().modgpu_abi_version() == 8


def test_host_policy_for_a_size(modgpu):
    """run = floor(S / bytes x (mask + 1)) with mask 255 from 1 GiB up: 48 chunks of every 256 at 1 GiB, 12 at 4 GiB, none at 2^40 (S is
    then less than one chunk per period); below 1 GiB the route is off.  The resident bytes the policy asks for never exceed S."""
    assert modgpu.keep_policy(1 << 30) == (True, 255, 48)
    assert modgpu.keep_policy(1 << 32) == (True, 255, 12)
    assert modgpu.keep_policy(1 << 40) == (True, 255, 0)
    assert modgpu.keep_policy((1 << 30) - 1) == (False, 255, 0)
    assert modgpu.keep_policy(320 << 20) == (False, 255, 0) and modgpu.keep_policy(0) == (False, 255, 0)
    for n in (1 << 30, (1 << 30) + 12345, 3 << 30, (1 << 32) + 77, 5 << 33, 1 << 36):
        route, mask, run = modgpu.keep_policy(n)
        assert route and mask == 255 and run == S * 256 // n and run * n <= S * 256 < (run + 1) * n, (n, run)
    import pytest
    with pytest.raises(modgpu.ModGpuError):
        modgpu.debug_set_keep(1, 3, 1)  # the shipped library has no such hook


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-keep` is the TU's own pass (1 kernel); the TU with one of its two store forms gone is REJECTED by name; the object
    waits for its own guard run, which ISA_CHECK=0 leaves out; the stand-in is wired; the TU is built WITH the atomic-optimizer flag (it
    has the ticket)."""
    B.isa_check_target("isa-check-keep", 1)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-keep"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a keep kernel with one store form"
    assert "0 sc1-only and 8 nt sc1 stores in the stream loop" in broken.stdout, broken.stdout[-3000:]
    B.guard_then_compile("cycle_keep_kernel")
    B.unguarded_plan("cycle_keep_kernel")
    B.standin_is_wired("standin_launch_keep.cpp")
    assert "cycle_keep_kernel.h" in B.make_var("CAPI_HDR").split()
    plan = B.dry_run("all")
    for step in ("-S --cuda-device-only", "-c"):
        lines = [ln for ln in plan if f" {step} cycle_keep_kernel.hip " in ln]
        assert len(lines) == 1 and " -mllvm -amdgpu-atomic-optimizer-strategy=None " in lines[0], (step, lines)
    assert sum("cycle_keep_kernel.o" in ln for ln in plan if " -shared " in ln and "libmodgpu" in ln) == 2  # both link lines


def test_codegen_guard_rules_on_altered_assembly():
    """Each rule of the keep branch of check_isa.check() on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_keep_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_keep_kernel.s")).read()
    assert ci.check(asm) == []
    names = list(ci.kernel_bodies(asm))
    assert names == ["_Z24modgpu_cycle_keep_kernelILi4ELi1024EEv13CycleKeepArgs"]
    name = names[0]

    def swap(old, new, count=1):
        assert old in asm
        return asm.replace(old, new, count)

    def meta(field, value):
        m = asm.index("amdhsa.kernels")
        i = asm.index("." + field + ":", m)
        return asm[:i] + "." + field + ":" + " " * 6 + str(value) + asm[asm.index("\n", i):]

    one_store = re.search(r"\tbuffer_store_dwordx4 [^\n]* offen sc1\n", asm).group(0)
    cases = {
        "register counts beyond the budget": meta("vgpr_count", 129),
        "spills, scratch or a private segment": meta("sgpr_spill_count", 3),
        "7 sc1-only and 8 nt sc1 stores": swap(one_store, ""),
        "7 sc1-only and 9 nt sc1 stores": swap(one_store, one_store.replace(" offen sc1", " offen nt sc1")),
        "a data store is neither nt sc1 nor sc1": swap(one_store, one_store.replace(" offen sc1", " offen")),
        "a data load is not nt": swap(" offen nt\n", " offen\n"),
        "global_atomic_add, expected 4": swap("\ts_barrier\n", "\tglobal_atomic_add v1, v2, v3, s[0:1] sc0\n\ts_barrier\n"),
        "the atomic optimizer rewrote the ticket atomic": swap("\ts_barrier\n", "\tv_mbcnt_lo_u32_b32 v1, -1, 0\n\ts_barrier\n"),
        "flat_ accesses": swap("\ts_barrier\n", "\tflat_load_dword v1, v[2:3]\n\ts_barrier\n"),
        "ticket mailbox traffic changed": swap("\tds_read_b32", "\tds_read_b64"),
        "keystream instruction mix changed": swap("\tv_addc_co_u32_sdwa", "\tv_add_co_u32_sdwa"),
        "touched OUTSIDE the keystream blocks": swap("\ts_barrier\n", "\tv_mov_b32_e32 v121, 0\n\ts_barrier\n"),
        "does not end with s_nop 0": swap("\ts_nop 0\n\t\n\t;;#ASMEND", "\t\n\t;;#ASMEND"),
        "holds another kernel": swap("\n" + name + ":", "\n_Z18modgpu_cycle_otherv:\n\ts_endpgm\n" + name + ":"),
        "can be reached with part of the wave masked off": swap("\ts_barrier\n", "\ts_and_saveexec_b64 s[90:91], vcc\n\ts_barrier\n"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_keep_host_code_under_asan_ubsan():
    B.run_sanitized_cases("san_keep_cases.py", "asan", "3 passed")


def test_keep_host_code_under_tsan():
    B.run_sanitized_cases("san_keep_cases.py", "tsan", "3 passed")
