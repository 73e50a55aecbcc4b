"""CPU checks of the rekey table call (modgpu_rekey_table_device & co., include/modgpu.h): the symbols are declared, exported and listed,
the entry layout is pinned, the new TU has a source hash of its own and the older TUs' hashes did not move, the host tier refuses before
anything is queued, modgpu_rekey_table_validate agrees with a brute force, the TU's code-generation guard passes the tree and rejects
broken builds, and the host code runs clean under ASan/UBSan and TSan against the CPU stand-in of the HIP runtime."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
PUBLIC = ("modgpu_rekey_table_workspace_bytes", "modgpu_rekey_table_device", "modgpu_rekey_table_validate")
TESTING = ("modgpu_time_rekey_table_device", "modgpu_rekey_table_kernel_source_hash")
DEBUG = "modgpu_debug_set_rekey_table_grid"
REKEY_TABLE_SRC = ("cycle_rekey_table_kernel.hip", "cycle_table_impl.h", "cycle_rekey_table_kernel.h", "cycle_table_kernel.h", "cycle_rekey_impl.h",
                   "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h")


def _sha(files):
    h = hashlib.sha256()
    for f in files:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()


def test_symbols_declared_exported_and_listed(modgpu):
    public = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    testing = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    for name in PUBLIC:
        assert re.search(r"\b%s\(" % name, public), name
    assert "typedef struct modgpu_rekey_table_entry {" in public and "} modgpu_rekey_table_entry_t;" in public
    for name in TESTING:
        assert re.search(r"\b%s\(" % name, testing), name
    assert "void modgpu_debug_set_rekey_table_grid(uint32_t grid);" in testing
    assert "9 = the rekey table call's stream kernel" in testing
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(PUBLIC + TESTING) <= names, (flavour, set(PUBLIC + TESTING) - names)
        assert (DEBUG in names) == (flavour == "testing")
    assert set(PUBLIC) <= set(modgpu.EXPORTS) and set(TESTING) <= set(modgpu.TESTING_EXPORTS)
    assert DEBUG in modgpu.DEBUG_EXPORTS
    for name in ("rekey_table_device", "time_rekey_table_device", "rekey_table", "rekey_table_workspace_bytes", "rekey_table_validate",
                 "rekey_table_kernel_source_hash", "debug_set_rekey_table_grid", "RekeyTableEntry", "REKEY_TABLE_DTYPE"):
        assert hasattr(modgpu, name), name
    assert modgpu.lib().modgpu_abi_version() == 8


def test_entry_layout_is_pinned(modgpu):
    """56 bytes, 8-byte aligned: the ctypes mirror, the numpy dtype and the header agree field by field."""
    E = modgpu.RekeyTableEntry
    assert ctypes.sizeof(E) == 56 and ctypes.alignment(E) == 8
    want = {"dst": 0, "src": 8, "n": 16, "off_from": 24, "off_to": 32, "key_from": 40, "key_to": 44, "flags": 48, "reserved": 52}
    assert {f: getattr(E, f).offset for f, _ in E._fields_} == want
    assert {f: modgpu.REKEY_TABLE_DTYPE.fields[f][1] for f in want} == want and modgpu.REKEY_TABLE_DTYPE.itemsize == 56
    hdr = open(os.path.join(CSRC, "cycle_rekey_table_kernel.h")).read()
    assert 'static_assert(sizeof(RekeyTableEntry) == 56, "the public entry layout");' in hdr
    assert 'static_assert(sizeof(RekeyTablePlan) == 64, "one s_load_dwordx16");' in hdr
    capi = open(os.path.join(CSRC, "modgpu_capi.cpp")).read()
    assert "sizeof(modgpu_rekey_table_entry_t) == 56" in capi


def test_source_hashes(modgpu):
    assert modgpu.rekey_table_kernel_source_hash() == _sha(REKEY_TABLE_SRC)
    assert modgpu.kernel_source_hash().startswith("d2832a17dddf0901")
    assert modgpu.kernel_source_hash() == _sha(("cycle_kernel_impl.h", "cycle_kernel.hip", "cycle_kernel.h", "lcg.h"))
    assert modgpu.to_kernel_source_hash() == _sha(("cycle_to_kernel.hip", "cycle_to_kernel.h", "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h"))
    assert modgpu.xfer_kernel_source_hash() == _sha(("cycle_xfer_kernel.hip", "cycle_xfer_kernel.h", "cycle_feed_kernel.h", "cycle_kernel_impl.h", "lcg.h"))
    assert modgpu.rekey_kernel_source_hash() == _sha(("cycle_rekey_kernel.hip", "cycle_rekey_kernel.h", "cycle_rekey_impl.h", "cycle_kernel_impl.h",
                                                     "cycle_kernel.h", "lcg.h"))
    assert modgpu.feed_kernel_source_hash() == _sha(("cycle_feed_kernel.hip", "cycle_feed_kernel.h", "cycle_kernel_impl.h", "lcg.h"))
    assert modgpu.table_kernel_source_hash() == _sha(("cycle_table_kernel.hip", "cycle_table_impl.h", "cycle_table_kernel.h", "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h"))
    assert len({modgpu.rekey_table_kernel_source_hash(), modgpu.table_kernel_source_hash(), modgpu.rekey_kernel_source_hash()}) == 3


def test_workspace_size_is_linear(modgpu):
    w = modgpu.rekey_table_workspace_bytes
    assert w(0) == 0 and w((1 << 22) + 1) == 0
    for n in (1, 16, 17, 1000, 100000, 1 << 22):
        assert 80 * n < w(n) <= 86 * n + 4096, (n, w(n))
        assert w(n) >= modgpu.table_workspace_bytes(n) + 16 * n and w(n) % 64 == 0


def _brute(t):
    """modgpu_rekey_batch_device_to's overlap rule plus the entry checks, O(n^2)"""
    live = [i for i in range(len(t)) if t["n"][i]]
    for i in range(len(t)):
        if t["flags"][i] or t["reserved"][i]:
            return False
    for i in live:
        d, s, n = int(t["dst"][i]), int(t["src"][i]), int(t["n"][i])
        if not d or not s:
            return False
        if d != s and d < s + n and s < d + n:
            return False
        for j in live:
            if j == i:
                continue
            dj, sj, nj = int(t["dst"][j]), int(t["src"][j]), int(t["n"][j])
            if (d < sj + nj and sj < d + n) or (d < dj + nj and dj < d + n):
                return False
    return True


def test_validate_against_brute_force(modgpu):
    """Random small tables over a small address range: overlapping sources, self-aliases, destinations touching or meeting other
    ranges, empty entries, flags and reserved."""
    rng = np.random.default_rng(19)
    seen = {True: 0, False: 0}
    for trial in range(3000):
        k = int(rng.integers(1, 9))
        t = modgpu.rekey_table(k)
        t["n"] = rng.integers(0, 12, size=k)
        t["dst"] = 4096 + rng.integers(0, 80, size=k)
        t["src"] = 4096 + rng.integers(0, 80, size=k)
        t["key_from"] = rng.integers(-5, 5, size=k)
        t["off_to"] = rng.integers(0, 1 << 62, size=k)
        alias = rng.random(k) < 0.3
        t["src"][alias] = t["dst"][alias]
        if trial % 50 == 0:
            t["flags"][int(rng.integers(0, k))] = 1
        if trial % 61 == 0:
            t["reserved"][int(rng.integers(0, k))] = 1
        if trial % 97 == 0:
            t["dst"][int(rng.integers(0, k))] = 0
        want = _brute(t)
        try:
            modgpu.rekey_table_validate(t)
            got = True
        except modgpu.ModGpuError as e:
            assert e.code == 1
            got = False
        assert got == want, (trial, t)
        seen[want] += 1
    assert seen[True] > 300 and seen[False] > 300, seen
    t = modgpu.rekey_table(2)
    t[0] = (1000, 5000, 100, 0, 7, 1, 2, 0, 0)
    t[1] = (1100, 5050, 100, 0, 7, 1, 2, 0, 0)       # sources overlap, destinations adjacent: fine
    modgpu.rekey_table_validate(t)
    t[1] = (1100, 1100, 100, 0, 7, 1, 2, 0, 0)       # self-alias next to entry 0's destination: fine
    modgpu.rekey_table_validate(t)
    for bad in ((1099, 1099, 100, 0, 7, 1, 2, 0, 0),  # ... one byte into it
                (1100, 1050, 100, 0, 7, 1, 2, 0, 0),  # a source inside another entry's destination
                (5000, 7000, 100, 0, 7, 1, 2, 0, 0),  # a destination on another entry's source
                (1200, 1210, 100, 0, 7, 1, 2, 0, 0),  # a destination partly over its own source
                (1100, 5050, 100, 0, 7, 1, 2, 0, 1)):  # reserved
        t[1] = bad
        with pytest.raises(modgpu.ModGpuError):
            modgpu.rekey_table_validate(t)
    with pytest.raises(modgpu.ModGpuError, match="entry 1: nonzero flags or reserved"):
        modgpu.rekey_table_validate(t)


def test_host_tier_refuses_before_the_device(modgpu):
    """Without a GPU: every host-tier refusal is MODGPU_ERR_INVALID and queues nothing; n_entries == 0 is a no-op; a well-formed call
    gets as far as the device and fails there (MODGPU_ERR_NO_DEVICE), i.e. nothing is computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    t = np.zeros(64, np.uint64)
    ws = np.zeros(4096, np.uint64)
    tp, wp = t.ctypes.data, ws.ctypes.data
    wb = modgpu.rekey_table_workspace_bytes(3)
    before = modgpu.path_stats()
    assert L.modgpu_rekey_table_device(None, 3, wp, wb, -1, None) == 1
    assert L.modgpu_rekey_table_device(tp, 3, None, wb, -1, None) == 1
    assert L.modgpu_rekey_table_device(tp + 4, 3, wp, wb, -1, None) == 1
    assert L.modgpu_rekey_table_device(tp, 3, wp + 4, wb, -1, None) == 1
    assert L.modgpu_rekey_table_device(tp, 3, wp, wb - 1, -1, None) == 1
    assert L.modgpu_rekey_table_device(tp, 3, wp, modgpu.table_workspace_bytes(3), -1, None) == 1  # the cycle table's size is short
    assert L.modgpu_rekey_table_device(tp, (1 << 22) + 1, wp, 1 << 40, -1, None) == 1
    assert L.modgpu_rekey_table_device(None, 0, None, 0, -1, None) == 0
    assert L.modgpu_rekey_table_device(tp, 3, wp, wb, -1, None) == 2
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] and st["scalar_calls"] == before["scalar_calls"]


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-rekey-table` passes the tree (3 kernels); the TU with the two-keystream block's operand pinned into a fixed
    temporary is REJECTED; the object waits for its own guard run, which ISA_CHECK=0 leaves out; the stand-in is wired.
    (`make isa-check` as a whole: tests/test_capi_cpu.py.)"""
    B.isa_check_target("isa-check-rekey-table", 3)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-rekey-table"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a two-keystream block whose input sits in a fixed temporary"
    assert "the compiler gave a two-keystream block operand a fixed temporary" in broken.stdout, broken.stdout[-3000:]
    B.guard_then_compile("cycle_rekey_table_kernel")
    B.unguarded_plan("cycle_rekey_table_kernel")
    B.standin_is_wired("standin_launch_rekey_table.cpp")
    assert tuple(B.make_var("REKEY_TABLE_SRC").split()) == REKEY_TABLE_SRC


def test_codegen_guard_rules_on_altered_assembly():
    """Rules of the rekey table branch of check_isa.check() on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_rekey_table_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_rekey_table_kernel.s")).read()
    assert ci.check(asm) == []
    names = list(ci.kernel_bodies(asm))
    assert len(names) == 3
    stream = next(n for n in names if "modgpu_cycle_rekey_table_kernel" in n)
    at = asm.index(stream + ":")

    def in_stream(old, new):
        i = asm.index(old, at)
        return asm[:i] + new + asm[i + len(old):]

    cases = {
        "a data load is not nt": in_stream(" offen nt\n", " offen\n"),
        "a data store is not nt sc1": in_stream(" offen nt sc1\n", " offen sc1\n"),
        "the atomic optimizer rewrote": in_stream("\ts_barrier\n", "\tv_mbcnt_lo_u32_b32 v1, -1, 0\n\ts_barrier\n"),
        "touched OUTSIDE the blocks": in_stream("\ts_barrier\n", "\tv_mov_b32_e32 v113, 0\n\ts_barrier\n"),
        "the entry search is not scalar": in_stream("\ts_barrier\n", "\tglobal_load_dword v1, v[2:3], off\n\tglobal_load_dword v1, v[2:3], off\n"
                                                   "\tglobal_load_dword v1, v[2:3], off\n\ts_barrier\n"),
        "is not 60 mads + 30 addc": in_stream("\tv_addc_co_u32_sdwa", "\tv_add_co_u32_sdwa"),
        "three-input XORs": in_stream("bitop3:0x96", "bitop3:0x69"),
        "does not end with s_nop 0": in_stream("\ts_nop 0\n\t\n\t;;#ASMEND", "\t\n\t;;#ASMEND"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_rekey_table_host_code_under_asan_ubsan():
    B.run_sanitized_cases("san_rekey_table_cases.py", "asan", "5 passed")


def test_rekey_table_host_code_under_tsan():
    B.run_sanitized_cases("san_rekey_table_cases.py", "tsan", "5 passed")
