"""CPU checks of the table call (modgpu_cycle_table_device & co., include/modgpu.h): the symbols are declared, exported and listed, the
entry layout is pinned, the new TU has a source hash of its own and the older TUs' hashes did not move, the host tier refuses before
anything is queued, modgpu_table_validate agrees with a brute force, the TU's code-generation guard passes the tree and rejects a
broken build, and the host code runs clean under ASan/UBSan and TSan against the CPU stand-in of the HIP runtime."""
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
PUBLIC = ("modgpu_table_workspace_bytes", "modgpu_cycle_table_device", "modgpu_table_status", "modgpu_table_validate")
TESTING = ("modgpu_time_cycle_table_device", "modgpu_table_kernel_source_hash")
TABLE_SRC = ("cycle_table_kernel.hip", "cycle_table_impl.h", "cycle_table_kernel.h", "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h")


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
    assert "typedef struct modgpu_table_entry {" in public and "} modgpu_table_entry_t;" in public
    for name in TESTING:
        assert re.search(r"\b%s\(" % name, testing), name
    assert "void modgpu_debug_set_table_grid(uint32_t grid);" in testing
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(PUBLIC + TESTING) <= names, (flavour, set(PUBLIC + TESTING) - names)
        assert ("modgpu_debug_set_table_grid" in names) == (flavour == "testing")
    assert set(PUBLIC) <= set(modgpu.EXPORTS) and set(TESTING) <= set(modgpu.TESTING_EXPORTS)
    assert "modgpu_debug_set_table_grid" in modgpu.DEBUG_EXPORTS
    assert modgpu.lib().modgpu_abi_version() == 8


def test_entry_layout_is_pinned(modgpu):
    """40 bytes, 8-byte aligned: the ctypes mirror, the numpy dtype and the header agree field by field."""
    E = modgpu.TableEntry
    assert ctypes.sizeof(E) == 40 and ctypes.alignment(E) == 8
    want = {"dst": 0, "src": 8, "n": 16, "stream_off": 24, "key": 32, "flags": 36}
    assert {f: getattr(E, f).offset for f, _ in E._fields_} == want
    assert {f: modgpu.TABLE_DTYPE.fields[f][1] for f in want} == want and modgpu.TABLE_DTYPE.itemsize == 40
    hdr = open(os.path.join(CSRC, "cycle_table_kernel.h")).read()
    assert 'static_assert(sizeof(CycleTableEntry) == 40, "the public entry layout");' in hdr


def test_source_hashes(modgpu):
    assert modgpu.table_kernel_source_hash() == _sha(TABLE_SRC)
    # the roofline's TU is untouched: the hash the committed profiles and bench.py's replayed traffic were taken on
    assert modgpu.kernel_source_hash().startswith("d2832a17dddf0901")
    assert modgpu.kernel_source_hash() == _sha(("cycle_kernel_impl.h", "cycle_kernel.hip", "cycle_kernel.h", "lcg.h"))
    assert modgpu.to_kernel_source_hash() == _sha(("cycle_to_kernel.hip", "cycle_to_kernel.h", "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h"))
    assert modgpu.xfer_kernel_source_hash() == _sha(("cycle_xfer_kernel.hip", "cycle_xfer_kernel.h", "cycle_feed_kernel.h", "cycle_kernel_impl.h", "lcg.h"))
    assert modgpu.rekey_kernel_source_hash() == _sha(("cycle_rekey_kernel.hip", "cycle_rekey_kernel.h", "cycle_rekey_impl.h", "cycle_kernel_impl.h",
                                                     "cycle_kernel.h", "lcg.h"))
    assert modgpu.feed_kernel_source_hash() == _sha(("cycle_feed_kernel.hip", "cycle_feed_kernel.h", "cycle_kernel_impl.h", "lcg.h"))


def test_workspace_size_is_linear(modgpu):
    w = modgpu.table_workspace_bytes
    assert w(0) == 0 and w((1 << 22) + 1) == 0
    for n in (1, 16, 17, 1000, 100000, 1 << 22):
        assert 64 * n < w(n) <= 70 * n + 4096, (n, w(n))


def _brute(t):
    """the overlap rule of modgpu_cycle_batch_device_to, O(n^2)"""
    live = [i for i in range(len(t)) if t["n"][i]]
    for i in range(len(t)):
        if t["flags"][i]:
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
    """Random small tables over a small address range: overlapping sources, self-aliases, destinations touching (adjacent to) or
    meeting other ranges, empty entries, flags."""
    rng = np.random.default_rng(9)
    seen = {True: 0, False: 0}
    for trial in range(3000):
        k = int(rng.integers(1, 9))
        t = modgpu.table(k)
        t["n"] = rng.integers(0, 12, size=k)
        t["dst"] = 4096 + rng.integers(0, 80, size=k)
        t["src"] = 4096 + rng.integers(0, 80, size=k)
        alias = rng.random(k) < 0.3
        t["src"][alias] = t["dst"][alias]
        if trial % 50 == 0:
            t["flags"][int(rng.integers(0, k))] = 1
        if trial % 97 == 0:
            t["dst"][int(rng.integers(0, k))] = 0
        want = _brute(t)
        try:
            modgpu.table_validate(t)
            got = True
        except modgpu.ModGpuError as e:
            assert e.code == 1
            got = False
        assert got == want, (trial, t)
        seen[want] += 1
    assert seen[True] > 300 and seen[False] > 300, seen
    # the named cases
    t = modgpu.table(2)
    t[0] = (1000, 5000, 100, 0, 1, 0)
    t[1] = (1100, 5050, 100, 0, 1, 0)       # sources overlap, destinations adjacent: fine
    modgpu.table_validate(t)
    t[1] = (1100, 1100, 100, 0, 1, 0)       # self-alias next to entry 0's destination: fine
    modgpu.table_validate(t)
    t[1] = (1099, 1099, 100, 0, 1, 0)       # ... one byte into it: refused
    with pytest.raises(modgpu.ModGpuError):
        modgpu.table_validate(t)
    t[1] = (1100, 1050, 100, 0, 1, 0)       # a source inside another entry's destination: refused
    with pytest.raises(modgpu.ModGpuError):
        modgpu.table_validate(t)
    t[1] = (5000, 7000, 100, 0, 1, 0)       # a destination on another entry's source: refused
    with pytest.raises(modgpu.ModGpuError):
        modgpu.table_validate(t)


def test_host_tier_refuses_before_the_device(modgpu):
    """Without a GPU: every host-tier refusal is MODGPU_ERR_INVALID and queues nothing; n_entries == 0 is a no-op; a well-formed call
    gets as far as the device and fails there (MODGPU_ERR_NO_DEVICE), i.e. nothing is computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    t = np.zeros(64, np.uint64)
    ws = np.zeros(4096, np.uint64)
    tp, wp = t.ctypes.data, ws.ctypes.data
    wb = modgpu.table_workspace_bytes(3)
    before = modgpu.path_stats()
    assert L.modgpu_cycle_table_device(None, 3, wp, wb, -1, None) == 1
    assert L.modgpu_cycle_table_device(tp, 3, None, wb, -1, None) == 1
    assert L.modgpu_cycle_table_device(tp + 4, 3, wp, wb, -1, None) == 1
    assert L.modgpu_cycle_table_device(tp, 3, wp + 4, wb, -1, None) == 1
    assert L.modgpu_cycle_table_device(tp, 3, wp, wb - 1, -1, None) == 1
    assert L.modgpu_cycle_table_device(tp, (1 << 22) + 1, wp, 1 << 40, -1, None) == 1
    assert L.modgpu_cycle_table_device(None, 0, None, 0, -1, None) == 0
    assert L.modgpu_cycle_table_device(tp, 3, wp, wb, -1, None) == 2
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] and st["scalar_calls"] == before["scalar_calls"]


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-table` is the guard's pass over the table TU (3 kernels); the TU with the keystream block's lane state pinned
    into a fixed temporary is REJECTED; the object waits for its own guard run, which ISA_CHECK=0 leaves out; the stand-in is wired.
    (`make isa-check` as a whole: tests/test_capi_cpu.py.)"""
    B.isa_check_target("isa-check-table", 3)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-table"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a keystream block whose input sits in a fixed temporary"
    assert "the compiler gave a block operand a fixed temporary" in broken.stdout, broken.stdout[-3000:]
    B.guard_then_compile("cycle_table_kernel")
    B.unguarded_plan("cycle_table_kernel")
    B.standin_is_wired("standin_launch_table.cpp")
    assert tuple(B.make_var("TABLE_SRC").split()) == TABLE_SRC


def test_the_table_tus_share_one_copy_of_their_device_code():
    """The five table TUs take what they have in common from cycle_table_impl.h: each of these lines of it -- the power tables, the line
    of 16 keys, the funnel, mulmod_keep, the descent's count -- is in that header and in none of the five .hip files, and every one of
    the five source lists (so every one of the five hashes) names the header."""
    header = "cycle_table_impl.h"
    tus = {"TABLE_SRC": "cycle_table_kernel.hip", "REKEY_TABLE_SRC": "cycle_rekey_table_kernel.hip", "VERIFY_TABLE_SRC": "cycle_verify_table_kernel.hip",
           "REKEY_VERIFY_TABLE_SRC": "cycle_rekey_verify_table_kernel.hip", "REKEY_MOVE_TABLE_SRC": "cycle_rekey_move_table_kernel.hip"}
    text = {f: open(os.path.join(CSRC, f)).read() for f in [header] + list(tus.values())}
    for token in ("make_pow_table<256>(1)", "struct Keys16", "__builtin_amdgcn_alignbyte(w.e", "mul_fold(x, 2u * y)", "keys.v[t] <= g"):
        assert [f for f, t in text.items() if token in t] == [header], token
    for var, hip in tus.items():
        src = B.make_var(var).split()
        assert src[0] == hip and src.count(header) == 1 and f'#include "{header}"' in text[hip], var


def test_codegen_guard_rules_on_altered_assembly():
    """Rules of the table branch of check_isa.check() on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_table_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_table_kernel.s")).read()
    assert ci.check(asm) == []
    names = list(ci.kernel_bodies(asm))
    assert len(names) == 3
    stream = next(n for n in names if "modgpu_cycle_table_kernel" in n)
    at = asm.index(stream + ":")

    def in_stream(old, new):
        i = asm.index(old, at)
        return asm[:i] + new + asm[i + len(old):]

    cases = {
        "a data load is not nt": in_stream(" offen nt\n", " offen\n"),
        "a data store is not nt sc1": in_stream(" offen nt sc1\n", " offen sc1\n"),
        "the atomic optimizer rewrote": in_stream("\ts_barrier\n", "\tv_mbcnt_lo_u32_b32 v1, -1, 0\n\ts_barrier\n"),
        "touched OUTSIDE the keystream blocks": in_stream("\ts_barrier\n", "\tv_mov_b32_e32 v121, 0\n\ts_barrier\n"),
        "the entry search is not scalar": in_stream("\ts_barrier\n", "\tglobal_load_dword v1, v[2:3], off\n\tglobal_load_dword v1, v[2:3], off\n"
                                                   "\tglobal_load_dword v1, v[2:3], off\n\ts_barrier\n"),
        "is not 30 mads + 15 addc": in_stream("\tv_addc_co_u32_sdwa", "\tv_add_co_u32_sdwa"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_table_host_code_under_asan_ubsan():
    B.run_sanitized_cases("san_table_cases.py", "asan", "5 passed")


def test_table_host_code_under_tsan():
    B.run_sanitized_cases("san_table_cases.py", "tsan", "5 passed")
