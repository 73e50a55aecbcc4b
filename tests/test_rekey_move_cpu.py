"""CPU checks of the move call (modgpu_rekey_move_device / modgpu_move_workspace_bytes / modgpu_move_status, include/modgpu.h): the
symbols are declared, exported and listed in both flavours, the workspace size behaves, validation comes before any device work, the
rekey TU's guard passes the tree with the move loop's rules and rejects hand-made faults in that loop, the stand-in of the body launch
is wired, and a stand-alone program drives the call on the CPU stand-in of the HIP runtime under ASan + UBSan (its own main, run
directly, the sanitizer runtimes linked statically: the environment's preloads are left alone)."""
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
NEW = ("modgpu_move_workspace_bytes", "modgpu_rekey_move_device", "modgpu_move_status")
CHUNK = 65536


def test_new_symbols_declared_exported_and_listed(modgpu):
    public = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    testing = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    assert re.search(r"\buint64_t modgpu_move_workspace_bytes\(uint64_t n\);", public)
    assert re.search(r"\bint modgpu_rekey_move_device\(void \*dev_dst, const void \*dev_src, uint64_t n,", public)
    assert re.search(r"\bint modgpu_move_status\(const void \*dev_workspace, int device, uint64_t \*stalled_chunk\);", public)
    assert "void modgpu_debug_set_move_grid(uint32_t grid);" in testing
    assert "modgpu_rekey_move_device" in public.split("int modgpu_rekey_device_to(")[0], "the rekey call's text points to the move call"
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
        assert ("modgpu_debug_set_move_grid" in names) == (flavour == "testing")
    assert set(NEW) <= set(modgpu.EXPORTS) and "modgpu_debug_set_move_grid" in modgpu.DEBUG_EXPORTS
    assert modgpu.lib().modgpu_abi_version() == 8
    for name in ("rekey_move_device", "move_workspace_bytes", "move_status", "debug_set_move_grid"):
        assert callable(getattr(modgpu, name)), name
    assert callable(modgpu.DeviceBuffer.move)


def test_workspace_bytes(modgpu):
    w = modgpu.move_workspace_bytes
    assert w(0) == 0 and w(CHUNK << 24) == 0 and w((CHUNK << 24) + 1) == 0 and w((1 << 64) - 1) == 0
    sizes = [1, 15, 16, CHUNK - 1, CHUNK, CHUNK + 1, 1 << 20, (1 << 20) + 1, 4 << 30, 1 << 39, (CHUNK << 24) - 1]
    got = [w(n) for n in sizes]
    assert all(g > 0 and g % 8 == 0 for g in got) and got == sorted(got), got
    # a flag per chunk, the pieces' scratch and a header: 4 bytes per 64 KiB and well under 256 KiB on top
    assert got[0] < 256 << 10 and got[-1] - got[0] <= 4 * (1 << 24) + 256


def test_validation_comes_before_the_device(modgpu):
    """Without a GPU: every refusal that needs no device is MODGPU_ERR_INVALID, n == 0 does nothing, and a call that passes those is
    MODGPU_ERR_NO_DEVICE -- nothing is computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    b = np.arange(4096, dtype=np.uint8)
    keep = b.copy()
    ws = np.zeros(modgpu.move_workspace_bytes(1000) // 8 + 1, np.uint64)
    p, w = b.ctypes.data, ws.ctypes.data
    L = modgpu.lib()
    K3, K4 = modgpu.as_int32(modgpu.KEY_PS3), modgpu.as_int32(modgpu.KEY_PS4)
    nb = modgpu.move_workspace_bytes(1000)
    before = modgpu.path_stats()
    call = L.modgpu_rekey_move_device
    assert call(None, p, 10, K3, 0, K4, 0, w, nb, -1, None) == 1
    assert call(p, None, 10, K3, 0, K4, 0, w, nb, -1, None) == 1
    assert call(p, p + 5, 1000, K3, 0, K4, 0, None, nb, -1, None) == 1
    assert call(p, p + 5, 1000, K3, 0, K4, 0, w + 4, nb, -1, None) == 1          # misaligned
    assert call(p, p + 5, 1000, K3, 0, K4, 0, w, nb - 1, -1, None) == 1          # short
    assert call(p, p + 5, 1000, K3, 0, K4, 0, p + 1000, nb, -1, None) == 1       # meets the source
    assert call(p + 5, p, 1000, K3, 0, K4, 0, p + 1000, nb, -1, None) == 1       # meets the destination
    assert call(p, p + 5, CHUNK << 24, K3, 0, K4, 0, w, 1 << 62, -1, None) == 1  # 2^24 chunks
    assert call(None, None, 0, K3, 0, K4, 0, None, 0, -1, None) == 0
    for d, s in ((p, p + 5), (p + 5, p), (p, p), (p, p + 2000)):
        assert call(d, s, 1000, K3, 3, K4, 5, w, nb, -1, None) == 2
    out = (np.zeros(1, np.uint64)).ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_uint64))
    assert L.modgpu_move_status(None, -1, out) == 1 and L.modgpu_move_status(w, -1, None) == 1 and L.modgpu_move_status(w, -1, out) == 2
    assert np.array_equal(b, keep) and not ws.any()
    assert modgpu.path_stats()["gpu_launches"] == before["gpu_launches"]


def test_codegen_guard_still_passes_and_the_standin_is_wired():
    B.isa_check_target("isa-check-rekey", 2)
    B.standin_is_wired("standin_launch_rekey_move.cpp")
    # not a row of the TU table (the move loop is part of the rekey TU's kernel): no object of its own among the thirteen
    assert "cycle_rekey_move_kernel.o" not in B.make_var("KERNEL_OBJS").split() and len(B.make_var("KERNEL_OBJS").split()) == 13


def test_codegen_guard_rules_of_the_move_loop_on_altered_assembly():
    """Each rule the move loop added to the rekey TU's entry of check_isa.py, on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_rekey_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_rekey_kernel.s")).read()
    assert ci.check(asm) == []
    first = list(ci.kernel_bodies(asm))[0]
    at = asm.index(first + ":")
    sleep = asm.index("\ts_sleep ", at)

    def at_sleep(old, new, back=False):
        i = asm.rindex(old, at, sleep) if back else asm.index(old, sleep)
        return asm[:i] + new + asm[i + len(old):]

    poll = re.compile(r"\tglobal_load_dword (v\d+, v\d+, s\[\d+:\d+\]) sc1\n").search(asm, sleep)
    block = next(m for m in ci.BLOCK.finditer(asm, at) if "s[94:95]" in m.group(0))
    wait = next(m for m in ci.BLOCK.finditer(asm, at) if re.fullmatch(r"\s*s_waitcnt vmcnt\([1-9]\d*\)\s*", m.group(1)))
    cases = {
        "s_barrier, expected 12": at_sleep("\ts_barrier\n", "\ts_barrier\n\ts_barrier\n"),
        "not a sleeping, clock-bounded one": at_sleep("\ts_sleep 8\n", "\ts_nop 0\n"),
        "s_memrealtime; expected 2 and 4": at_sleep("\ts_memrealtime ", "\ts_memtime "),
        "a cache write-back or invalidate": at_sleep("\ts_sleep 8\n", "\tbuffer_inv sc1\n\ts_sleep 8\n"),
        "agent-scope flag reads": asm[:poll.start()] + "\tglobal_load_dword " + poll.group(1) + "\n" + asm[poll.end():],
        "agent-scope dword stores": at_sleep("\tglobal_store_dword v", "\tglobal_store_short v", back=True),
        "global_atomic_add and 1 global_atomic_cmpswap": at_sleep("\tglobal_atomic_cmpswap ", "\tglobal_atomic_swap "),
        "an s_barrier can be reached with part of the wave masked off": at_sleep("\ts_sleep 8\n", "\ts_sleep 8\n\ts_barrier\n"),
        "wait for the chunk's loads is not one": asm[:wait.start()] + wait.group(0).replace("vmcnt(", "vmcnt(1") + asm[wait.end():],
        "between the wait for the chunk's loads and the barrier": asm[:wait.end()] + "\n\tglobal_store_dword v1, v2, s[2:3] sc1\n" + asm[wait.end():],
        "two-keystream blocks, expected 17": asm[:block.start()] + block.group(0).replace("s[94:95]", "s[92:93]") + asm[block.end():],
        "a data store is not nt sc1": at_sleep(" offen nt sc1\n", " offen sc1\n"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_move_on_the_standin_under_asan_ubsan():
    """tests/rekey_move_main.cpp: shifts x phases x sizes in both directions with the key pairs in rotation, every key pair on a few
    geometries, the largest size at 2 or 3 of its 6 phases (the full cross product is the GPU test's); every byte of the arena against
    a model, the launch counts, the plans of the body launches, and every host refusal."""
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "rekey-move-main"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", MODGPU_REQUIRE_GPU="0")
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "rekey_move_main")], env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1].endswith(", 0 failed") and int(lines[-1].split()[0]) == len(lines) - 1 > 1000, lines[-1]
    for what in ("down ps3->ps4", "up   compaction", "down plain", "up   from-identity", "down to-identity", "up   both-identity", "same ps3->ps4",
                 "refusal: 2^24 chunks", "refusal: workspace that is not device memory", "refusal: misaligned workspace", "refusal: short workspace",
                 "refusal: workspace meets the destination", "refusal: null source", "launch plans: 0 move plan errors, 0 rekey plan errors"):
        assert any(ln.startswith("ok   " + what) for ln in lines), what
