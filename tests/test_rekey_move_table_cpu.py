"""CPU checks of the rekey move table call (modgpu_rekey_move_table_device & co., include/modgpu.h): the symbols are declared, exported
and listed in both flavours, the entry layout is the rekey table call's and the workspace starts with the table call's header, the
workspace size behaves, the host validator decides every fault of the direction and order rule as the device does, tier 1 comes before
any device work, the TU has the Makefile rules of a table row and a hash of its own, its guard passes the tree and rejects a hand-made
fault and a broken build, the stand-in is wired, and a stand-alone program drives the call on the CPU stand-in of the HIP runtime
under ASan + UBSan (its own main, run directly, the sanitizer runtimes linked statically: the environment's preloads are left alone)."""
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
PUBLIC = ("modgpu_rekey_move_table_workspace_bytes", "modgpu_rekey_move_table_device", "modgpu_rekey_move_table_validate", "modgpu_rekey_move_table_status")
TESTING = ("modgpu_rekey_move_table_kernel_source_hash",)
DEBUG = "modgpu_debug_set_move_table_grid"
SRC = ("cycle_rekey_move_table_kernel.hip", "cycle_table_impl.h", "cycle_rekey_move_table_kernel.h", "cycle_rekey_table_kernel.h", "cycle_table_kernel.h", "cycle_rekey_impl.h",
       "cycle_kernel_impl.h", "cycle_kernel.h", "lcg.h")
CHUNK = 65536
MAX_ENTRIES = 1 << 22


def test_symbols_declared_exported_and_listed(modgpu):
    public = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    testing = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    assert "uint64_t modgpu_rekey_move_table_workspace_bytes(uint64_t n_entries, uint64_t total_bytes);" in public
    assert re.search(r"\bint modgpu_rekey_move_table_device\(const modgpu_rekey_table_entry_t \*dev_entries, uint64_t n_entries, uint64_t total_bytes,\s+"
                     r"void \*dev_workspace, uint64_t workspace_bytes, int device, void \*hip_stream\);", public)
    assert "int modgpu_rekey_move_table_validate(const modgpu_rekey_table_entry_t *host_entries, uint64_t n_entries);" in public
    assert "int modgpu_rekey_move_table_status(const void *dev_workspace, int device, uint64_t *first_bad_entry, uint64_t *stalled_chunk);" in public
    text = public.split("uint64_t modgpu_rekey_move_table_workspace_bytes(")[0].split("a TABLE of rekey entries MOVED")[1]
    for said in ("FIVE kernel launches", "variant 15", "Page-locked host memory anywhere in a table\n * is not supported", "DOWNWARD", "UPWARD",
                 "total_bytes / 64 KiB + 2 * n_entries", "32 bytes of scratch per entry", "never touches the library's ring", "2 s"):
        assert said in text, said
    assert "#define MODGPU_ABI_VERSION 8\n" in public
    assert "void modgpu_debug_set_move_table_grid(uint32_t grid);" in testing and "modgpu_rekey_move_table_kernel_source_hash(void);" in testing
    assert "15 = the move launch of modgpu_rekey_move_table_device" in testing and "modgpu_rekey_move_table_kernel_source_hash() for variant 15" in testing
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(PUBLIC + TESTING) <= names, (flavour, set(PUBLIC + TESTING) - names)
        assert (DEBUG in names) == (flavour == "testing")
    assert set(PUBLIC) <= set(modgpu.EXPORTS) and set(TESTING) <= set(modgpu.TESTING_EXPORTS) and DEBUG in modgpu.DEBUG_EXPORTS
    for name in ("rekey_move_table_device", "rekey_move_table_workspace_bytes", "rekey_move_table_validate", "rekey_move_table_status",
                 "compaction_table", "rekey_move_table_kernel_source_hash", "debug_set_move_table_grid"):
        assert callable(getattr(modgpu, name)), name
    assert callable(modgpu.DeviceBuffer.compact)
    assert modgpu.lib().modgpu_abi_version() == 8


def test_layouts_are_reused():
    """the entry is the rekey table call's 56 bytes as it stands; the workspace starts with the table call's header (modgpu_table_status
    reads it); the plan record is one s_load_dwordx16"""
    hdr = open(os.path.join(CSRC, "cycle_rekey_move_table_kernel.h")).read()
    assert '#include "cycle_rekey_table_kernel.h"' in hdr and "const RekeyTableEntry *entries;" in hdr and "struct RekeyTableEntry" not in hdr
    assert "sizeof(MoveTableHdr) == sizeof(CycleTableHdr) && offsetof(MoveTableHdr, first_bad) == offsetof(CycleTableHdr, first_bad)" in hdr
    assert 'static_assert(sizeof(MoveTablePlan) == 64, "one s_load_dwordx16");' in hdr
    assert "constexpr int CYCLE_REKEY_MOVE_TABLE = 15;" in hdr and "constexpr uint64_t kMoveTableStallTicks = 200000000ull;" in hdr
    capi = open(os.path.join(CSRC, "modgpu_capi.cpp")).read()
    assert "uint64_t at = sizeof(MoveTableHdr);" in capi


def test_source_list_hash_and_row(modgpu):
    assert tuple(B.make_var("REKEY_MOVE_TABLE_SRC").split()) == SRC
    assert "cycle_rekey_move_table_kernel.h" in B.make_var("CAPI_HDR").split()
    # a row of the Makefile's table of TUs like every other: its object is on both link lines, once
    assert "rekey_move_table" in B.make_var("TUS").split() and "cycle_rekey_move_table_kernel.o" in B.make_var("KERNEL_OBJS").split()
    for lib in ("libmodgpu.so", "libmodgpu_testing.so"):
        links = [ln.split() for ln in B.dry_run("all") if " -shared " in ln and f" -o ../{lib} " in ln]
        assert len(links) == 1 and links[0].count("cycle_rekey_move_table_kernel.o") == 1, links
    h = hashlib.sha256()
    for f in SRC:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    assert modgpu.rekey_move_table_kernel_source_hash() == h.hexdigest()
    others = {modgpu.kernel_source_hash(), modgpu.feed_kernel_source_hash(), modgpu.to_kernel_source_hash(), modgpu.xfer_kernel_source_hash(),
              modgpu.rekey_kernel_source_hash(), modgpu.table_kernel_source_hash(), modgpu.rekey_table_kernel_source_hash(),
              modgpu.verify_kernel_source_hash(), modgpu.verify_table_kernel_source_hash(), modgpu.rekey_verify_kernel_source_hash(),
              modgpu.keep_kernel_source_hash(), modgpu.rekey_verify_table_kernel_source_hash()}
    assert len(others) == 12 and modgpu.rekey_move_table_kernel_source_hash() not in others
    assert modgpu.kernel_source_hash().startswith("d2832a17dddf0901")


def test_workspace_bytes(modgpu):
    w = modgpu.rekey_move_table_workspace_bytes
    assert w(0, 1000) == 0 and w(0, 0) == 0 and w(MAX_ENTRIES + 1, 1000) == 0 and w(1, (1 << 64) - 1) == 0 and w(1, CHUNK << 31) == 0
    ns = [1, 2, 16, 17, 1000, 1024, 1025, 100000, MAX_ENTRIES]
    bs = [0, 1, CHUNK - 1, CHUNK, 1 << 20, (1 << 20) + 1, 4 << 30, 1 << 40]
    grid = [[w(n, b) for b in bs] for n in ns]
    assert all(g > 0 and g % 64 == 0 for row in grid for g in row)
    assert all(row == sorted(row) for row in grid) and all(col == tuple(sorted(col)) for col in zip(*grid)), "not monotone"
    # per entry: the rekey table call's records, 32 bytes of scratch and two chunks' flag and window; per 64 KiB: 12 bytes
    for n, row in zip(ns, grid):
        assert row[0] >= modgpu.rekey_table_workspace_bytes(n) + (32 + 2 * 12) * n
        assert 12 * (4 << 30) // CHUNK <= row[6] - row[0] <= 12 * (4 << 30) // CHUNK + 128


def _table(modgpu, rows):
    t = modgpu.rekey_table(len(rows))
    for i, (d, s, n) in enumerate(rows):
        t[i]["dst"], t[i]["src"], t[i]["n"] = d, s, n
        t[i]["key_from"], t[i]["key_to"], t[i]["off_from"], t[i]["off_to"] = 1, 2, s, d
    return t


DOWN = [(1000, 1100, 50), (1050, 1200, 100), (1150, 1300, 1), (1151, 1301, 40), (2000, 2000, 10), (2010, 2500, 64)]
UP = [(s, d, n) for d, s, n in DOWN]


def test_validate_takes_downward_and_upward_tables(modgpu):
    for rows in (DOWN, UP, DOWN[:1], UP[:1], [(5, 5, 9)], [(5, 5, 9), (14, 14, 1), (15, 16, 3)], [(5, 5, 9), (14, 14, 1), (16, 15, 3)]):
        modgpu.rekey_move_table_validate(_table(modgpu, rows))
    # empty entries are dropped before the rule applies, whatever their pointers
    holes = [(0, 0, 0), DOWN[0], (9, 1 << 40, 0), DOWN[1], DOWN[2], (1 << 40, 3, 0)] + DOWN[3:] + [(7, 7, 0)]
    modgpu.rekey_move_table_validate(_table(modgpu, holes))
    modgpu.rekey_move_table_validate(modgpu.rekey_table(0))
    modgpu.rekey_move_table_validate(modgpu.rekey_table(3))  # all empty
    # a destination on top of another entry's source is the point of the call; the rekey table call's validator refuses it
    with pytest.raises(modgpu.ModGpuError):
        modgpu.rekey_table_validate(_table(modgpu, DOWN))


@pytest.mark.parametrize("what,rows,bad", [
    ("an upward entry in a downward table", DOWN[:3] + [(1301, 1151, 40)] + DOWN[4:], 3),
    ("a downward entry in an upward table", UP[:5] + [(2010, 2500, 64)], 5),
    ("the direction is the first sliding entry's", [(5, 5, 9)] + UP[:2] + DOWN[3:4], 3),
    ("two entries listed in falling order", [DOWN[0], DOWN[2], DOWN[1]] + DOWN[3:], 2),
    ("overlapping destinations", DOWN[:1] + [(1049, 1200, 100)] + DOWN[2:], 1),
    ("overlapping sources", DOWN[:3] + [(1151, 1300, 40)] + DOWN[4:], 3),
    ("a destination below the previous one across an empty entry", DOWN[:2] + [(0, 0, 0), (1149, 1300, 1)] + DOWN[3:], 3),
    ("a null source", DOWN[:4] + [(2000, 0, 10)], 4),
    ("a null destination", [(0, 1100, 50)] + DOWN[1:], 0),
    ("an entry of 1 TiB or more", DOWN[:5] + [(2010, 1 << 41, 1 << 40)], 5),
])
def test_validate_names_the_entry_at_fault(modgpu, what, rows, bad):
    with pytest.raises(modgpu.ModGpuError, match=f"entry {bad}:") as e:
        modgpu.rekey_move_table_validate(_table(modgpu, rows))
    assert e.value.code == 1, what


def test_validate_flags_and_limits(modgpu):
    for field in ("flags", "reserved"):
        t = _table(modgpu, DOWN)
        t[4][field] = 1
        t[2][field] = 1 << 31
        with pytest.raises(modgpu.ModGpuError, match="entry 2: nonzero flags or reserved"):
            modgpu.rekey_move_table_validate(t)
    L = modgpu.lib()
    assert L.modgpu_rekey_move_table_validate(None, 3) == 1 and L.modgpu_rekey_move_table_validate(None, 0) == 0
    assert L.modgpu_rekey_move_table_validate(_table(modgpu, DOWN).ctypes.data, MAX_ENTRIES + 1) == 1


def test_compaction_table(modgpu):
    keep = [(100, 50), (200, 1), (201, 0), (300, 70000), (80000, 16)]
    t = modgpu.compaction_table(1 << 30, keep, modgpu.KEY_PS4, part_off=7)
    new = [100, 150, 151, 151, 70151]
    assert [int(x) - (1 << 30) for x in t["dst"]] == new and [int(x) - (1 << 30) for x in t["src"]] == [o for o, _ in keep]
    assert [int(x) for x in t["n"]] == [n for _, n in keep]
    assert [int(x) for x in t["off_from"]] == [7 + o for o, _ in keep] and [int(x) for x in t["off_to"]] == [7 + o for o in new]
    assert set(t["key_from"]) == set(t["key_to"]) == {modgpu.as_int32(modgpu.KEY_PS4)} and not t["flags"].any() and not t["reserved"].any()
    modgpu.rekey_move_table_validate(t)
    with pytest.raises(ValueError):
        modgpu.compaction_table(1 << 30, [(100, 50), (149, 5)], modgpu.KEY_PS4)
    assert modgpu.compaction_table(1 << 30, [], modgpu.KEY_PS4).size == 0


def test_tier_1_comes_before_the_device(modgpu):
    """Without a GPU: every host-tier refusal is MODGPU_ERR_INVALID and queues nothing; n_entries == 0 is a no-op; a well-formed call
    gets as far as the device and fails there (MODGPU_ERR_NO_DEVICE), i.e. nothing is computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    t = np.zeros(64, np.uint64)
    wb = modgpu.rekey_move_table_workspace_bytes(3, 1 << 20)
    ws = np.zeros(wb // 8 + 8, np.uint64)
    tp, wp = t.ctypes.data, ws.ctypes.data
    before = modgpu.path_stats()
    call = L.modgpu_rekey_move_table_device
    assert call(None, 3, 1 << 20, wp, wb, -1, None) == 1
    assert call(tp, 3, 1 << 20, None, wb, -1, None) == 1
    assert call(tp + 4, 3, 1 << 20, wp, wb, -1, None) == 1
    assert call(tp, 3, 1 << 20, wp + 4, wb, -1, None) == 1
    assert call(tp, 3, 1 << 20, wp, wb - 1, -1, None) == 1
    assert call(tp, 3, (1 << 20) + 16 * CHUNK, wp, wb, -1, None) == 1     # the workspace was sized for fewer chunks (sections are whole lines)
    assert call(tp, MAX_ENTRIES + 1, 1 << 20, wp, 1 << 62, -1, None) == 1
    assert call(tp, 3, CHUNK << 31, wp, 1 << 62, -1, None) == 1           # beyond 2^31 chunks
    assert call(None, 0, 0, None, 0, -1, None) == 0
    assert call(tp, 3, 1 << 20, wp, wb, -1, None) == 2
    a, b = ctypes.c_uint64(5), ctypes.c_uint64(5)
    status = L.modgpu_rekey_move_table_status
    assert status(None, -1, ctypes.byref(a), ctypes.byref(b)) == 1 and status(wp, -1, None, ctypes.byref(b)) == 1 and status(wp, -1, ctypes.byref(a), None) == 1
    assert status(wp, -1, ctypes.byref(a), ctypes.byref(b)) == 2
    assert not t.any() and not ws.any()
    assert modgpu.path_stats()["gpu_launches"] == before["gpu_launches"]


def test_codegen_guard_passes_and_the_standin_is_wired():
    B.isa_check_target("isa-check-rekey-move-table", 5)
    # the object waits for its guard, which ISA_CHECK=0 leaves out without touching a stamp
    B.guard_then_compile("cycle_rekey_move_table_kernel")
    B.unguarded_plan("cycle_rekey_move_table_kernel")
    # `isa-check`, the aggregate of every TU, runs this one's guard, once
    guard = "python3 check_isa.py cycle_rekey_move_table_kernel.s"
    runs = [ln for ln in B.dry_run("isa-check") if ln.startswith("python3 check_isa.py")]
    assert len(runs) == 12 and runs.count(guard) == 1, runs
    B.standin_is_wired("standin_launch_rekey_move_table.cpp")
    flag = "-amdgpu-atomic-optimizer-strategy=None"
    for step in ("-S --cuda-device-only", "-c"):
        lines = [ln for ln in B.dry_run("all") if f" {step} cycle_rekey_move_table_kernel.hip " in ln]
        assert len(lines) == 1 and f" -mllvm {flag} " in lines[0], (step, lines)


def test_codegen_guard_rejects_a_build_whose_poll_does_not_sleep():
    r = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-rekey-move-table"], capture_output=True, text=True, timeout=900)
    assert r.returncode != 0, "the guard accepted a move kernel whose poll spins without sleeping"
    assert "the poll is not a sleeping, clock-bounded one" in r.stdout, r.stdout[-3000:]


def test_codegen_guard_rules_on_altered_assembly():
    """Each rule of the TU's entry in check_isa.py, on the tree's own assembly with one fault put in by hand."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_rekey_move_table_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_rekey_move_table_kernel.s")).read()
    assert ci.check(asm) == []
    move = next(k for k in ci.kernel_bodies(asm) if "move_table_kernel" in k)
    at = asm.index(move + ":")
    sleep = asm.index("\ts_sleep ", at)

    def at_sleep(old, new, back=False):
        i = asm.rindex(old, at, sleep) if back else asm.index(old, sleep)
        return asm[:i] + new + asm[i + len(old):]

    poll = re.compile(r"\tglobal_load_dword (v\d+, v\d+, s\[\d+:\d+\]) sc1\n").search(asm, sleep)
    block = next(m for m in ci.BLOCK.finditer(asm, at) if "s[94:95]" in m.group(0))
    wait = next(m for m in ci.BLOCK.finditer(asm, at) if re.fullmatch(r"\s*s_waitcnt vmcnt\([1-9]\d*\)\s*", m.group(1)))
    ticket = re.compile(r"\tglobal_atomic_add (v\d+, v\d+, v\d+, s\[\d+:\d+\])( offset:\d+)? sc0\n").search(asm, at)
    cases = {
        "s_barrier, expected 8": at_sleep("\ts_barrier\n", "\ts_barrier\n\ts_barrier\n"),
        "not a sleeping, clock-bounded one": at_sleep("\ts_sleep 8\n", "\ts_nop 0\n"),
        "s_memrealtime; expected 2 and 4": at_sleep("\ts_memrealtime ", "\ts_memtime "),
        "a cache write-back or invalidate": at_sleep("\ts_sleep 8\n", "\tbuffer_inv sc1\n\ts_sleep 8\n"),
        "agent-scope flag reads": asm[:poll.start()] + "\tglobal_load_dword " + poll.group(1) + "\n" + asm[poll.end():],
        "agent-scope dword stores": at_sleep("\tglobal_store_dword v", "\tglobal_store_short v", back=True),
        "global_atomic_cmpswap (expected 2": at_sleep("\tglobal_atomic_cmpswap ", "\tglobal_atomic_swap "),
        "expected 4 returning ones": asm[:ticket.start()] + ticket.group(0).replace(" sc0\n", "\n") + asm[ticket.end():],
        "an s_barrier can be reached with part of the wave masked off": at_sleep("\ts_sleep 8\n", "\ts_sleep 8\n\ts_barrier\n"),
        "wait for the chunk's loads is not one": asm[:wait.start()] + wait.group(0).replace("vmcnt(", "vmcnt(1") + asm[wait.end():],
        "between the wait for the chunk's loads and the barrier": asm[:wait.end()] + "\n\tglobal_store_dword v1, v2, s[2:3] sc1\n" + asm[wait.end():],
        "two-keystream blocks, expected 8": asm[:block.start()] + block.group(0).replace("s[94:95]", "s[92:93]") + asm[block.end():],
        "a data store is not nt sc1": at_sleep(" offen nt sc1\n", " offen sc1\n"),
        "holds 0 modgpu_cycle_rekey_move_table_place": asm.replace("modgpu_cycle_rekey_move_table_place", "modgpu_cycle_rekey_move_table_plaze"),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])


def test_move_table_on_the_standin_under_asan_ubsan():
    """tests/rekey_move_table_main.cpp: the matrix at reduced size, the waits across entries, every device refusal and every host
    refusal, every byte of the arena against a model, and the windows the stand-in planned."""
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "rekey-move-table-main"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", MODGPU_REQUIRE_GPU="0")
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "rekey_move_table_main")], env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1].endswith(", 0 failed") and int(lines[-1].split()[0]) == len(lines) - 1 > 150, lines[-1]
    for what in ("down ps3->ps4", "up   compaction", "down plain", "up   from-identity", "down to-identity", "up   both-identity", "down mixed", "up   mixed",
                 "down big mixed", "up   big mixed", "down across gaps below a chunk", "up   across 300 small entries", "down an entry in the middle stays",
                 "up   with empty entries", "down one entry", "device refusal: an upward entry in a downward table", "device refusal: two entries listed in falling order",
                 "device refusal: overlapping destinations", "device refusal: overlapping sources", "device refusal: nonzero flags",
                 "device refusal: total_bytes too small for the table", "refusal: short workspace", "refusal: workspace that is not device memory",
                 "launch plans: 0 window errors"):
        assert any(ln.startswith("ok   " + what) for ln in lines), what
