"""CPU checks of the relayout call (modgpu_rekey_relayout_table_device & _validate, include/modgpu.h): a table of rekey entries whose
segments slide both ways, moved as two sweeps of the rekey move table call's five launches.  The symbols are declared, exported and
listed in both flavours; the host validator takes every table of the rule without its direction clause and names the entry at fault for
the rest, while the move table call's validator still refuses a mixed table; tier 1 comes before any device work; the splice arithmetic
and the table builder give hand-computed values; the TU still has five kernels and passes its guard; the stand-in is wired; and a
stand-alone program drives the call on the CPU stand-in of the HIP runtime under ASan + UBSan (its own main, run directly, the
sanitizer runtimes linked statically: the environment's preloads are left alone)."""
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
PUBLIC = ("modgpu_rekey_relayout_table_device", "modgpu_rekey_relayout_table_validate")
CHUNK = 65536
MAX_ENTRIES = 1 << 22


def test_symbols_declared_exported_and_listed(modgpu):
    public = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    assert re.search(r"\bint modgpu_rekey_relayout_table_device\(const modgpu_rekey_table_entry_t \*dev_entries, uint64_t n_entries, uint64_t total_bytes,\s+"
                     r"void \*dev_workspace, uint64_t workspace_bytes, int device, void \*hip_stream\);", public)
    assert "int modgpu_rekey_relayout_table_validate(const modgpu_rekey_table_entry_t *host_entries, uint64_t n_entries);" in public
    # its comment block stands behind the move table call's declarations, which are as they were
    text = public.split("int modgpu_rekey_move_table_status(const void *dev_workspace")[1].split("int modgpu_rekey_relayout_table_device(")[0]
    for said in ("TEN kernel launches", "variant 15", "no direction clause", "ALL OR NOTHING", "not per sweep", "modgpu_rekey_move_table_workspace_bytes",
                 "modgpu_rekey_move_table_status", "in the numbering of the sweep that stalled", "diagnostic only", "sweep 1 then stores nothing"):
        assert said in text, said
    assert "#define MODGPU_ABI_VERSION 8\n" in public
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(PUBLIC) <= names, (flavour, set(PUBLIC) - names)
    assert set(PUBLIC) <= set(modgpu.EXPORTS)
    for name in ("rekey_relayout_table_device", "rekey_relayout_table_validate", "relayout_table", "splice_moves"):
        assert callable(getattr(modgpu, name)), name
    assert callable(modgpu.DeviceBuffer.relayout) and callable(modgpu.DeviceBuffer.splice)
    assert modgpu.lib().modgpu_abi_version() == 8


def test_the_sweep_is_a_mode_not_a_kernel():
    """no kernel and no TU was added: the sweep is a trailing field of MoveTableArgs, the records keep their sizes, and the sweep-aware
    plan and finish have launch functions of their own"""
    hdr = open(os.path.join(CSRC, "cycle_rekey_move_table_kernel.h")).read()
    args = hdr.split("struct MoveTableArgs {")[1].split("};")[0]
    assert args.rstrip().splitlines()[-1].strip().startswith("uint32_t sweep;")
    assert 'static_assert(sizeof(MoveTablePlan) == 64, "one s_load_dwordx16");' in hdr and 'static_assert(sizeof(MoveTableBlk) == 32, "two per line");' in hdr
    assert "hipError_t modgpu_launch_rekey_relayout_plan(const MoveTableArgs &a, uint32_t sweep, hipStream_t stream);" in hdr
    assert "hipError_t modgpu_launch_rekey_relayout_finish(const MoveTableArgs &a, uint32_t sweep, hipStream_t stream);" in hdr
    src = open(os.path.join(CSRC, "cycle_rekey_move_table_kernel.hip")).read()
    assert len(re.findall(r"^(?:template <[^>]*>\n)?__global__ ", src, re.M)) == 5
    assert "rekey_relayout" not in B.make_var("TUS")


def _table(modgpu, rows):
    t = modgpu.rekey_table(len(rows))
    for i, (d, s, n) in enumerate(rows):
        t[i]["dst"], t[i]["src"], t[i]["n"] = d, s, n
        t[i]["key_from"], t[i]["key_to"], t[i]["off_from"], t[i]["off_to"] = 1, 2, s, d
    return t


DOWN = [(1000, 1100, 50), (1050, 1200, 100), (1150, 1300, 1), (1151, 1301, 40), (2000, 2000, 10), (2010, 2500, 64)]
UP = [(s, d, n) for d, s, n in DOWN]
ALTERNATING = [(1007, 1000, 9), (1018, 1025, 9), (1057, 1050, 9), (1068, 1075, 9)]


def far(rows, by=10000):
    return [(d + by, s + by, n) for d, s, n in rows]


def test_validate_takes_tables_that_slide_both_ways(modgpu):
    mixed = [DOWN + far(UP), UP + far(DOWN), DOWN[:2] + far(UP[:3]) + far(DOWN, 20000), ALTERNATING, ALTERNATING[1:]]
    for rows in mixed:
        modgpu.rekey_relayout_table_validate(_table(modgpu, rows))
        with pytest.raises(modgpu.ModGpuError, match="slides (up in a downward|down in an upward) table"):
            modgpu.rekey_move_table_validate(_table(modgpu, rows))  # the move table call's validator refuses them exactly as before
    # empty entries are dropped before the rule applies, whatever their pointers
    holes = [(0, 0, 0)] + DOWN[:2] + [(9, 1 << 40, 0)] + DOWN[2:] + [(1 << 40, 3, 0)] + far(UP) + [(7, 7, 0)]
    modgpu.rekey_relayout_table_validate(_table(modgpu, holes))
    modgpu.rekey_relayout_table_validate(modgpu.rekey_table(0))
    modgpu.rekey_relayout_table_validate(modgpu.rekey_table(3))  # all empty
    # every table the move table call's validator takes
    for rows in (DOWN, UP, DOWN[:1], UP[:1], [(5, 5, 9)], [(5, 5, 9), (14, 14, 1), (15, 16, 3)], [(5, 5, 9), (14, 14, 1), (16, 15, 3)],
                 [(0, 0, 0), DOWN[0], (9, 1 << 40, 0), DOWN[1], DOWN[2], (1 << 40, 3, 0)] + DOWN[3:] + [(7, 7, 0)]):
        modgpu.rekey_move_table_validate(_table(modgpu, rows))
        modgpu.rekey_relayout_table_validate(_table(modgpu, rows))


@pytest.mark.parametrize("what,rows,bad", [
    ("an upward entry whose destination runs into the next, downward, entry's", [(1100, 1000, 50), (1149, 1200, 50)], 1),
    ("falling order across a direction change", [(1200, 1300, 50), (1100, 1000, 50)], 1),
    ("falling order across the other direction change", DOWN[:2] + [far(UP)[1], far(UP)[0]], 3),
    ("overlapping sources across a direction change", [(1000, 1100, 50), (1300, 1149, 50)], 1),
    ("overlapping destinations inside one direction", DOWN[:1] + [(1049, 1200, 100)] + DOWN[2:] + far(UP), 1),
    ("a destination below the previous one across an empty entry", ALTERNATING[:2] + [(0, 0, 0), (1026, 1050, 9)], 3),
    ("a null source", DOWN[:4] + [(2000, 0, 10)] + far(UP), 4),
    ("a null destination", [(0, 1100, 50)] + DOWN[1:] + far(UP), 0),
    ("an entry of 1 TiB or more", DOWN + far(UP)[:2] + [(1 << 42, 1 << 41, 1 << 40)], 8),
])
def test_validate_names_the_entry_at_fault(modgpu, what, rows, bad):
    with pytest.raises(modgpu.ModGpuError, match=f"entry {bad}:") as e:
        modgpu.rekey_relayout_table_validate(_table(modgpu, rows))
    assert e.value.code == 1, what


def test_validate_flags_and_limits(modgpu):
    for field in ("flags", "reserved"):
        t = _table(modgpu, DOWN + far(UP))
        t[9][field] = 1
        t[7][field] = 1 << 31  # an entry that sweep 0 filters
        with pytest.raises(modgpu.ModGpuError, match="entry 7: nonzero flags or reserved"):
            modgpu.rekey_relayout_table_validate(t)
        t[2][field] = 1        # ... and a lower one that sweep 1 filters
        with pytest.raises(modgpu.ModGpuError, match="entry 2: nonzero flags or reserved"):
            modgpu.rekey_relayout_table_validate(t)
    L = modgpu.lib()
    assert L.modgpu_rekey_relayout_table_validate(None, 3) == 1 and L.modgpu_rekey_relayout_table_validate(None, 0) == 0
    assert L.modgpu_rekey_relayout_table_validate(_table(modgpu, DOWN).ctypes.data, MAX_ENTRIES + 1) == 1


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
    call = L.modgpu_rekey_relayout_table_device
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
    assert not t.any() and not ws.any()
    assert modgpu.path_stats()["gpu_launches"] == before["gpu_launches"]


def test_splice_moves(modgpu):
    sp = modgpu.splice_moves
    # a growing edit first: everything behind it slides up, until the shrinking edit takes more back
    assert sp(1000, [(100, 10, 50), (300, 100, 20), (600, 30, 0)]) == (
        [(0, 0, 100), (110, 150, 190), (400, 360, 200), (630, 560, 370)], 930, [(100, 50), (340, 20)])
    # a deletion alone: one stationary segment and one that slides down
    assert sp(1000, [(200, 300, 0)]) == ([(0, 0, 200), (500, 200, 500)], 700, [])
    # adjacent edits leave no segment between them; an edit at offset 0 and one up to the end leave none outside
    assert sp(1000, [(0, 100, 7), (100, 50, 60), (150, 0, 5), (900, 100, 1)]) == ([(150, 72, 750)], 823, [(0, 7), (7, 60), (67, 5), (822, 1)])
    # an insertion: nothing goes away
    assert sp(10, [(4, 0, 3)]) == ([(0, 0, 4), (4, 7, 6)], 13, [(4, 3)])
    assert sp(1000, []) == ([(0, 0, 1000)], 1000, []) and sp(0, []) == ([], 0, [])
    for edits in ([(100, 50, 1), (149, 5, 1)], [(300, 10, 1), (100, 10, 1)], [(990, 20, 0)], [(10, -1, 0)]):
        with pytest.raises(ValueError):
            sp(1000, edits)


def test_relayout_table(modgpu):
    moves = [(0, 0, 100), (110, 150, 190), (400, 360, 200), (630, 560, 0)]
    t = modgpu.relayout_table(1 << 30, moves, modgpu.KEY_PS4, part_off=7)
    assert [int(x) - (1 << 30) for x in t["src"]] == [0, 110, 400, 630] and [int(x) - (1 << 30) for x in t["dst"]] == [0, 150, 360, 560]
    assert [int(x) for x in t["n"]] == [100, 190, 200, 0]
    assert [int(x) for x in t["off_from"]] == [7, 117, 407, 637] and [int(x) for x in t["off_to"]] == [7, 157, 367, 567]
    assert set(t["key_from"]) == set(t["key_to"]) == {modgpu.as_int32(modgpu.KEY_PS4)} and not t["flags"].any() and not t["reserved"].any()
    modgpu.rekey_relayout_table_validate(t)
    with pytest.raises(modgpu.ModGpuError, match="entry 2:"):
        modgpu.rekey_move_table_validate(t)
    t = modgpu.relayout_table(1 << 30, moves[:2], modgpu.KEY_PS3, modgpu.KEY_PS4)
    assert set(t["key_from"]) == {modgpu.as_int32(modgpu.KEY_PS3)} and set(t["key_to"]) == {modgpu.as_int32(modgpu.KEY_PS4)}
    assert [int(x) for x in t["off_from"]] == [0, 110] and [int(x) for x in t["off_to"]] == [0, 150]
    assert modgpu.relayout_table(1 << 30, [], modgpu.KEY_PS4).size == 0
    # what a splice hands it
    moves, new_size, holes = modgpu.splice_moves(1000, [(100, 10, 50), (300, 100, 20)])
    modgpu.rekey_relayout_table_validate(modgpu.relayout_table(1 << 30, moves, modgpu.KEY_PS4))
    assert new_size == 960 and holes == [(100, 50), (340, 20)]


def test_codegen_guard_passes_and_the_standin_is_wired():
    B.isa_check_target("isa-check-rekey-move-table", 5)
    B.standin_is_wired("standin_launch_rekey_relayout_table.cpp")
    B.standin_is_wired("standin_launch_rekey_move_table.cpp")


def test_relayout_on_the_standin_under_asan_ubsan():
    """tests/rekey_relayout_table_main.cpp: the run patterns, the small alternating tables, empty entries between runs, every device
    refusal and every host refusal, every byte of the arena against a model, and the windows the stand-in planned."""
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "rekey-relayout-table-main"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", MODGPU_REQUIRE_GPU="0")
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "rekey_relayout_table_main")], env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1].endswith(", 0 failed") and int(lines[-1].split()[0]) == len(lines) - 1 > 150, lines[-1]
    for what in ("pattern DU phase 0", "pattern UD phase 1", "pattern DSU phase 7", "pattern UDUD phase 0", "pattern DDUUDD phase 7", "pattern DUD big up",
                 "pattern UDU big down", "pure down", "pure up", "alternating 64 x 9", "alternating 64 x 1000", "empty entries between the runs of DSU",
                 "device refusal: an upward entry's destination runs into the next, downward, entry's", "device refusal: falling order across a direction change",
                 "device refusal: nonzero flags on an entry sweep 0 filters", "device refusal: nonzero flags on an entry sweep 1 filters",
                 "device refusal: total_bytes enough for each sweep alone, too small for the table", "validator refusal: falling sources",
                 "validator refusal: overlapping destinations", "refusal: validate a null table", "refusal: short workspace",
                 "refusal: workspace that is not device memory", "launch plans: 0 window errors"):
        assert any(ln.startswith("ok   " + what) for ln in lines), what
