"""CPU checks of what the five table calls share on the host (modulate_amd/csrc/modgpu_capi.cpp: one workspace walk, one call body)
and in the stand-ins (tests/cpu_runtime_standin/standin_table.h): every workspace size against the sizes recorded from the commit
before the shared walk, and the four three-launch calls driven on the CPU stand-in of the HIP runtime by a stand-alone program under
ASan + UBSan (its own main, run directly, the sanitizer runtimes linked statically: the environment's preloads are left alone)."""
import json
import os
import subprocess

import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")


def test_workspace_bytes_are_the_recorded_ones(modgpu):
    """tests/golden/table_workspace_bytes.json: every offset of every layout adds up to what it was before the layouts shared a walk"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "table_workspace_bytes.json")))
    ns, bs = gold["n_entries"], gold["total_bytes"]
    assert len(ns) == 16 and len(bs) == 8 and ns[-1] == 1 << 22
    for name in ("table", "rekey_table", "verify_table", "verify_rekey_table"):
        got = {str(n): getattr(modgpu, name + "_workspace_bytes")(n) for n in ns}
        assert got == gold[name], name
    got = {str(n): {str(b): modgpu.rekey_move_table_workspace_bytes(n, b) for b in bs} for n in ns}
    assert got == gold["rekey_move_table"]


def test_shared_pieces_exist_once():
    capi = open(os.path.join(CSRC, "modgpu_capi.cpp")).read()
    assert capi.count("if (cnt <= 16) break;") == 1
    assert capi.count('"more than 4194304 entries') == 3  # the call body, and the two validators' own copies
    assert capi.count('"null table or workspace"') == 1 and capi.count("hipEventElapsedTime(") == 1
    standin = os.path.join(ROOT, "tests", "cpu_runtime_standin")
    texts = {f: open(os.path.join(standin, f)).read() for f in os.listdir(standin) if f.endswith((".cpp", ".h"))}
    assert [f for f, t in texts.items() if "(16 - (d & 15)) & 15" in t] == ["standin_table.h"]
    # the stand-ins stay a second implementation: the shared header is written from the record types and lcg.h, not from the device code
    assert "_impl.h" not in texts["standin_table.h"].split("#pragma once")[1]
    assert "standin_table.h" in B.make_var("SHIM_DEPS")


def test_table_calls_on_the_standin_under_asan_ubsan():
    """tests/table_calls_main.cpp: every entry size at every phase, the degenerate keys, table lengths across the level and record
    edges, planted mismatches, every device refusal and every host refusal with its text, every byte of the arena and every result
    against a model."""
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "table-calls-main"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", MODGPU_REQUIRE_GPU="0")
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "table_calls_main")], env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1].endswith(", 0 failed") and int(lines[-1].split()[0]) == len(lines) - 1 == 194, lines[-1]
    for call in ("cycle table", "rekey table", "verify table", "verify rekey table"):
        for what in ("sizes at dst phase 0+0 src phase 0", "sizes at dst phase 65520+15 src phase 3", "length 1 ", "length 16 ", "length 17 ", "length 1024 ",
                     "length 1025 ", "length 4097 ", "empty entries only", "device refusal: a null source", "device refusal: a null destination",
                     "device refusal: nonzero flags", "device refusal: an entry of 1 TiB", "refusal: too many entries", "refusal: null table",
                     "refusal: misaligned workspace", "refusal: short workspace", "refusal: workspace that is not device memory",
                     "refusal: status of host memory", "refusal: timing without iterations", "refusals queued nothing"):
            assert any(ln.startswith(f"ok   {call}: {what}") for ln in lines), (call, what)
    for call in ("verify table", "verify rekey table"):
        for what in ("nothing planted", "refusal: null results", "refusal: misaligned results", "refusal: results that are not device memory",
                     "refusal: summary of host memory"):
            assert any(ln.startswith(f"ok   {call}: {what}") for ln in lines), (call, what)
    for call in ("rekey table", "verify rekey table"):
        assert any(ln.startswith(f"ok   {call}: device refusal: nonzero reserved") for ln in lines), call
    assert lines[-2].startswith("ok   launches: ")


def test_a_null_device_table_is_refused_not_taken_for_an_empty_one(modgpu):
    """A table in device memory whose address is NULL -- a DeviceBuffer already freed, or None -- reaches the library with its n and is
    refused there (tier 1, before any device work); only an empty HOST table is a call with nothing to do."""
    import numpy as np
    freed = object.__new__(modgpu.DeviceBuffer)  # as DeviceBuffer.free() leaves one (made without a device)
    freed.nbytes, freed.device, freed.ptr = 4096, -1, None
    ws = np.zeros(1 << 16, np.uint64)
    res = np.zeros(4 * 3, np.uint64)
    before = modgpu.path_stats()["gpu_launches"]
    for table in (freed, None):
        for call in (modgpu.cycle_table_device, modgpu.rekey_table_device):
            with pytest.raises(modgpu.ModGpuError, match="null table or workspace"):
                call(table, ws.ctypes.data, n=3)
        with pytest.raises(modgpu.ModGpuError, match="null table or workspace"):
            modgpu.rekey_move_table_device(table, 1 << 20, ws.ctypes.data, n=3)
        for call in (modgpu.verify_table_device, modgpu.verify_rekey_table_device):
            with pytest.raises(modgpu.ModGpuError, match="null table or workspace"):
                call(table, res.ctypes.data, ws.ctypes.data, n=3)
    assert modgpu.path_stats()["gpu_launches"] == before and not ws.any() and not res.any()
    # ... while a host table without entries is done at once, whatever the other arguments
    assert modgpu.cycle_table_device(modgpu.table(0)) is None and modgpu.rekey_table_device(modgpu.rekey_table(0)) is None
    assert modgpu.rekey_move_table_device(modgpu.rekey_table(0)) is None
    assert modgpu.verify_table_device(modgpu.table(0)).size == 0 and modgpu.verify_rekey_table_device(modgpu.rekey_table(0)).size == 0
