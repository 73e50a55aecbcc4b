"""CPU checks of the list transfers (modgpu_cycle_host_to_device_list, modgpu_cycle_device_to_host_list, include/modgpu.h): the symbols
are declared, exported by both library flavours and listed; the header is still plain C99; without a GPU every refusal the host alone
can see is MODGPU_ERR_INVALID and a valid list MODGPU_ERR_NO_DEVICE, with nothing launched and nothing computed on the host; the list
mode adds no kernel to the transfer TU; and the host code -- validation, the packed stream through the pipelines, the plan, failures, a
wedged kernel, two threads, the cut above the one-launch limit (windows inside long entries too), slots filled three times over at
chunks of one and two pieces, entries above 8 MiB, 70 000 entries -- runs clean under ASan + UBSan and under TSan on the CPU stand-in of
the HIP runtime, as a stand-alone program (tests/xfer_list_main.cpp: its own main, run directly, the sanitizer runtimes linked
statically: the environment's preloads are left alone)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
NEW = ("modgpu_cycle_host_to_device_list", "modgpu_cycle_device_to_host_list")


def test_new_symbols_declared_exported_and_listed(modgpu):
    header = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(const modgpu_table_entry_t \*host_entries, uint64_t n_entries, int device\);$" % name, header, re.M), name
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    assert set(NEW) <= set(modgpu.EXPORTS)
    assert modgpu.lib().modgpu_abi_version() == 8
    assert callable(modgpu.cycle_host_to_device_list) and callable(modgpu.cycle_device_to_host_list)
    assert all(hasattr(modgpu.DeviceBuffer, m) for m in ("upload_ranges", "download_ranges", "fill"))
    assert "`fill`" in modgpu.DeviceBuffer.splice.__doc__


def test_header_is_still_plain_c99(tmp_path):
    src = tmp_path / "x.c"
    src.write_text('#include "modgpu.h"\n#include "modgpu_testing.h"\n'
                   "int use(const modgpu_table_entry_t *t) {\n"
                   "  return modgpu_cycle_host_to_device_list(t, 0, -1) + modgpu_cycle_device_to_host_list(t, 0, -1)\n"
                   "       + (int)MODGPU_TUNABLE_XFER_LIST_MOST_BYTES;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "x.o")])


def test_list_mode_is_a_mode_of_the_four_transfer_kernels():
    """no new TU, no new __global__, no new instantiation: the list loop sits behind `if constexpr (FUNNEL)` in the one kernel template,
    its launch function takes the funnel instantiations, and its stand-in is a file of its own, wired into the sanitizer builds"""
    hip = open(os.path.join(CSRC, "cycle_xfer_kernel.hip")).read()
    assert hip.count("__global__") == 1 and hip.count("hipLaunchKernelGGL") == 1
    assert "if constexpr (FUNNEL)" in hip and "? (AUX_NT | AUX_SC1) : AUX_SC1;" in hip
    assert hip.count("XferShape<true, true>::launch") == 2 and hip.count("XferShape<false, true>::launch") == 2
    assert "xfer_list" not in B.make_var("TABLE") and "cycle_xfer_kernel.h" in B.make_var("XFER_SRC")
    B.standin_is_wired("standin_launch_xfer_list.cpp")
    standin = open(os.path.join(ROOT, "tests", "cpu_runtime_standin", "standin_launch_xfer_list.cpp")).read()
    assert "_impl.h" not in standin and "lcg.h" in standin  # a second implementation, from the record types and lcg.h


def test_validation_comes_before_the_device(modgpu):
    """Without a GPU: every refusal the host alone can see returns 1 and names the lowest entry at fault, a valid list returns
    MODGPU_ERR_NO_DEVICE, a list without bytes MODGPU_OK -- and nothing was launched or computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    a, b = np.arange(4096, dtype=np.uint8) % 251, np.full(4096, 0x3C, np.uint8)
    keep_a, keep_b = a.copy(), b.copy()
    before = modgpu.path_stats()

    def good():
        t = modgpu.table(4)
        for i in range(4):
            t[i]["dst"], t[i]["src"], t[i]["n"], t[i]["stream_off"], t[i]["key"] = b.ctypes.data + 1000 * i, a.ctypes.data + 1000 * i, 100 * i, i, 1 + i
        return t

    def err():
        return L.modgpu_last_error().decode()

    for call in (L.modgpu_cycle_host_to_device_list, L.modgpu_cycle_device_to_host_list):
        def run(t, n=None):
            return call(ctypes.c_void_p(t.ctypes.data), t.size if n is None else n, -1)
        assert call(None, 3, -1) == 1 and "NULL list" in err()
        assert run(good(), (1 << 22) + 1) == 1 and "more than 4194304 entries" in err()
        t = good()
        t["dst"][2] = 0
        assert run(t) == 1 and err().startswith("entry 2:") and "NULL pointer" in err()
        t = good()
        t["src"][1] = t["src"][3] = 0
        assert run(t) == 1 and err().startswith("entry 1:") and "NULL pointer" in err()
        t = good()
        t["flags"][0] = t["flags"][3] = 1  # (entry 0 is empty: its flags count all the same)
        assert run(t) == 1 and err().startswith("entry 0:") and "flags" in err()
        t = good()
        t["n"][3] = 1 << 39
        assert run(t) == 1 and err().startswith("entry 3:") and "2^39" in err()
        assert run(good()) == 2  # MODGPU_ERR_NO_DEVICE
        assert call(None, 0, -1) == 0
        t = good()
        t["n"][:] = 0
        t["dst"][:] = 0
        assert run(t) == 0  # a list with no bytes: nothing to queue, MODGPU_OK even without a device
    assert np.array_equal(a, keep_a) and np.array_equal(b, keep_b)
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] == 0 and st["scalar_calls"] == before["scalar_calls"] and st["gpu_calls"] == before["gpu_calls"]
    with pytest.raises(modgpu.ModGpuError) as e:  # the Python face: check=True runs table_validate first (two destinations that meet)
        t = good()
        t["dst"][3] = t["dst"][2]
        modgpu.cycle_host_to_device_list(t, check=True)
    assert e.value.code == 1


def _run_main(flavour, env_extra):
    env = dict(os.environ, MODGPU_REQUIRE_GPU="0", **env_extra)
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW", "MODGPU_HOST_PIPES", "MODGPU_HOST_CHUNK_MB"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "xfer_list_main_" + flavour)], env=env, capture_output=True, text=True, timeout=900)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1].endswith(", 0 failed") and int(lines[-1].split()[0]) == len(lines) - 1 == 67, lines[-1]
    whats = ["the chunk size from the host trace", "phases and sizes", "boundaries", "empty entries", "only empty entries", "no entries", "one byte",
             "same bytes as the single calls one by one, both ways", "shared sources, both ways", "refusals queued nothing and wrote nothing",
             "a good list after the refusals", "two threads at once on separate buffers", "cut above the one-launch limit: 7 launches",
             "cut above the one-launch limit, boundaries list", "one launch again with the limit back",
             "a wedged kernel: MODGPU_ERR_HIP within the host deadline, sources intact",
             # the lists of the GPU suite's long cases: slots filled three times over, the second jump table's entries, windows inside entries, > 65 535 records
             "cut at three pieces, phases and sizes", "cut at three pieces, boundaries list", "cut inside long entries: 7 launches",
             "entries longer than 8 MiB", "seventy thousand entries"]
    whats += [f"every slot refilled: feed chunk {knob}, chunks of {chunk}, {which}" for knob, chunk in ((32768, 32768), (65536, 32768), (131072, 65536))
              for which in ("phases and sizes", "boundaries")]
    for d in ("up", "down"):
        whats += [f"refusal {d}: {w}" for w in ("null list", "too many entries", "null dst", "null src, the lowest of two", "flags", "2^39 bytes",
                                                "host memory as the device side", "device range past its allocation",
                                                "a device side below a flagged entry", "a flagged entry below a device side",
                                                "a device that does not exist")]
        whats += [f"injected failure {d} piece {p} stage {s}" for p in (0, -2, -1) for s in (0, 1, 2)]
    for what in whats:
        assert any(ln.startswith(f"ok   {what}") for ln in lines), what


def test_list_transfers_on_the_standin_under_asan_ubsan():
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "../_san/xfer_list_main_asan"])
    _run_main("asan", {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})


def test_list_transfers_on_the_standin_under_tsan():
    if not B.sanitizer_runtime("libtsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "../_san/xfer_list_main_tsan"])
    _run_main("tsan", {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1 suppressions=" + os.path.join(ROOT, "tests", "tsan.supp")})
