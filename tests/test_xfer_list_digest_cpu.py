"""CPU checks of the digesting list transfers (modgpu_cycle_host_to_device_list_digest, modgpu_cycle_device_to_host_list_digest,
include/modgpu.h): the symbols are declared, exported by both library flavours and listed; the header is still plain C99; without a
GPU every refusal the host alone can see is MODGPU_ERR_INVALID with its text and a valid list MODGPU_ERR_NO_DEVICE, with nothing launched
and nothing computed on the host; the digest mode adds no kernel to the transfer TU, the guard passes the tree and rejects a returning
atomic; and the host code -- the records' refusals, their initialisation, the digest records of every window, a failure in the middle --
runs clean under ASan + UBSan and under TSan on the CPU stand-in of the HIP runtime, as a stand-alone program
(tests/xfer_list_digest_main.cpp: its own main, run directly, the sanitizer runtimes linked statically: the environment's preloads are
left alone), every record against the Adler-32 of a model."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
NEW = ("modgpu_cycle_host_to_device_list_digest", "modgpu_cycle_device_to_host_list_digest")


def test_new_symbols_declared_exported_and_listed(modgpu):
    header = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(const modgpu_table_entry_t \*host_entries, uint64_t n_entries, uint32_t side,\s+"
                         r"modgpu_digest_result_t \*dev_records, int device\);$" % name, header, re.M), name
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NEW) <= names, (flavour, set(NEW) - names)
    assert set(NEW) <= set(modgpu.EXPORTS)
    assert modgpu.lib().modgpu_abi_version() == 8  # exports only added
    assert callable(modgpu.cycle_host_to_device_list_digest) and callable(modgpu.cycle_device_to_host_list_digest)
    assert all(hasattr(modgpu.DeviceBuffer, m) for m in ("upload_ranges_digest", "download_ranges_checked"))


def test_header_is_still_plain_c99(tmp_path):
    src = tmp_path / "x.c"
    src.write_text('#include "modgpu.h"\n'
                   "int use(const modgpu_table_entry_t *t, modgpu_digest_result_t *r) {\n"
                   "  return modgpu_cycle_host_to_device_list_digest(t, 0, MODGPU_DIGEST_INPUT, r, -1)\n"
                   "       + modgpu_cycle_device_to_host_list_digest(t, 0, MODGPU_DIGEST_OUTPUT, r, -1);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "x.o")])


def test_digest_mode_is_a_mode_of_the_funnel_kernels_and_the_guard_holds_it():
    """no new TU, __global__ or instantiation: the digest launch delegates to the list launch inside the HIP TU; the sum helpers are
    restated there (the TU keeps its five files); the guard passes the tree with 4 kernels and rejects the sums' atomic made returning;
    the stand-in is a file of its own, a second implementation, wired into the sanitizer builds"""
    hip = open(os.path.join(CSRC, "cycle_xfer_kernel.hip")).read()
    assert hip.count("__global__") == 1 and hip.count("hipLaunchKernelGGL") == 1
    assert hip.count("XferShape<true, true>::launch") == 2 and hip.count("XferShape<false, true>::launch") == 2
    assert "cycle_table_impl.h" not in hip and "v_mov_b32 %0, 0x01010101" in hip
    assert re.search(r"modgpu_launch_cycle_xfer_list_digest\([^)]*\)\s*\{[^}]*return modgpu_launch_cycle_xfer_list\(a, upload, grid, stream\);", hip)
    assert B.make_var("XFER_SRC").split() == ["cycle_xfer_kernel.hip", "cycle_xfer_kernel.h", "cycle_feed_kernel.h", "cycle_kernel_impl.h", "lcg.h"]
    h = open(os.path.join(CSRC, "cycle_xfer_kernel.h")).read()
    assert "constexpr int CYCLE_XFER_LIST_DIGEST = 22;" in h
    B.isa_check_target("isa-check-xfer", 4)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-xfer-digest"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a returning atomic in the list digest mode"
    assert "a 64-bit atomic returns its value (sc0): the list digest mode's sums are non-returning" in broken.stdout, broken.stdout[-3000:]
    B.standin_is_wired("standin_launch_xfer_list_digest.cpp")
    standin = open(os.path.join(ROOT, "tests", "cpu_runtime_standin", "standin_launch_xfer_list_digest.cpp")).read()
    assert "_impl.h" not in standin and "lcg.h" in standin and "standin_launch_xfer_list.cpp\"" not in standin


def test_validation_comes_before_the_device(modgpu):
    """Without a GPU: every refusal the host alone can see returns 1 with its text, a valid list -- one without bytes too, whose records
    would still be written -- MODGPU_ERR_NO_DEVICE, no entries MODGPU_OK, and nothing was launched or computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    a, b = np.arange(4096, dtype=np.uint8) % 251, np.full(4096, 0x3C, np.uint8)
    records = np.full(4 * 32 + 8, 0xA7, np.uint8)
    rp = records.ctypes.data + (-records.ctypes.data % 8)
    keep_a, keep_b, keep_r = a.copy(), b.copy(), records.copy()
    before = modgpu.path_stats()

    def good():
        t = modgpu.table(4)
        for i in range(4):
            t[i]["dst"], t[i]["src"], t[i]["n"], t[i]["stream_off"], t[i]["key"] = b.ctypes.data + 1000 * i, a.ctypes.data + 1000 * i, 100 * i, i, 1 + i
        return t

    def err():
        return L.modgpu_last_error().decode()

    for call in (L.modgpu_cycle_host_to_device_list_digest, L.modgpu_cycle_device_to_host_list_digest):
        def run(t, n=None, side=0, r=rp):
            return call(ctypes.c_void_p(t.ctypes.data), t.size if n is None else n, side, ctypes.c_void_p(r), -1)
        assert call(None, 3, 0, ctypes.c_void_p(rp), -1) == 1 and "NULL list" in err()
        assert run(good(), (1 << 22) + 1) == 1 and "more than 4194304 entries" in err()
        assert run(good(), r=0) == 1 and "NULL records with n_entries > 0" in err()
        assert run(good(), r=rp + 4) == 1 and "the records are not 8-byte aligned" in err()
        assert run(good(), side=2) == 1 and "a side other than output (0) and input (1)" in err()
        t = good()
        t["dst"][2] = 0
        assert run(t) == 1 and err().startswith("entry 2:") and "NULL pointer" in err()
        t = good()
        t["src"][1] = t["src"][3] = 0
        assert run(t, side=1) == 1 and err().startswith("entry 1:") and "NULL pointer" in err()
        t = good()
        t["flags"][0] = t["flags"][3] = 1
        assert run(t) == 1 and err().startswith("entry 0:") and "flags" in err()
        t = good()
        t["n"][3] = 1 << 39
        assert run(t) == 1 and err().startswith("entry 3:") and "2^39" in err()
        assert run(good()) == 2 and run(good(), side=1) == 2  # MODGPU_ERR_NO_DEVICE
        assert call(None, 0, 7, None, -1) == 0  # no entries: nothing is looked at
        t = good()
        t["n"][:] = 0
        t["dst"][:] = 0
        assert run(t) == 2  # a list with no bytes still writes its records: it needs the device
    assert np.array_equal(a, keep_a) and np.array_equal(b, keep_b) and np.array_equal(records, keep_r)
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] == 0 and st["scalar_calls"] == before["scalar_calls"] and st["gpu_calls"] == before["gpu_calls"]
    with pytest.raises(modgpu.ModGpuError) as e:  # the Python face: check=True runs table_validate first (two destinations that meet)
        t = good()
        t["dst"][3] = t["dst"][2]
        modgpu.cycle_host_to_device_list_digest(t, records=rp, check=True)
    assert e.value.code == 1


def _run_main(flavour, env_extra):
    env = dict(os.environ, MODGPU_REQUIRE_GPU="0", **env_extra)
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW", "MODGPU_HOST_PIPES", "MODGPU_HOST_CHUNK_MB"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "xfer_list_digest_main_" + flavour)], env=env, capture_output=True, text=True, timeout=900)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1].endswith(", 0 failed") and int(lines[-1].split()[0]) == len(lines) - 1 == 58, lines[-1]
    whats = ["the chunk size from the host trace", "only empty entries: records written, nothing launched", "refusals queued nothing and wrote nothing",
             "a good list after the refusals", "the call twice on the same records: the same records", "injected failure at a middle chunk, up",
             "injected failure at a middle chunk, down", "cut inside long entries"]
    for case in ("phases and sizes", "boundaries", "every source byte 0xFF", "the position wraps twice", "ten thousand tiny entries", "empty entries",
                 "entries longer than 8 MiB", "no entries", "cut into windows of 300000: 7 launches, a clipped entry",
                 "cut into windows of 98304: 19 launches, a clipped entry", "one launch again with the limit back"):
        whats += [f"{case}, side output", f"{case}, side input"]
    for d in ("up", "down"):
        whats += [f"refusal {d}: {w}" for w in ("null list", "too many entries", "null records", "misaligned records", "a third side", "host memory as records",
                                                "records past their allocation", "records inside an entry's device range", "null dst", "flags",
                                                "2^39 bytes", "host memory as the device side", "a device that does not exist")]
        whats.append(f"no entries {d}: nothing touched")
    for what in whats:
        assert any(ln.startswith(f"ok   {what}") for ln in lines), what


def test_digesting_list_transfers_on_the_standin_under_asan_ubsan():
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "../_san/xfer_list_digest_main_asan"])
    _run_main("asan", {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})


def test_digesting_list_transfers_on_the_standin_under_tsan():
    if not B.sanitizer_runtime("libtsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "../_san/xfer_list_digest_main_tsan"])
    _run_main("tsan", {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1 suppressions=" + os.path.join(ROOT, "tests", "tsan.supp")})
