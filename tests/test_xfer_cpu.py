"""CPU checks of the transfer entry points (modgpu_cycle_host_to_device, modgpu_cycle_device_to_host, modgpu_cycle_file_to_device,
modgpu_cycle_device_to_file, include/modgpu.h): the symbols are in both library flavours, the header is still plain C99, the new TU has
a source hash of its own, its code-generation guard passes the tree and rejects a broken build, argument validation happens before any
device work, and the host code runs clean under ASan/UBSan and TSan against the CPU stand-in of the HIP runtime."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
NEW = ("modgpu_cycle_host_to_device", "modgpu_cycle_device_to_host", "modgpu_cycle_file_to_device", "modgpu_cycle_device_to_file")


def test_new_symbols_in_both_flavours(modgpu):
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NEW) | {"modgpu_xfer_kernel_source_hash"} <= names, (flavour, set(NEW) - names)
        assert ("modgpu_debug_set_xfer_form" in names) == (flavour == "testing")
    assert set(NEW) <= set(modgpu.EXPORTS) and "modgpu_xfer_kernel_source_hash" in modgpu.TESTING_EXPORTS
    assert modgpu.lib().modgpu_abi_version() == 8


def test_header_declares_them_as_plain_c99(tmp_path):
    src = tmp_path / "x.c"
    src.write_text('#include "modgpu.h"\n#include "modgpu_testing.h"\n'
                   "int use(void *d, const uint8_t *h, uint8_t *o) {\n"
                   "  return modgpu_cycle_host_to_device(d, h, 0, 1, 0, -1) + modgpu_cycle_device_to_host(o, d, 0, 1, 0, -1)\n"
                   "       + modgpu_cycle_file_to_device(\"p\", 0, d, 0, 1, 0, -1) + modgpu_cycle_device_to_file(d, 0, \"p\", 1, 0, -1)\n"
                   "       + (modgpu_xfer_kernel_source_hash() != 0);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "x.o")])


def test_xfer_kernel_source_hash_matches_its_sources(modgpu):
    h = hashlib.sha256()
    for f in ("cycle_xfer_kernel.hip", "cycle_xfer_kernel.h", "cycle_feed_kernel.h", "cycle_kernel_impl.h", "lcg.h"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    assert modgpu.xfer_kernel_source_hash() == h.hexdigest()
    assert len({modgpu.xfer_kernel_source_hash(), modgpu.to_kernel_source_hash(), modgpu.kernel_source_hash(),
                modgpu.feed_kernel_source_hash()}) == 4


def test_codegen_guard_of_the_new_tu():
    """`make isa-check-xfer` is the guard's pass over the transfer TU (4 kernels); the TU with the download's stores across PCIe made
    nt is REJECTED; the object waits for its own guard run, which ISA_CHECK=0 leaves out; the stand-in is wired.
    (`make isa-check` as a whole: tests/test_capi_cpu.py.)"""
    B.isa_check_target("isa-check-xfer", 4)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-xfer"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted nt stores across PCIe in the download kernel"
    assert "a download store across PCIe is not `sc1` without nt" in broken.stdout, broken.stdout[-3000:]
    B.guard_then_compile("cycle_xfer_kernel")
    B.unguarded_plan("cycle_xfer_kernel")
    B.standin_is_wired("standin_launch_xfer.cpp")


def test_validation_comes_before_the_device(modgpu, tmp_path):
    """Without a GPU: NULL with n > 0 is MODGPU_ERR_INVALID, n == 0 does nothing, every valid call is MODGPU_ERR_NO_DEVICE -- nothing is
    computed on the host.  (A host pointer passed as the device side needs a device to be told apart: tests/san_xfer_cases.py.)"""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    import ctypes
    L = modgpu.lib()
    b = np.arange(256, dtype=np.uint8)
    keep = b.copy()
    p = ctypes.c_void_p(b.ctypes.data)
    before = modgpu.path_stats()
    assert L.modgpu_cycle_host_to_device(None, p, 10, 1, 0, -1) == 1
    assert L.modgpu_cycle_host_to_device(p, None, 10, 1, 0, -1) == 1
    assert L.modgpu_cycle_device_to_host(None, p, 10, 1, 0, -1) == 1
    assert L.modgpu_cycle_device_to_host(p, None, 10, 1, 0, -1) == 1
    assert L.modgpu_cycle_file_to_device(None, 0, p, 10, 1, 0, -1) == 1
    assert L.modgpu_cycle_file_to_device(str(tmp_path / "none").encode(), 0, None, 10, 1, 0, -1) == 1
    assert L.modgpu_cycle_device_to_file(None, 10, str(tmp_path / "o").encode(), 1, 0, -1) == 1
    for rc in (L.modgpu_cycle_host_to_device(None, None, 0, 1, 0, -1), L.modgpu_cycle_device_to_host(None, None, 0, 1, 0, -1)):
        assert rc == 0
    assert L.modgpu_cycle_host_to_device(ctypes.c_void_p(b.ctypes.data + 128), p, 10, 1, 0, -1) == 2
    assert L.modgpu_cycle_device_to_host(p, ctypes.c_void_p(b.ctypes.data + 128), 10, 1, 0, -1) == 2
    assert np.array_equal(b, keep)
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] == 0 and st["scalar_calls"] == before["scalar_calls"]


def test_transfer_host_code_under_asan_ubsan():
    B.run_sanitized_cases("san_xfer_cases.py", "asan", "14 passed")


def test_transfer_host_code_under_tsan():
    B.run_sanitized_cases("san_xfer_cases.py", "tsan", "14 passed")
