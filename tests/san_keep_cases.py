"""Cases for the sanitizer builds of libmodgpu's host code: the KEEP route of a single in-place device buffer (cycle_keep_kernel.h).

Not collected by a plain `pytest tests/`: tests/test_keep_cpu.py runs this file in a child process with MODGPU_LIB pointing at
_san/libmodgpu_asan.so or _san/libmodgpu_tsan.so and the matching runtime preloaded (the pattern of tests/san_verify_cases.py).  In those
builds a launch executes the launch PLAN on the CPU (tests/cpu_runtime_standin/standin_launch_keep.cpp hands the plan to the work-queue
shape's stand-in and checks the policy), so the sanitizers see every byte the plan says the kernel touches; the bytes are compared with
the oracle's."""
import ctypes
import os
import threading

import numpy as np
import pytest

import modulate_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not os.environ.get("MODGPU_LIB"), reason="runs only against a sanitizer build (tests/test_keep_cpu.py)")

CHUNK = 65536
PS4 = M.KEY_PS4


@pytest.fixture(scope="module")
def lib():
    L = M.lib()
    assert M.testing_hooks() and M.device_count() == 8, "expects the shim build with MODGPU_SHIM_DEVICES=8"
    for name in ("modgpu_shim_keep_launches", "modgpu_shim_keep_kept", "modgpu_shim_keep_plan_errors", "modgpu_shim_batch_plan_errors"):
        getattr(L, name).restype = ctypes.c_ulonglong
    M.use_testing_flavour()
    M.DeviceBuffer(16).free()  # device preparation (its own tiny launches, two of them keep launches) happens here, not inside a case
    yield L
    M.debug_set_keep(0, 0, 0)
    M.debug_set_launch(None, 0)
    assert L.modgpu_shim_keep_plan_errors() == 0 and L.modgpu_shim_batch_plan_errors() == 0


def run(n, phase, off, policy):
    """one in-place call over n bytes at `phase` past the allocation's start, 64 guard bytes either side; returns the launch"""
    pt = O.splitmix_bytes(n, n + phase)
    buf = M.DeviceBuffer(n + phase + 128)
    img = np.full(n + 128, 0xA5, np.uint8)
    img[64:64 + n] = pt
    buf.upload(img, offset=phase)
    M.debug_set_keep(*policy)
    buf.cycle(PS4, n=n, offset=phase + 64, stream_off=off)
    buf.sync()
    info = M.last_launch()
    got = buf.download(n + 128, offset=phase)
    buf.free()
    assert (got[:64] == 0xA5).all() and (got[64 + n:] == 0xA5).all()
    assert np.array_equal(got[64:64 + n], O.cycle_at(pt.copy(), PS4, off)), (n, phase, off, policy)
    return info


def test_forced_policies_route_and_leave_the_bytes_alone(lib):
    M.debug_set_launch("queue", 0)
    before, kept = lib.modgpu_shim_keep_launches(), lib.modgpu_shim_keep_kept()
    for policy in ((1, 1, 0), (1, 1, 1), (1, 3, 1), (1, 3, 3), (1, 0, 1)):
        for n, phase, off in ((7 * CHUNK + 77, 5, 0), (3 * CHUNK + 1, 0, (1 << 33) + 12345), (100, 3, 9)):
            info = run(n, phase, off, policy)
            assert info["kernel"] == "shim keep" and info["variant"] == 2 and info["source_hash"] == M.keep_kernel_source_hash(), info
    assert lib.modgpu_shim_keep_launches() - before == 15 and lib.modgpu_shim_keep_kept() - kept == 12


def test_route_off_and_threshold(lib):
    M.debug_set_launch("queue", 0)
    before = lib.modgpu_shim_keep_launches()
    assert run(5 * CHUNK + 3, 1, 4, (M.KEEP_OFF, 1, 1))["kernel"] == "shim queue"
    assert run(5 * CHUNK + 3, 1, 4, (5 * CHUNK + 4, 1, 1))["kernel"] == "shim queue"   # one byte short of the forced threshold
    assert run(5 * CHUNK + 3, 1, 4, (5 * CHUNK + 3, 1, 1))["kernel"] == "shim keep"
    info = run(5 * CHUNK + 3, 1, 4, (0, 0, 0))  # the shipped rule: far below 1 GiB
    assert info["kernel"] == "shim queue" and info["source_hash"] == M.kernel_source_hash()
    assert lib.modgpu_shim_keep_launches() - before == 1
    # a batch never takes the route, whatever the hook says
    M.debug_set_keep(1, 3, 1)
    M.debug_set_batch(1)
    a, b = M.DeviceBuffer(2 * CHUNK), M.DeviceBuffer(3 * CHUNK)
    M.cycle_batch_device([a.ptr, b.ptr], [2 * CHUNK, 3 * CHUNK], PS4, device=0)
    a.sync()
    assert M.last_launch()["variant"] == 3 and M.last_launch()["kernel"] == "shim queue" and lib.modgpu_shim_keep_launches() - before == 1
    M.debug_set_batch(0)
    a.free()
    b.free()


def test_hook_and_launches_from_several_threads(lib):
    """the hook is set while other threads launch: every call sees one whole policy (TSan: no race on the three words)"""
    M.debug_set_launch("queue", 0)
    errors = []

    def worker(k):
        try:
            for i in range(6):
                info = run(2 * CHUNK + 17 * k + i, k, i, (1, 3, 1 + (i + k) % 3))
                assert info["variant"] == 2
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
