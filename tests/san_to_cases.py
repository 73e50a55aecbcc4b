"""Cases for the sanitizer builds of libmodgpu's host code: the OUT-OF-PLACE entry points (modgpu_cycle_device_to /
modgpu_cycle_batch_device_to).

Not collected by a plain `pytest tests/`: tests/test_cycle_to_cpu.py runs this file in a child process with MODGPU_LIB pointing at
_san/libmodgpu_asan.so or _san/libmodgpu_tsan.so and the matching runtime preloaded (the pattern of tests/test_sanitizers.py and
tests/san_lib_cases.py).  In those builds a launch executes the launch PLAN on the CPU (tests/cpu_runtime_standin/standin_launch_to.cpp):
it reads the source and writes the destination exactly where the plan says the kernel would, so the sanitizers see every byte, and
every case compares the destination with the oracle and checks that the source did not change."""
import ctypes
import os
import threading

import numpy as np
import pytest

import modulate_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not os.environ.get("MODGPU_LIB"), reason="runs only against a sanitizer build (tests/test_cycle_to_cpu.py)")

CHUNK = 65536
GUARD = 32


@pytest.fixture(scope="module")
def lib():
    L = M.lib()
    assert M.testing_hooks() and M.device_count() == 8, "expects the shim build with MODGPU_SHIM_DEVICES=8"
    for name in ("modgpu_shim_to_launches", "modgpu_shim_to_collisions", "modgpu_shim_to_plan_errors", "modgpu_shim_launches"):
        getattr(L, name).restype = ctypes.c_ulonglong
    yield L
    assert L.modgpu_shim_to_collisions() == 0 and L.modgpu_shim_to_plan_errors() == 0


def launches(lib):
    return lib.modgpu_shim_to_launches(0) + lib.modgpu_shim_to_launches(1)


def run(src, dst, pt, ps, pd, key, so=0, device=-1):
    n = pt.size
    s_img = np.full(src.nbytes, 0xA5, np.uint8)
    s_img[GUARD + ps:GUARD + ps + n] = pt
    d_img = np.full(dst.nbytes, 0x5A, np.uint8)
    src.upload(s_img)
    dst.upload(d_img)
    M.cycle_device_to(dst.ptr + GUARD + pd, src.ptr + GUARD + ps, n, key, so, device=device)
    dst.sync()
    want = d_img.copy()
    want[GUARD + pd:GUARD + pd + n] = pt
    O.cycle_at(want[GUARD + pd:GUARD + pd + n], key, so)
    assert np.array_equal(dst.download(), want), (n, ps, pd, hex(key), so)
    assert np.array_equal(src.download(), s_img), ("source changed", n, ps, pd)


def test_phase_grid(lib):
    """Every (src phase, dst phase) mod 16, at sizes around 0, one word, one chunk, and three chunks + 5."""
    sizes = [0, 15, 16, 17, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5]
    src, dst = M.DeviceBuffer(max(sizes) + 2 * GUARD + 16), M.DeviceBuffer(max(sizes) + 2 * GUARD + 16)
    rng = np.random.default_rng(3)
    before = launches(lib)
    for n in sizes:
        pt = rng.integers(0, 256, size=n, dtype=np.uint8)
        for ps in range(16):
            for pd in range(16):
                run(src, dst, pt, ps, pd, [0x90CFC0AB, 0xC64EED30, 12345][(ps + pd) % 3], so=n)
    assert launches(lib) - before == 256 * (len(sizes) - 1)  # one launch per non-empty call
    assert M.last_launch()["variant"] == 5
    src.free()
    dst.free()


def test_stream_offsets_near_2_32_and_2_64(lib):
    src, dst = M.DeviceBuffer(CHUNK + 200), M.DeviceBuffer(CHUNK + 200)
    pt = O.splitmix_bytes(CHUNK + 77, 9)
    for so in ((1 << 32) - 17, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 64) - CHUNK - 77, (1 << 64) - 3, O.PERIOD - 9):
        run(src, dst, pt, 7, 2, 0xC64EED30, so)
    src.free()
    dst.free()


def test_zero_residue_keys_copy(lib):
    src, dst = M.DeviceBuffer(3 * CHUNK + 200), M.DeviceBuffer(3 * CHUNK + 200)
    before = launches(lib)
    for key in (0, 0x7FFFFFFF, 0x80000001):
        for n, ps, pd in ((3 * CHUNK + 5, 5, 0), (17, 0, 9), (1, 3, 3)):
            run(src, dst, O.splitmix_bytes(n, n), ps, pd, key)
    assert launches(lib) == before, "an identity keystream is a copy, not a kernel"
    src.free()
    dst.free()


def test_exact_alias_is_the_in_place_call(lib):
    n = 3 * CHUNK + 5
    pt = O.splitmix_bytes(n + 64, 12)
    a, b = M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64)
    a.upload(pt)
    b.upload(pt)
    M.cycle_device_to(a.ptr + 3, a.ptr + 3, n, 0x90CFC0AB, 11)
    M.cycle_device(b.ptr + 3, n, 0x90CFC0AB, 11)
    a.sync()
    b.sync()
    assert np.array_equal(a.download(), b.download())
    with pytest.raises(M.ModGpuError) as e:
        M.cycle_device_to(a.ptr + 4, a.ptr + 3, n, 0x90CFC0AB)
    assert e.value.code == 1
    a.free()
    b.free()


def test_forty_entry_batch_takes_three_launches(lib):
    """40 files of one part, sources overlapping, destinations at every phase: 16 + 16 + 8 entries, three launches, in order."""
    part_n = 2 * CHUNK + 999
    pt = O.splitmix_bytes(part_n, 5)
    enc = pt.copy()
    O.cycle_at(enc, 0xC64EED30, 0)
    part = M.DeviceBuffer(part_n + 16)
    part.upload(enc, offset=3)
    rng = np.random.default_rng(40)
    sizes = [int(x) for x in rng.integers(0, CHUNK + 100, size=40)]
    sizes[7] = 0
    offs = [int(rng.integers(0, part_n - s + 1)) for s in sizes]
    out = M.DeviceBuffer(sum(sizes) + 32 * 40)
    dsts, at = [], 0
    for i, s in enumerate(sizes):
        at += i % 16
        dsts.append(out.ptr + at)
        at += s + 16 - i % 16
    before = launches(lib)
    M.cycle_batch_device_to(dsts, [part.ptr + 3 + o for o in offs], sizes, 0xC64EED30, stream_offs=offs)
    out.sync()
    assert launches(lib) - before == 3
    for i, (s, o) in enumerate(zip(sizes, offs)):
        assert np.array_equal(out.download(s, offset=dsts[i] - out.ptr), pt[o:o + s]), i
    assert np.array_equal(part.download(part_n, offset=3), enc)
    # a destination that meets another entry's source: the whole call is refused, nothing queued
    with pytest.raises(M.ModGpuError) as e:
        M.cycle_batch_device_to([dsts[0], part.ptr + 3], [part.ptr + 3, part.ptr + 100], [10, 10], 1)
    assert e.value.code == 1
    assert launches(lib) - before == 3
    part.free()
    out.free()


def test_eight_threads_at_once(lib):
    """Eight threads call at once, two per device, on the devices' null streams: the ticket ring, the per-thread launch record and
    the counters under ThreadSanitizer; every result bit-exact."""
    n = CHUNK + 333
    errors = []

    def worker(t):
        try:
            dev = t % 4
            src, dst = M.DeviceBuffer(n + 2 * GUARD + 16, device=dev), M.DeviceBuffer(n + 2 * GUARD + 16, device=dev)
            pt = O.splitmix_bytes(n, 100 + t)
            for k in range(4):
                run(src, dst, pt, (t + k) % 16, (3 * t + k) % 16, 0x90CFC0AB, so=t << 32, device=dev)
                assert M.last_launch()["variant"] == 5
            src.free()
            dst.free()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
