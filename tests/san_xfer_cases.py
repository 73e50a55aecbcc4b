"""Cases for the sanitizer builds of libmodgpu's host code: the TRANSFER entry points (modgpu_cycle_host_to_device,
modgpu_cycle_device_to_host, modgpu_cycle_file_to_device, modgpu_cycle_device_to_file).

Not collected by a plain `pytest tests/`: tests/test_xfer_cpu.py runs this file in a child process with MODGPU_LIB pointing at
_san/libmodgpu_asan.so or _san/libmodgpu_tsan.so and the matching runtime preloaded (the pattern of tests/test_cycle_to_cpu.py).  In
those builds a launch runs the transfer kernels' protocol on the CPU (tests/cpu_runtime_standin/standin_launch_xfer.cpp) while the
library's pipelines fill and drain their slots, so the sanitizers see every byte; "device memory" is what modgpu_shim_xfer_alloc
hands out.  Every case compares the destination with the oracle, checks the guard bytes around it and that the source did not change."""
import ctypes
import mmap
import os
import threading
import time

import numpy as np
import pytest

import modulate_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not os.environ.get("MODGPU_LIB"), reason="runs only against a sanitizer build (tests/test_xfer_cpu.py)")

CHUNK = 128 << 10  # a host-fed call's chunk up to 8 MiB (half of the 256 KiB feed chunk)
GUARD = 32
KEYS = [0x90CFC0AB, 0xC64EED30, 12345]


@pytest.fixture(scope="module")
def lib():
    with M.testing_flavour():  # (the modgpu_debug_* hooks; MODGPU_LIB is the sanitizer build either way)
        L = M.lib()
        assert M.testing_hooks() and M.device_count() == 8, "expects the shim build with MODGPU_SHIM_DEVICES=8"
        L.modgpu_shim_xfer_alloc.restype = ctypes.c_void_p
        L.modgpu_shim_xfer_alloc.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
        L.modgpu_shim_xfer_free.argtypes = [ctypes.c_void_p]
        for name in ("modgpu_shim_xfer_launches", "modgpu_shim_xfer_gave_up", "modgpu_shim_to_launches"):
            getattr(L, name).restype = ctypes.c_ulonglong
        L.modgpu_shim_wedge_next_xfer.argtypes = [ctypes.c_int]
        try:
            yield L
        finally:
            M.debug_set_xfer_form(None)
            M.debug_inject_failure_at(0, -1)


class Dev:
    """'device memory' of the stand-in: registered with it, read and written here through a numpy view"""

    def __init__(self, lib, n, device=0):
        self.lib, self.n = lib, n
        self.ptr = lib.modgpu_shim_xfer_alloc(n, device)
        self.a = np.ctypeslib.as_array(ctypes.cast(self.ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(n,))

    def free(self):
        self.a = None
        self.lib.modgpu_shim_xfer_free(self.ptr)


def launches(lib):
    return lib.modgpu_shim_xfer_launches(0) + lib.modgpu_shim_xfer_launches(1)


def want_of(pt, key, so):
    w = pt.copy()
    return O.cycle_at(w, key, so)


def upload(lib, dev, host, pt, ph, pd, key, so=0, device=-1, alone=True):
    """pt at host[GUARD + ph], uploaded to dev[GUARD + pd]; returns nothing, asserts everything"""
    n = pt.size
    host[:] = 0xA5
    host[GUARD + ph:GUARD + ph + n] = pt
    keep = np.array(host, copy=True)
    dev.a[:] = 0x5A
    before = launches(lib)
    src = host[GUARD + ph:GUARD + ph + n]
    M.cycle_host_to_device(dev.ptr + GUARD + pd, src, key, so, device=device)
    want = np.full(dev.n, 0x5A, np.uint8)
    want[GUARD + pd:GUARD + pd + n] = want_of(pt, key, so)
    assert np.array_equal(dev.a, want), ("upload", n, ph, pd, hex(key), so)
    assert np.array_equal(np.asarray(host), keep), ("upload changed its source", n, ph, pd)
    assert not alone or launches(lib) - before == 1  # (alone: no other thread launches meanwhile)


def download(lib, dev, host, pt, ph, pd, key, so=0, device=-1, alone=True):
    n = pt.size
    dev.a[:] = 0xA5
    dev.a[GUARD + pd:GUARD + pd + n] = pt
    keep = dev.a.copy()
    host[:] = 0x5A
    before = launches(lib)
    M.cycle_device_to_host(host[GUARD + ph:GUARD + ph + n], dev.ptr + GUARD + pd, key, so, device=device)
    want = np.full(host.size, 0x5A, np.uint8)
    want[GUARD + ph:GUARD + ph + n] = want_of(pt, key, so)
    assert np.array_equal(np.asarray(host), want), ("download", n, ph, pd, hex(key), so)
    assert np.array_equal(dev.a, keep), ("download changed its source", n, ph, pd)
    assert not alone or launches(lib) - before == 1


SIZES = [1, 15, 16, 17, CHUNK - 1, CHUNK + 1, 5 * CHUNK + 7]


def test_pageable_phase_grid(lib):
    """Both directions from / to pageable memory: sizes around one word, one chunk and several chunks, every destination phase mod 16."""
    big = max(SIZES) + 2 * GUARD + 16
    dev, host = Dev(lib, big), np.empty(big, np.uint8)
    rng = np.random.default_rng(1)
    for n in SIZES:
        pt = rng.integers(0, 256, size=n, dtype=np.uint8)
        for ph in range(16):
            upload(lib, dev, host, pt, (ph * 7) % 16, ph, KEYS[ph % 3], so=n)
            download(lib, dev, host, pt, ph, (ph * 5) % 16, KEYS[(ph + 1) % 3], so=3 * n)
    assert M.last_launch()["variant"] == 6 and M.last_launch()["source_hash"] == M.xfer_kernel_source_hash()
    dev.free()


def test_page_locked_phase_grid(lib):
    """Page-locked caller memory: one launch straight on the caller's pages, no slots; every phase pair's residue mod 16."""
    big = 3 * CHUNK + 2 * GUARD + 16
    dev, pin = Dev(lib, big), M.PinnedBuffer(big)
    assert pin.pinned
    rng = np.random.default_rng(2)
    before = M.host_pool_stats()
    for n in (1, 17, CHUNK + 1, 3 * CHUNK):
        pt = rng.integers(0, 256, size=n, dtype=np.uint8)
        for ph in range(16):
            upload_pinned(lib, dev, pin, pt, ph, (ph * 3 + 1) % 16, KEYS[ph % 3], so=ph)
            download_pinned(lib, dev, pin, pt, (ph * 5) % 16, ph, KEYS[(ph + 2) % 3], so=ph << 20)
    assert M.host_pool_stats()["pipelines_run_by_workers"] == before["pipelines_run_by_workers"], "a page-locked transfer runs no pipelines"
    pin.free()
    dev.free()


def upload_pinned(lib, dev, pin, pt, ph, pd, key, so):
    n = pt.size
    pin.array[:] = 0xA5
    pin.array[GUARD + ph:GUARD + ph + n] = pt
    keep = pin.array.copy()
    dev.a[:] = 0x5A
    before = launches(lib)
    lib_rc = M.lib().modgpu_cycle_host_to_device(ctypes.c_void_p(dev.ptr + GUARD + pd), ctypes.c_void_p(pin.ptr + GUARD + ph), n, M.as_int32(key), so, -1)
    assert lib_rc == 0, M.lib().modgpu_last_error()
    want = np.full(dev.n, 0x5A, np.uint8)
    want[GUARD + pd:GUARD + pd + n] = want_of(pt, key, so)
    assert np.array_equal(dev.a, want) and np.array_equal(pin.array, keep), ("pinned upload", n, ph, pd)
    assert launches(lib) - before == 1


def download_pinned(lib, dev, pin, pt, ph, pd, key, so):
    n = pt.size
    dev.a[:] = 0xA5
    dev.a[GUARD + pd:GUARD + pd + n] = pt
    keep = dev.a.copy()
    pin.array[:] = 0x5A
    before = launches(lib)
    lib_rc = M.lib().modgpu_cycle_device_to_host(ctypes.c_void_p(pin.ptr + GUARD + ph), ctypes.c_void_p(dev.ptr + GUARD + pd), n, M.as_int32(key), so, -1)
    assert lib_rc == 0, M.lib().modgpu_last_error()
    want = np.full(pin.nbytes, 0x5A, np.uint8)
    want[GUARD + ph:GUARD + ph + n] = want_of(pt, key, so)
    assert np.array_equal(pin.array, want) and np.array_equal(dev.a, keep), ("pinned download", n, ph, pd)
    assert launches(lib) - before == 1


def test_read_only_mapping_is_never_written(lib):
    """A PROT_READ mapping as the upload's source: any write to it would fault (the call would not return)."""
    n = 3 * CHUNK + 11
    pt = O.splitmix_bytes(n, 7)
    m = mmap.mmap(-1, n + 4096, prot=mmap.PROT_READ | mmap.PROT_WRITE)
    m[5:5 + n] = pt.tobytes()
    libc = ctypes.CDLL(None, use_errno=True)
    addr = ctypes.addressof(ctypes.c_char.from_buffer(m))
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(ctypes.c_void_p(addr), n + 4096, mmap.PROT_READ) == 0
    dev = Dev(lib, n + 64)
    try:
        rc = M.lib().modgpu_cycle_host_to_device(ctypes.c_void_p(dev.ptr + 9), ctypes.c_void_p(addr + 5), n, M.as_int32(0xC64EED30), 77, -1)
        assert rc == 0, M.lib().modgpu_last_error()
        assert np.array_equal(dev.a[9:9 + n], want_of(pt, 0xC64EED30, 77))
        assert np.array_equal(np.frombuffer(ctypes.string_at(addr + 5, n), np.uint8), pt)
        M.cycle_host_to_device(dev.ptr + 1, pt.tobytes(), 0x90CFC0AB, 5)  # a bytes object: read-only in Python too
        assert np.array_equal(dev.a[1:1 + n], want_of(pt, 0x90CFC0AB, 5))
    finally:
        assert libc.mprotect(ctypes.c_void_p(addr), n + 4096, mmap.PROT_READ | mmap.PROT_WRITE) == 0
        m.close()
        dev.free()


def test_file_endpoints(lib, tmp_path):
    """A part file as the upload's source (at a file offset) and as the download's destination (created, truncated, 0644)."""
    n = 4 * CHUNK + 333
    pt = O.splitmix_bytes(n + 100, 8)
    part = tmp_path / "part.bin"
    part.write_bytes(pt.tobytes())
    dev = Dev(lib, n + 164)
    for off, pd in ((0, 0), (100, 7), (37, 13)):
        m = n + 100 - off
        dev.a[:] = 0x5A
        M.cycle_file_to_device(str(part), dev.ptr + pd, m, 0xC64EED30, file_off=off, stream_off=off)
        assert np.array_equal(dev.a[pd:pd + m], want_of(pt[off:], 0xC64EED30, off)) and (dev.a[pd + m:] == 0x5A).all()
    assert part.read_bytes() == pt.tobytes()
    out = tmp_path / "out.bin"
    out.write_bytes(b"x" * (3 * n))  # longer than what is written: truncated
    dev.a[3:3 + n] = pt[:n]
    keep = dev.a.copy()
    M.cycle_device_to_file(dev.ptr + 3, n, str(out), 0x90CFC0AB, stream_off=1 << 40)
    got = np.frombuffer(out.read_bytes(), np.uint8)
    assert got.size == n and np.array_equal(got, want_of(pt[:n], 0x90CFC0AB, 1 << 40))
    assert np.array_equal(dev.a, keep)
    fresh = tmp_path / "fresh.bin"
    M.cycle_device_to_file(dev.ptr, 17, str(fresh), 1)
    assert (os.stat(fresh).st_mode & 0o777) == (0o644 & ~_umask())
    with pytest.raises(M.ModGpuError) as e:
        M.cycle_file_to_device(str(part), dev.ptr, n, 1, file_off=200)  # past the end of the file
    assert e.value.code != 0
    assert part.read_bytes() == pt.tobytes()
    dev.free()


def _umask():
    u = os.umask(0)
    os.umask(u)
    return u


def test_stream_offsets_near_2_64_and_identity_keys(lib):
    n = 2 * CHUNK + 77
    pt = O.splitmix_bytes(n, 9)
    dev, host = Dev(lib, n + 2 * GUARD + 16), np.empty(n + 2 * GUARD + 16, np.uint8)
    for so in ((1 << 64) - n - 77, (1 << 64) - 3, (1 << 32) - 17, O.PERIOD - 9):
        upload(lib, dev, host, pt, 3, 11, 0xC64EED30, so)
        download(lib, dev, host, pt, 14, 1, 0x90CFC0AB, so)
    for key in (0, 0x7FFFFFFF, 0x80000001):  # 0 mod 2^31-1: the bytes are copied unchanged
        upload(lib, dev, host, pt, 5, 6, key, 123)
        download(lib, dev, host, pt, 6, 5, key, 123)
        assert np.array_equal(want_of(pt, key, 123), pt)
    dev.free()


def test_validation_before_anything_is_queued(lib):
    dev = Dev(lib, 4096, device=0)
    other = Dev(lib, 4096, device=3)
    host = np.zeros(4096, np.uint8)
    before = launches(lib)

    def code(fn, *a, **kw):
        with pytest.raises(M.ModGpuError) as e:
            fn(*a, **kw)
        return e.value.code

    L = M.lib()
    assert L.modgpu_cycle_host_to_device(None, ctypes.c_void_p(host.ctypes.data), 10, 1, 0, 0) == 1
    assert L.modgpu_cycle_host_to_device(ctypes.c_void_p(dev.ptr), None, 10, 1, 0, 0) == 1
    assert L.modgpu_cycle_device_to_host(None, ctypes.c_void_p(dev.ptr), 10, 1, 0, 0) == 1
    assert L.modgpu_cycle_device_to_host(ctypes.c_void_p(host.ctypes.data), None, 10, 1, 0, 0) == 1
    assert L.modgpu_cycle_file_to_device(None, 0, ctypes.c_void_p(dev.ptr), 10, 1, 0, 0) == 1
    assert L.modgpu_cycle_device_to_file(None, 10, b"/nonexistent/x", 1, 0, 0) == 1
    assert code(M.cycle_host_to_device, host.ctypes.data, host[:100], 1, device=0) == 1        # a host pointer as the device side
    assert code(M.cycle_device_to_host, host[:100], host.ctypes.data + 200, 1, device=0) == 1
    assert code(M.cycle_host_to_device, other.ptr, host[:100], 1, device=0) == 1               # another device's memory
    assert code(M.cycle_host_to_device, dev.ptr + 4000, host[:100], 1, device=0) == 1          # runs past the allocation
    assert launches(lib) == before
    # n == 0 does nothing, NULL pointers included
    assert L.modgpu_cycle_host_to_device(None, None, 0, 1, 0, 0) == 0
    assert L.modgpu_cycle_device_to_host(None, None, 0, 1, 0, 0) == 0
    assert launches(lib) == before
    # the calling thread's current device is restored
    L.modgpu_shim_set_device(2)
    M.cycle_host_to_device(other.ptr, host[:100], 1, device=3)
    assert L.modgpu_shim_get_device() == 2
    L.modgpu_shim_set_device(0)
    dev.free()
    other.free()


@pytest.mark.parametrize("stage", [M.STAGE_FILL, M.STAGE_LAUNCH, M.STAGE_SYNC, M.STAGE_DRAIN, M.STAGE_AFTER_DRAIN])
def test_injected_failures(lib, stage):
    """A failure at the first, a middle and the last piece: an error, the source intact, no hang -- and the next call is right."""
    n = 6 * CHUNK + 5
    pt = O.splitmix_bytes(n, 10)
    dev, host = Dev(lib, n + 2 * GUARD + 16), np.empty(n + 2 * GUARD + 16, np.uint8)
    for piece in (0, M.INJECT_PIECE_MIDDLE, M.INJECT_PIECE_LAST):
        for direction in ("up", "down"):
            if direction == "up" and stage == M.STAGE_DRAIN:
                continue  # (an upload drains nothing: the kernel writes the device buffer itself)
            dev.a[:] = 0
            dev.a[GUARD:GUARD + n] = pt
            host[:] = 0
            host[GUARD:GUARD + n] = pt
            keep_d, keep_h = dev.a.copy(), host.copy()
            M.debug_inject_failure_at(piece, stage)
            t0 = time.monotonic()
            with pytest.raises(M.ModGpuError) as e:
                if direction == "up":
                    M.cycle_host_to_device(dev.ptr + GUARD, host[GUARD:GUARD + n], 0x90CFC0AB)
                else:
                    M.cycle_device_to_host(host[GUARD:GUARD + n], dev.ptr + GUARD, 0x90CFC0AB)
            assert e.value.code == 3 and "injected" in str(e.value), (piece, direction, str(e.value))
            assert time.monotonic() - t0 < 30
            assert not M.debug_injection_armed()
            if direction == "up":
                assert np.array_equal(host, keep_h)
            else:
                assert np.array_equal(dev.a, keep_d)
            upload(lib, dev, host, pt, 0, 0, 0x90CFC0AB)
            download(lib, dev, host, pt, 0, 0, 0x90CFC0AB)
    dev.free()


def test_wedged_kernel_returns_within_the_host_deadline(lib):
    """A transfer kernel that stops responding half-way: the call returns an error within the host deadline instead of hanging.
    Device 7 only: the device's host-buffer routes are abandoned afterwards, as for the host-fed kernel."""
    M.debug_set_host_tunable("feed_patience_ms", 200)
    n = 6 * CHUNK
    dev, host = Dev(lib, n, device=7), O.splitmix_bytes(n, 11)
    keep = host.copy()
    try:
        lib.modgpu_shim_wedge_next_xfer(1)
        t0 = time.monotonic()
        with pytest.raises(M.ModGpuError) as e:
            M.cycle_host_to_device(dev.ptr, host, 0x90CFC0AB, device=7)
        took = time.monotonic() - t0
        assert e.value.code == 3 and took < 4 * 0.2 + 2 + 5, (took, str(e.value))
        assert np.array_equal(host, keep)
        with pytest.raises(M.ModGpuError):  # the device's routes stay abandoned
            M.cycle_host_to_device(dev.ptr, host, 0x90CFC0AB, device=7)
    finally:
        lib.modgpu_shim_release_wedged_xfer()
        M.debug_set_host_tunable("feed_patience_ms", 10000)
    # (dev is not freed: the wedged launch was let go but the library keeps the lost call's slots and words out of circulation)


def test_upload_beside_cycle_host_on_one_device(lib):
    """An upload and a modgpu_cycle_host call on the same device at once, several times over: they share the staging set; both right."""
    n = 5 * CHUNK + 3
    pt = O.splitmix_bytes(n, 12)
    errors = []

    def up(t):
        try:
            dev, host = Dev(lib, n + 2 * GUARD + 16, device=1), np.empty(n + 2 * GUARD + 16, np.uint8)
            for k in range(4):
                upload(lib, dev, host, pt, (t + k) % 16, (3 * k) % 16, KEYS[k % 3], so=k << 33, device=1, alone=False)
                download(lib, dev, host, pt, k % 16, (t + 5 * k) % 16, KEYS[(k + 1) % 3], so=k, device=1, alone=False)
            dev.free()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def host_call(t):
        try:
            for k in range(4):
                b = O.splitmix_bytes(3 * n, 50 + t + k)
                want = want_of(b, 0xC64EED30, k)
                M.cycle_host(b, 0xC64EED30, k, device=1)
                assert np.array_equal(b, want)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=up, args=(t,)) for t in range(2)] + [threading.Thread(target=host_call, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


def test_dma_reference_form(lib):
    """The testing flavour's DMA form of both directions (a device slot and an out-of-place launch per chunk) gives the same bytes."""
    M.debug_set_xfer_form("dma")
    try:
        n = 3 * CHUNK + 9
        dev, host = Dev(lib, n + 2 * GUARD + 16), np.empty(n + 2 * GUARD + 16, np.uint8)
        pt = O.splitmix_bytes(n, 13)
        to0 = lib.modgpu_shim_to_launches(0) + lib.modgpu_shim_to_launches(1)
        for ph, pd in ((0, 0), (3, 9), (15, 1)):
            dev.a[:] = 0x5A
            host[:] = 0
            host[GUARD + ph:GUARD + ph + n] = pt
            M.cycle_host_to_device(dev.ptr + GUARD + pd, host[GUARD + ph:GUARD + ph + n], 0xC64EED30, 99)
            assert np.array_equal(dev.a[GUARD + pd:GUARD + pd + n], want_of(pt, 0xC64EED30, 99))
            assert (dev.a[:GUARD + pd] == 0x5A).all() and (dev.a[GUARD + pd + n:] == 0x5A).all()
            dev.a[GUARD + pd:GUARD + pd + n] = pt
            out = np.zeros(n, np.uint8)
            M.cycle_device_to_host(out, dev.ptr + GUARD + pd, 0xC64EED30, 99)
            assert np.array_equal(out, want_of(pt, 0xC64EED30, 99))
        assert lib.modgpu_shim_to_launches(0) + lib.modgpu_shim_to_launches(1) > to0
        dev.free()
    finally:
        M.debug_set_xfer_form(None)
