"""GPU: the transfer entry points (modgpu_cycle_host_to_device, modgpu_cycle_device_to_host, modgpu_cycle_file_to_device,
modgpu_cycle_device_to_file) against the CPU oracle.

Every case checks the destination bytes, guard bytes on both sides of the destination, that the source is unchanged and that the
call was ONE launch of a transfer kernel.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte compared
here came from a kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = [0x90CFC0AB, 0xC64EED30, 1, 0xFFFFFFFF, 0x80000000, 12345, 0xDEADBEEF]
CHUNK = 128 << 10
GUARD = 64


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def one_launch(M, before):
    st = M.path_stats()
    assert st["gpu_launches"] - before == 1, st["gpu_launches"] - before
    ll = M.last_launch()
    assert ll["variant"] == 6 and "modgpu_cycle_xfer_kernel<" in ll["kernel"] and ll["source_hash"] == M.xfer_kernel_source_hash(), ll
    return ll


def enc(oracle, pt, key, so):
    w = pt.copy()
    return oracle.cycle_at(w, key, so)


def up_and_down(M, oracle, dev, host_src, host_dst, pt, ph, pd, key, so):
    """pt from host_src[GUARD + ph] up into dev[GUARD + pd], checked; then the device bytes down into host_dst[GUARD + ph], checked"""
    n = pt.size
    host_src[:] = 0xA5
    host_src[GUARD + ph:GUARD + ph + n] = pt
    keep = np.array(host_src, copy=True)
    dev.upload(np.full(dev.nbytes, 0x5A, np.uint8))
    before = M.path_stats()["gpu_launches"]
    M.cycle_host_to_device(dev.ptr + GUARD + pd, host_src[GUARD + ph:GUARD + ph + n], key, so)
    ll = one_launch(M, before)
    want = np.full(dev.nbytes, 0x5A, np.uint8)
    want[GUARD + pd:GUARD + pd + n] = enc(oracle, pt, key, so)
    assert np.array_equal(dev.download(), want), ("upload", n, ph, pd, hex(key), so)
    assert np.array_equal(np.asarray(host_src), keep), "the upload changed its source"
    # down: the ciphertext just made comes back as plaintext, the device bytes stay
    host_dst[:] = 0x33
    before = M.path_stats()["gpu_launches"]
    M.cycle_device_to_host(host_dst[GUARD + ph:GUARD + ph + n], dev.ptr + GUARD + pd, key, so)
    one_launch(M, before)
    w2 = np.full(host_dst.size, 0x33, np.uint8)
    w2[GUARD + ph:GUARD + ph + n] = pt
    assert np.array_equal(np.asarray(host_dst), w2), ("download", n, ph, pd, hex(key), so)
    assert np.array_equal(dev.download(), want), "the download changed its source"
    return ll


def test_pageable_parity_every_phase(gpu, oracle):
    M = gpu
    sizes = [1, 15, 16, 17, 4097, CHUNK - 1, CHUNK + 1, 5 * CHUNK + 7, (16 << 20) + 3]
    cap = max(sizes) + 2 * GUARD + 16
    dev = M.DeviceBuffer(cap)
    a, b = np.empty(cap, np.uint8), np.empty(cap, np.uint8)
    rng = np.random.default_rng(7)
    for n in sizes:
        pt = rng.integers(0, 256, size=n, dtype=np.uint8)
        phases = range(16) if n < (1 << 20) else (0, 5, 12)
        for pd in phases:
            up_and_down(M, oracle, dev, a, b, pt, (pd * 7 + n) % 16, pd, KEYS[(pd + n) % len(KEYS)], so=n * pd)
    dev.free()


def test_page_locked_parity_and_funnel(gpu, oracle):
    """The caller's page-locked pages read / written across PCIe where they lie; host and device phases that differ by a non-whole
    number of dwords take the funnel form."""
    M = gpu
    cap = (3 << 20) + 2 * GUARD + 16
    dev = M.DeviceBuffer(cap)
    pa, pb = M.PinnedBuffer(cap), M.PinnedBuffer(cap)
    assert pa.pinned and pb.pinned
    rng = np.random.default_rng(8)
    forms = set()
    for n in (1, 17, 4097, CHUNK + 1, (3 << 20) + 5):
        pt = rng.integers(0, 256, size=n, dtype=np.uint8)
        for ph, pd in ((0, 0), (3, 3), (1, 0), (0, 2), (7, 12), (15, 1)):
            ll = up_and_down(M, oracle, dev, pa.array, pb.array, pt, ph, pd, KEYS[(ph + pd) % len(KEYS)], so=(n << 20) + ph)
            forms.add(ll["kernel"])
    assert any("true>" in k for k in forms) and any("false>" in k for k in forms), forms
    pa.free()
    pb.free()
    dev.free()


def test_file_endpoints(gpu, oracle, tmp_path):
    M = gpu
    n = (9 << 20) + 333
    pt = oracle.splitmix_bytes(n + 100, 8)
    part = tmp_path / "part.bin"
    part.write_bytes(pt.tobytes())
    dev = M.DeviceBuffer(n + 2 * GUARD + 100)
    dev.upload(np.full(dev.nbytes, 0x5A, np.uint8))
    before = M.path_stats()["gpu_launches"]
    M.cycle_file_to_device(str(part), dev.ptr + GUARD + 3, n, 0xC64EED30, file_off=100, stream_off=100)
    one_launch(M, before)
    want = np.full(dev.nbytes, 0x5A, np.uint8)
    want[GUARD + 3:GUARD + 3 + n] = enc(oracle, pt[100:], 0xC64EED30, 100)
    assert np.array_equal(dev.download(), want)
    out = tmp_path / "out.bin"
    out.write_bytes(b"x" * (2 * n))
    before = M.path_stats()["gpu_launches"]
    M.cycle_device_to_file(dev.ptr + GUARD + 3, n, str(out), 0xC64EED30, stream_off=100)
    one_launch(M, before)
    assert out.read_bytes() == pt[100:].tobytes()
    assert np.array_equal(dev.download(), want)
    assert part.read_bytes() == pt.tobytes()
    dev.free()


def test_offsets_near_2_64_identity_keys_and_validation(gpu, oracle):
    M = gpu
    n = 3 * CHUNK + 77
    pt = oracle.splitmix_bytes(n, 9)
    dev = M.DeviceBuffer(n + 2 * GUARD + 16)
    a, b = np.empty(n + 2 * GUARD + 16, np.uint8), np.empty(n + 2 * GUARD + 16, np.uint8)
    for so in ((1 << 64) - n - 77, (1 << 64) - 3, (1 << 32) - 17):
        up_and_down(M, oracle, dev, a, b, pt, 3, 11, 0xC64EED30, so)
    for key in (0, 0x7FFFFFFF, 0x80000001):
        up_and_down(M, oracle, dev, a, b, pt, 5, 6, key, 123)
    before = M.path_stats()["gpu_launches"]
    for fn, args in ((M.cycle_host_to_device, (a.ctypes.data, b[:100], 1)), (M.cycle_device_to_host, (b[:100], a.ctypes.data, 1)),
                     (M.cycle_host_to_device, (dev.ptr + dev.nbytes - 50, b[:100], 1))):
        with pytest.raises(M.ModGpuError) as e:
            fn(*args)
        assert e.value.code == 1, str(e.value)
    assert M.path_stats()["gpu_launches"] == before
    dev.free()


def test_4gib_pageable_upload_equals_the_device_cipher(gpu, oracle):
    """4 GiB from pageable memory: undoing the upload with modgpu_cycle_device (same key and offset) gives the plaintext back, so the
    upload equals modgpu_cycle_device on the same bytes; the source is intact; one launch."""
    M = gpu
    n = 4 << 30
    block = oracle.splitmix_bytes(64 << 20, 4)
    pt = np.tile(block, n // block.size)
    pt[12345] ^= 0xFF  # (not periodic at the block size)
    dev = M.DeviceBuffer(n + 16)
    before = M.path_stats()["gpu_launches"]
    M.cycle_host_to_device(dev.ptr + 5, pt, 0x90CFC0AB, 777)
    one_launch(M, before)
    head = dev.download(1 << 20, offset=5)
    assert np.array_equal(head, enc(oracle, pt[:1 << 20], 0x90CFC0AB, 777))
    M.cycle_device(dev.ptr + 5, n, 0x90CFC0AB, 777)
    dev.sync()
    step = 256 << 20
    for o in range(0, n, step):
        assert np.array_equal(dev.download(step, offset=5 + o), pt[o:o + step]), o
    assert pt[12345] == block[12345] ^ 0xFF and np.array_equal(pt[:block.size // 2], np.r_[block[:12345], block[12345] ^ 0xFF, block[12346:block.size // 2]])
    dev.free()


def test_torch_tensor_as_destination_and_source(gpu):
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_torch_xfer_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_XFER_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
