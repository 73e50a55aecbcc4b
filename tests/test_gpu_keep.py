"""GPU: the keep kernel (cycle_keep_kernel.hip -- the work-queue kernel with a cache policy per chunk) against the CPU oracle.

A cache policy must never change a byte, so these are parity tests under forced policies (modgpu_debug_set_keep) at the smallest shapes
that reach every code path of the kernel: the static chunks and the tickets, the cut first chunk, the ragged last one, head and tail
bytes, fewer chunks than workgroups -- each with no chunk resident, some, and all.  The expected bytes are the oracle's keystream, never
the library's.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte compared here came from a kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
CHUNK = 65536
GUARD = 64
KEEP = "modgpu_cycle_keep_kernel<4, 1024>"
MAIN = "modgpu_cycle_queue_kernel<4, 1024>"
POLICIES = [(1, 0), (1, 1), (3, 1), (3, 3), (0, 1)]  # (mask, run): none resident, alternating, one in four, three in four, all
OFFSETS = [0, (1 << 33) + 12345]
BIG = 437 * CHUNK + 77  # 200 main workgroups take their two static chunks, the other 37 + are tickets
SMALL = 3 * CHUNK + 1   # fewer chunks than workgroups
PHASE = 5               # bytes past a 64 KiB boundary: a cut first chunk and 11 head bytes


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


@pytest.fixture(scope="module")
def reference(oracle):
    """plaintext and, per stream offset, the oracle's ciphertext of BIG bytes under PS4: computed once, never written to"""
    pt = oracle.splitmix_bytes(BIG, 0x6B656570)
    ct = {off: oracle.cycle_at(pt.copy(), PS4, off) for off in OFFSETS}
    pt.setflags(write=False)
    for c in ct.values():
        c.setflags(write=False)
    return pt, ct


class Rig:
    """A device allocation in which the buffer under test starts PHASE bytes past a 64 KiB boundary, with GUARD bytes of 0xA5 either side."""

    def __init__(self, M, cap):
        self.M = M
        self.buf = M.DeviceBuffer(cap + 2 * CHUNK)
        self.at = (-self.buf.ptr) % CHUNK + CHUNK + PHASE  # offset of the data inside the allocation
        assert (self.buf.ptr + self.at) % CHUNK == PHASE and self.at >= GUARD

    def put(self, data):
        img = np.full(data.size + 2 * GUARD, 0xA5, np.uint8)
        img[GUARD:GUARD + data.size] = data
        self.buf.upload(img, offset=self.at - GUARD)

    def cycle(self, n, key, off):
        self.buf.cycle(key, n=n, offset=self.at, stream_off=off)
        self.buf.sync()
        return self.M.last_launch()

    def get(self, n):
        img = self.buf.download(n + 2 * GUARD, offset=self.at - GUARD)
        assert (img[:GUARD] == 0xA5).all() and (img[GUARD + n:] == 0xA5).all(), "the guard bytes around the buffer were written"
        return img[GUARD:GUARD + n]

    def free(self):
        self.buf.free()


def forced(M, mask, run):
    """every single-buffer launch through the work queue, and from one byte up through the keep kernel with this policy"""
    M.debug_set_launch("queue", 0)
    M.debug_set_keep(1, mask, run)


def restore(M):
    M.debug_set_keep(0, 0, 0)
    M.debug_set_launch(None, 0)


@pytest.mark.parametrize("mask,run", POLICIES)
def test_parity_under_every_policy(gpu, reference, mask, run):
    """437 chunks + 77 bytes starting 5 bytes past a 64 KiB boundary: the buffer and its guards against the oracle at both stream offsets;
    the launch is variant 2, 200 main workgroups, the keep kernel by name, the keep TU by hash."""
    pt, ct = reference
    with gpu.testing_flavour():
        rig = Rig(gpu, BIG)
        try:
            forced(gpu, mask, run)
            for off in OFFSETS:
                rig.put(pt)
                info = rig.cycle(BIG, PS4, off)
                assert info["kernel"] == KEEP and info["variant"] == 2 and info["source_hash"] == gpu.keep_kernel_source_hash(), info
                assert info["main_groups"] == 200 and info["bytes"] == BIG and info["chunk_bytes"] == CHUNK, info
                got = rig.get(BIG)
                bad = np.flatnonzero(got != ct[off])
                assert bad.size == 0, (mask, run, off, int(bad[0]), int(bad.size))
        finally:
            restore(gpu)
            rig.free()


@pytest.mark.parametrize("mask,run", POLICIES)
def test_parity_with_fewer_chunks_than_workgroups(gpu, reference, mask, run):
    pt, ct = reference
    with gpu.testing_flavour():
        rig = Rig(gpu, SMALL)
        try:
            forced(gpu, mask, run)
            for off in OFFSETS:
                rig.put(pt[:SMALL])
                info = rig.cycle(SMALL, PS4, off)
                assert info["kernel"] == KEEP and info["variant"] == 2, info
                assert np.array_equal(rig.get(SMALL), ct[off][:SMALL]), (mask, run, off)
        finally:
            restore(gpu)
            rig.free()


def test_involution_across_the_two_kernels(gpu, reference):
    """encrypt with one chunk in four resident, decrypt through the MAIN kernel (route off): the ciphertext is the oracle's and the
    plaintext returns"""
    pt, ct = reference
    off = OFFSETS[1]
    with gpu.testing_flavour():
        rig = Rig(gpu, BIG)
        try:
            rig.put(pt)
            forced(gpu, 3, 1)
            assert rig.cycle(BIG, PS4, off)["kernel"] == KEEP
            assert np.array_equal(rig.get(BIG), ct[off])
            gpu.debug_set_keep(gpu.KEEP_OFF, 1, 0)
            info = rig.cycle(BIG, PS4, off)
            assert info["kernel"] == MAIN and info["source_hash"] == gpu.kernel_source_hash(), info
            assert np.array_equal(rig.get(BIG), pt)
        finally:
            restore(gpu)
            rig.free()


def test_default_routing(gpu, oracle):
    """no hook: 320 MiB still runs on the main work-queue kernel; a call of the threshold's size (1 GiB) runs on the keep kernel with the
    policy modgpu_keep_policy states.  The 1 GiB pass is checked by involution and three 1 MiB windows of the oracle's keystream (the
    buffer holds zeros, so the ciphertext IS the keystream)."""
    n_small, n_big, win = 320 << 20, 1 << 30, 1 << 20
    assert gpu.keep_policy(n_small)[0] is False and gpu.keep_policy(n_big)[0] is True and gpu.keep_policy(n_big - 1)[0] is False
    buf = gpu.DeviceBuffer(n_big)
    try:
        zeros = np.zeros(64 << 20, np.uint8)
        for o in range(0, n_big, zeros.size):
            buf.upload(zeros, offset=o)
        buf.cycle(PS3, n=n_small, stream_off=7)
        buf.sync()
        info = gpu.last_launch()
        assert info["kernel"] == MAIN and info["variant"] == 2 and info["source_hash"] == gpu.kernel_source_hash(), info
        buf.cycle(PS3, n=n_small, stream_off=7)  # and back to zeros
        buf.cycle(PS3, n=n_big, stream_off=7)
        buf.sync()
        info = gpu.last_launch()
        assert info["kernel"] == KEEP and info["variant"] == 2 and info["source_hash"] == gpu.keep_kernel_source_hash(), info
        assert info["main_groups"] == 200 and info["grid"] == 256 and info["bytes"] == n_big, info
        for at in (0, (n_big // 2) - 12345, n_big - win):
            assert np.array_equal(buf.download(win, offset=at), oracle.keystream(PS3, win, 7 + at)), at
        buf.cycle(PS3, n=n_big, stream_off=7)
        buf.sync()
        for o in range(0, n_big, zeros.size):
            assert not buf.download(zeros.size, offset=o).any(), o
    finally:
        buf.free()
