"""GPU: the out-of-place entry points (modgpu_cycle_device_to / modgpu_cycle_batch_device_to) against the CPU oracle.

Every case checks the destination bytes, guard bytes on both sides of the destination, and that the source is unchanged.
conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte compared here came from a kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hip_rt import Stream

pytestmark = pytest.mark.gpu

KEYS = [0x90CFC0AB, 0xC64EED30, 1, 0xFFFFFFFF, 0x80000000, 12345, (-127772) & 0xFFFFFFFF, 0xDEADBEEF]  # test_gpu_parity.py's
ZERO_KEYS = [0, 0x7FFFFFFF, 0x80000001]
CHUNK = 65536
GUARD = 64
EDGE_SIZES = [0, 1, 15, 16, 17, 255, 4097, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


class Pair:
    """A source and a destination allocation, each with room for any phase and GUARD bytes on both sides."""

    def __init__(self, M, cap):
        self.cap = cap
        self.src = M.DeviceBuffer(cap + 2 * GUARD + 16)
        self.dst = M.DeviceBuffer(cap + 2 * GUARD + 16)

    def run(self, M, oracle, pt, ps, pd, key, so=0, ks=None, check=True):
        n = pt.size
        s_off, d_off = GUARD + ps, GUARD + pd
        src_img = np.full(n + 2 * GUARD + 16, 0xA5, np.uint8)
        src_img[s_off:s_off + n] = pt
        dst_img = np.full(n + 2 * GUARD + 16, 0x5A, np.uint8)
        self.src.upload(src_img)
        self.dst.upload(dst_img)
        M.cycle_device_to(self.dst.ptr + d_off, self.src.ptr + s_off, n, key, so)
        self.dst.sync()
        if not check:
            return
        got = self.dst.download(n + 2 * GUARD, offset=d_off - GUARD)
        want = pt ^ (oracle.keystream(key, n, so) if ks is None else ks)
        assert np.array_equal(got[GUARD:GUARD + n], want), (n, ps, pd, hex(key), so)
        assert (got[:GUARD] == 0x5A).all() and (got[GUARD + n:] == 0x5A).all(), ("guard", n, ps, pd)
        assert np.array_equal(self.src.download(src_img.size), src_img), ("source changed", n, ps, pd)

    def free(self):
        self.src.free()
        self.dst.free()


def test_phase_grid_at_edge_sizes(gpu, oracle):
    """Every (src phase, dst phase) mod 16 at the sizes where heads, tails and chunk edges meet."""
    pair = Pair(gpu, max(EDGE_SIZES))
    rng = np.random.default_rng(7)
    for n in EDGE_SIZES:
        pt = rng.integers(0, 256, size=n, dtype=np.uint8)
        key = KEYS[n % len(KEYS)]
        ks = oracle.keystream(key, n, 0)
        for ps in range(16):
            for pd in range(16):
                pair.run(gpu, oracle, pt, ps, pd, key, ks=ks)
                if n and ps == 3 and pd == 7:
                    assert gpu.last_launch()["variant"] == 5
    pair.free()


def test_both_source_forms(gpu, oracle):
    """The unaligned-load form and the funnel form (testing flavour) agree with the oracle at the phases that separate them."""
    with gpu.testing_flavour():
        pair = Pair(gpu, 3 * CHUNK + 5)
        pt = np.random.default_rng(8).integers(0, 256, size=3 * CHUNK + 5, dtype=np.uint8)
        ks = oracle.keystream(0xC64EED30, pt.size, 99)
        try:
            for form in ("unaligned", "funnel"):
                gpu.debug_set_to_form(form)
                for ps, pd in ((1, 0), (5, 0), (2, 15), (7, 4), (4, 0), (0, 0)):
                    pair.run(gpu, oracle, pt, ps, pd, 0xC64EED30, so=99, ks=ks)
                    info = gpu.last_launch()
                    assert info["variant"] == 5
                    assert ("true" in info["kernel"]) == (form == "funnel" and (ps - pd) % 4 != 0), info
        finally:
            gpu.debug_set_to_form(None)
            pair.free()


def test_large_sizes_phase_subset(gpu, oracle):
    """256 MiB + 48 and 1 GiB + 13: whole-buffer parity for a few phases, plus the reported launch."""
    for n, phases in (((256 << 20) + 48, ((0, 0), (5, 0), (3, 11))), ((1 << 30) + 13, ((0, 0), (5, 0)))):
        pair = Pair(gpu, n)
        pt = oracle.splitmix_bytes(n, 11)
        key, so = 0x90CFC0AB, (1 << 32) - 12345
        ks = oracle.keystream(key, n, so)
        for ps, pd in phases:
            pair.run(gpu, oracle, pt, ps, pd, key, so=so, ks=ks)
            info = gpu.last_launch()
            assert info["variant"] == 5 and info["bytes"] == n and info["source_hash"] == gpu.to_kernel_source_hash(), info
        pair.free()


def test_keys_and_zero_keys(gpu, oracle):
    pair = Pair(gpu, 3 * CHUNK + 5)
    pt = oracle.splitmix_bytes(3 * CHUNK + 5, 3)
    for key in KEYS:
        pair.run(gpu, oracle, pt, 5, 0, key)
    for key in ZERO_KEYS:  # identity keystream: out of place that is a copy
        pair.run(gpu, oracle, pt, 5, 9, key)
        pair.run(gpu, oracle, pt[:17], 0, 3, key)
    pair.free()


def test_stream_offsets_to_2_to_64(gpu, oracle):
    """test_gpu_parity.py's offsets: byte j is at stream position stream_off + j in the integers."""
    P = oracle.PERIOD
    offs = [1, 15, 16, 4095, 4096, 4097, (1 << 24) + 5, P - 100, P - 1, P, P + 1, (1 << 32) - 17, (1 << 32) - 1, 1 << 32,
            (1 << 40) + 123, (1 << 63) + 99, (1 << 64) - 70000]
    pair = Pair(gpu, 66000)
    zeros = np.zeros(66000, np.uint8)
    for key in (0x90CFC0AB, 0xC64EED30, 12345):
        for off in offs:
            pair.run(gpu, oracle, zeros, 3, 0, key, so=off)
    pair.free()


def test_config2_size_matches_the_golden_digest(gpu, oracle, golden):
    """2^32 - 1 zero bytes out of place with the golden key: fnv1a64(dst) is the reference's own digest, from the out-of-place
    work-queue kernel (variant 5)."""
    L = golden["large"]
    n = L["n"]
    src, dst = gpu.DeviceBuffer(n), gpu.DeviceBuffer(n)
    zeros = np.zeros(1 << 28, np.uint8)
    for o in range(0, n, 1 << 28):
        src.upload(zeros[:min(1 << 28, n - o)], offset=o)
    gpu.cycle_device_to(dst.ptr, src.ptr, n, L["key"])
    dst.sync()
    info = gpu.last_launch()
    assert info["variant"] == 5 and info["bytes"] == n, info
    h = oracle.FNV_OFFSET
    for o in range(0, n, 1 << 28):
        h = oracle.fnv1a64(dst.download(min(1 << 28, n - o), offset=o), h)
    assert f"{h:016x}" == L["fnv_all"]
    for o in (0, n // 2, n - (1 << 20)):
        assert not src.download(1 << 20, offset=o).any()
    src.free()
    dst.free()


def test_alias_and_overlap(gpu, oracle):
    n = 3 * CHUNK + 5
    pt = oracle.splitmix_bytes(n + 64, 4)
    a, b = gpu.DeviceBuffer(n + 64), gpu.DeviceBuffer(n + 64)
    a.upload(pt)
    b.upload(pt)
    gpu.cycle_device_to(a.ptr + 3, a.ptr + 3, n, 0xC64EED30, 7)  # exact alias == the in-place call
    gpu.cycle_device(b.ptr + 3, n, 0xC64EED30, 7)
    a.sync()
    b.sync()
    assert np.array_equal(a.download(), b.download())
    want = pt.copy()
    oracle.cycle_at(want[3:3 + n], 0xC64EED30, 7)
    assert np.array_equal(a.download(), want)
    a.upload(pt)
    m = 1000
    for d_off, s_off in ((4, 3), (3, 4), (3 + m - 1, 3), (3, 3 + m - 1)):  # partial overlaps, down to one byte
        with pytest.raises(gpu.ModGpuError) as e:
            gpu.cycle_device_to(a.ptr + d_off, a.ptr + s_off, m, 0xC64EED30)
        assert e.value.code == 1
    a.sync()
    assert np.array_equal(a.download(), pt), "a refused call queued nothing"
    a.free()
    b.free()


@pytest.mark.parametrize("n_files", [16, 40])
def test_batch_gather_files_of_a_resident_part(gpu, oracle, n_files):
    """CArk::ExtractFiles on the device: file i at offset o_i of one encrypted part goes to its own buffer with stream_off = o_i.
    Sources overlap each other; destinations have every phase."""
    part_n = (24 << 20) + 7
    key = 0x90CFC0AB
    pt = oracle.splitmix_bytes(part_n, 21)
    part = gpu.DeviceBuffer(part_n + 16)
    enc = pt.copy()
    oracle.cycle_at(enc, key, 0)
    part.upload(enc, offset=5)
    rng = np.random.default_rng(n_files)
    sizes = [int(x) for x in rng.integers(0, 3 << 20, size=n_files)]
    sizes[0], sizes[1], sizes[2] = 0, 1, 17
    offs = [int(rng.integers(0, part_n - s + 1)) for s in sizes]
    offs[3] = offs[4] = 0  # two files from the same source bytes
    outs = gpu.DeviceBuffer(sum(sizes) + 32 * n_files)
    dsts, at = [], 0
    for i, s in enumerate(sizes):
        at += i % 16
        dsts.append(outs.ptr + at)
        at += s + 16 - (i % 16)
    srcs = [part.ptr + 5 + o for o in offs]
    gpu.cycle_batch_device_to(dsts, srcs, sizes, key, stream_offs=offs)
    outs.sync()
    for i, (s, o) in enumerate(zip(sizes, offs)):
        if s:
            assert np.array_equal(outs.download(s, offset=dsts[i] - outs.ptr), pt[o:o + s]), (i, s, o)
    assert np.array_equal(part.download(part_n, offset=5), enc), "the part must not change"
    if n_files <= 16:
        assert gpu.last_launch()["variant"] == 5
    part.free()
    outs.free()


def test_in_place_and_out_of_place_share_the_ring_on_four_streams(gpu, oracle):
    """In-place and out-of-place launches in flight together on 4 streams of one device: each gets its own ticket pair."""
    n = (260 << 20) + 3  # beyond 256 MiB: the in-place calls take the work-queue shape too
    pt = oracle.splitmix_bytes(n, 31)
    key = 0xC64EED30
    streams = [Stream() for _ in range(4)]
    bufs = [gpu.DeviceBuffer(n + 16) for _ in range(6)]
    for b in bufs:
        b.upload(pt)
    rounds = 3
    for _ in range(rounds):
        gpu.cycle_device(bufs[0].ptr, n, key, 0, stream=streams[0].handle)
        gpu.cycle_device_to(bufs[2].ptr + 1, bufs[1].ptr, n, key, 0, stream=streams[1].handle)
        gpu.cycle_device(bufs[3].ptr, n, key, 0, stream=streams[2].handle)
        gpu.cycle_device_to(bufs[5].ptr, bufs[4].ptr + 3, n - 3, key, 3, stream=streams[3].handle)
    for s in streams:
        s.sync()
        s.destroy()
    ct = oracle.cycle(pt.copy(), key)
    assert np.array_equal(bufs[0].download(n), ct)  # odd number of in-place rounds
    assert np.array_equal(bufs[3].download(n), ct)
    assert np.array_equal(bufs[2].download(n, offset=1), ct) and np.array_equal(bufs[1].download(n), pt)
    assert np.array_equal(bufs[5].download(n - 3), ct[3:]) and np.array_equal(bufs[4].download(n), pt)
    for b in bufs:
        b.free()


def test_page_locked_host_source(gpu, oracle):
    n = (16 << 20) + 13
    pb = gpu.PinnedBuffer(n + 8)
    pt = oracle.splitmix_bytes(n, 41)
    pb.array[3:3 + n] = pt
    d = gpu.DeviceBuffer(n + 16)
    gpu.cycle_device_to(d.ptr + 1, pb.ptr + 3, n, 0x90CFC0AB, 77)
    d.sync()
    want = pt.copy()
    oracle.cycle_at(want, 0x90CFC0AB, 77)
    assert np.array_equal(d.download(n, offset=1), want)
    assert np.array_equal(pb.array[3:3 + n], pt)
    d.free()
    pb.free()


def test_torch_views_streams_and_graph_capture(modgpu):
    assert modgpu.device_count() >= 1
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_torch_cycle_to_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_CYCLE_TO_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
