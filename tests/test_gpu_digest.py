"""GPU: the digest entry points (modgpu_digest_device / modgpu_digest_batch_device / modgpu_digest_results) against zlib.

The expected value is always zlib.adler32 of bytes the CPU oracle made, or -- where every output byte is 0xFF -- the closed form in
Python integers; it is never taken from the library.  Every case keeps 4 KiB bands around the source, the destination and the record
and checks them unchanged.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every number compared here came from
a kernel."""
import ctypes
import zlib

import numpy as np
import pytest

from hip_rt import Graph, Stream, hip

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
KEYS = [PS4, PS3, 1, 0xFFFFFFFF, 0x80000000, 12345, (-127772) & 0xFFFFFFFF, 0xDEADBEEF]  # test_gpu_verify.py's, and its ZERO_KEYS and OFFSETS
ZERO_KEYS = [0, 0x7FFFFFFF, 0x80000001]
OFFSETS = [(1 << 32) - 17, (1 << 32) + 5, (1 << 63) - 9, (1 << 63) + 11, (1 << 64) - 3]
CHUNK = 65536
EDGE_SIZES = [0, 1, 15, 16, 17, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5]
# against a chunk-aligned address.  1, 5, 15: the aligned body starts 16 bytes into a chunk (a cut first chunk that is nearly whole);
# CHUNK - 17: it starts 16 bytes before the chunk's end (a cut first chunk of one word); CHUNK - 1: it starts on the next boundary
PHASES = [0, 1, 5, 15, CHUNK - 17, CHUNK - 1]
BAND = 4096
BIG = (48 << 20) + 3
P = 65521


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def cipher(oracle, data, key, off):
    w = data.copy()
    if w.size:
        oracle.cycle_at(w, key, off)
    return w


def adler(data):
    return zlib.adler32(data.tobytes()) & 0xFFFFFFFF


def record(r):
    """(s1 mod p, s2 mod p, n) of a record, and what the formula makes of them"""
    assert int(r["reserved"]) == 0
    s1, s2, n = int(r["s1"]) % P, int(r["s2"]) % P, int(r["n"])
    return n, ((n + n * s1 - s2) % P) << 16 | (1 + s1) % P


class Rig:
    """A source and a destination allocation, chunk-aligned inside, with room for any phase up to a chunk and a 4 KiB band on both
    sides, and a record with a 4 KiB band on both sides (0xEE: a record nobody zeroed shows)."""

    def __init__(self, M, cap):
        self.M = M
        self.size = cap + 2 * BAND + 2 * CHUNK
        self.sb, self.db = M.DeviceBuffer(self.size + CHUNK), M.DeviceBuffer(self.size + CHUNK)
        self.s0 = (-self.sb.ptr) % CHUNK  # offset of a chunk-aligned address; data goes to s0 + CHUNK + phase (>= BAND behind s0)
        self.d0 = (-self.db.ptr) % CHUNK
        self.rb = M.DeviceBuffer(2 * BAND + 32)
        self.res = self.rb.ptr + BAND

    def put(self, buf, base, data, phase, fill):
        img = np.full(self.size, fill, np.uint8)
        at = CHUNK + phase
        img[at:at + data.size] = data
        buf.upload(img, offset=base)
        return img

    def digest(self, n, ps, key, off, pd=None, alias=False):
        """one call; returns (n, adler32) of the record after checking the bands around it and the launch count"""
        M = self.M
        self.rb.upload(np.full(2 * BAND + 32, 0xEE, np.uint8))
        src = self.sb.ptr + self.s0 + CHUNK + ps
        dst = src if alias else None if pd is None else self.db.ptr + self.d0 + CHUNK + pd
        before = M.path_stats()["gpu_launches"]
        M.digest_device(src, key, off, dst=dst, result=self.res, n=n)
        self.rb.sync()
        assert M.path_stats()["gpu_launches"] - before == (1 if n else 0)
        got = self.rb.download()
        assert (got[:BAND] == 0xEE).all() and (got[BAND + 32:] == 0xEE).all(), "the bands around the record were written"
        recs, adlers = M.digest_results(self.res)
        assert np.array_equal(got[BAND:BAND + 32], recs[0:1].view(np.uint8))
        rec = got[BAND:BAND + 32].view(M.DIGEST_RESULT_DTYPE)[0]
        assert int(adlers[0]) == record(rec)[1] == M.digest_adler32(rec)
        return record(rec)

    def free(self):
        for b in (self.sb, self.db, self.rb):
            b.free()


def test_edge_sizes_phases_keys_offsets_digest_only(gpu, oracle):
    """Digest only at the sizes where heads, tails and chunk edges meet, every source phase, real and identity keys, offsets beyond 32
    and 63 bits in rotation: zlib's Adler-32 of the oracle's output each time; the source, its bands, the destination buffer and the
    record's bands are bit-identical afterwards; one launch per non-empty call, none for an empty one."""
    rig = Rig(gpu, max(EDGE_SIZES))
    rng = np.random.default_rng(16)
    d_img = rig.put(rig.db, rig.d0, np.zeros(0, np.uint8), 0, 0x5A)
    k = 0
    for n in EDGE_SIZES:
        data = rng.integers(0, 256, size=n, dtype=np.uint8)
        for ps in PHASES:
            s_img = rig.put(rig.sb, rig.s0, data, ps, 0xA5)
            for key in KEYS[:3] + ZERO_KEYS:
                off = OFFSETS[k % len(OFFSETS)]
                k += 1
                want = adler(cipher(oracle, data, key, off) if key not in ZERO_KEYS else data)
                assert rig.digest(n, ps, key, off) == (n, want), (n, ps, hex(key), off)
            assert np.array_equal(rig.sb.download(rig.size, offset=rig.s0), s_img), "the source or its bands changed"
    assert np.array_equal(rig.db.download(rig.size, offset=rig.d0), d_img), "a digest-only call wrote somewhere"
    rig.free()


def test_fused_stores_what_the_out_of_place_call_stores(gpu, oracle):
    """Fused: the destination (and its bands) is byte for byte the image modgpu_cycle_device_to leaves from the same start, which is the
    oracle's output; the digest is zlib's Adler-32 of it; (dst - src) mod 4 in {0, 1, 3} -- both forms of the reader -- and dst == src."""
    rig = Rig(gpu, max(EDGE_SIZES))
    ref = gpu.DeviceBuffer(rig.size + CHUNK)
    r0 = (rig.d0 + rig.db.ptr - ref.ptr) % CHUNK  # the same chunk phase as the rig's destination
    rng = np.random.default_rng(17)
    k = 0
    for n in EDGE_SIZES:
        data = rng.integers(0, 256, size=n, dtype=np.uint8)
        for ps, pd in ((0, 0), (5, 6), (2, 5), (15, CHUNK - 4), (CHUNK - 17, 18), (CHUNK - 1, 2)):
            assert (pd - ps) % 4 in (0, 1, 3)
            key, off = (KEYS + ZERO_KEYS)[k % 11], OFFSETS[k % 5]
            k += 1
            out = cipher(oracle, data, key, off) if key not in ZERO_KEYS else data
            s_img = rig.put(rig.sb, rig.s0, data, ps, 0xA5)
            d_img = rig.put(rig.db, rig.d0, np.zeros(0, np.uint8), 0, 0x5A)
            ref.upload(d_img, offset=r0)
            assert rig.digest(n, ps, key, off, pd=pd) == (n, adler(out)), (n, ps, pd, hex(key))
            if n > 32:
                assert gpu.last_launch()["kernel"].startswith("modgpu_cycle_to_kernel<4, 1024, " + ("true" if (pd - ps) % 4 else "false")), (ps, pd)
            gpu.cycle_device_to(ref.ptr + r0 + CHUNK + pd, rig.sb.ptr + rig.s0 + CHUNK + ps, n, key, off)
            ref.sync()
            got = rig.db.download(rig.size, offset=rig.d0)
            d_img[CHUNK + pd:CHUNK + pd + n] = out
            assert np.array_equal(got, d_img), "the destination is not the oracle's output inside untouched bands"
            assert np.array_equal(got, ref.download(rig.size, offset=r0)), "the destination differs from modgpu_cycle_device_to's"
            assert np.array_equal(rig.sb.download(rig.size, offset=rig.s0), s_img), "the source or its bands changed"
        # dst == src: in place, with a checksum
        key, off = KEYS[k % 8], OFFSETS[k % 5]
        s_img = rig.put(rig.sb, rig.s0, data, 7, 0xA5)
        out = cipher(oracle, data, key, off)
        assert rig.digest(n, 7, key, off, alias=True) == (n, adler(out)), (n, "alias")
        s_img[CHUNK + 7:CHUNK + 7 + n] = out
        assert np.array_equal(rig.sb.download(rig.size, offset=rig.s0), s_img)
    ref.free()
    rig.free()


def test_many_chunks_and_every_grid(gpu, oracle):
    """48 MiB + 3 at the shipped grid (more chunks than two rounds of it), and 40 chunks + 77 bytes on 1, 3 and 256 workgroups (testing
    flavour): a workgroup then owns many chunks of the entry, the sums are the same, and they are zlib's."""
    rig = Rig(gpu, BIG)
    data = oracle.splitmix_bytes(BIG, 48)
    want = adler(cipher(oracle, data, PS4, OFFSETS[1]))
    s_img = rig.put(rig.sb, rig.s0, data, 5, 0xA5)
    assert rig.digest(BIG, 5, PS4, OFFSETS[1]) == (BIG, want)
    info = gpu.last_launch()
    assert info["variant"] == 16 and info["bytes"] == BIG and 2 * info["grid"] < BIG // CHUNK, info
    assert np.array_equal(rig.sb.download(rig.size, offset=rig.s0), s_img)
    n = 40 * CHUNK + 77
    want = adler(cipher(oracle, data[:n], PS3, 9))
    with gpu.testing_flavour():
        try:
            for grid in (1, 3, 256, 0):
                gpu.debug_set_digest_grid(grid)
                for pd in (None, 2):
                    assert rig.digest(n, 5, PS3, 9, pd=pd) == (n, want), (grid, pd)
                    if grid:
                        assert gpu.last_launch()["grid"] == min(grid, 40), grid
        finally:
            gpu.debug_set_digest_grid(0)
    rig.free()


@pytest.mark.parametrize("n", [CHUNK, (512 << 20) + 77, (1 << 32) + 3 * CHUNK + 77])
def test_overflow_bounds_all_ones(gpu, n):
    """Every output byte 0xFF: the source is 0xFF ^ keystream, made on the device (a fill and one in-place cycle call), so the sums are
    the largest an entry of n bytes can have -- 32-bit lane sums at one chunk, unreduced 64-bit sums past 2^64 from about 380 MB,
    positions and chunk indices past 32 bits at 4 GiB + 3 chunks + 77.  Expected: A = 1 + 255 n, B = n + 255 n (n + 1) / 2, mod 65521."""
    off = (1 << 40) + 3
    buf = gpu.DeviceBuffer(n + 2 * BAND + 16)
    rb = gpu.DeviceBuffer(2 * BAND + 32)
    rb.upload(np.full(2 * BAND + 32, 0xEE, np.uint8))
    assert hip().hipMemset(ctypes.c_void_p(buf.ptr), 0xFF, ctypes.c_size_t(n + 2 * BAND + 16)) == 0
    at = BAND + 5
    gpu.cycle_device(buf.ptr + at, n, PS4, off)
    buf.sync()
    edges = [buf.download(2 * BAND, offset=0), buf.download(2 * BAND + 16 - 5, offset=n + 5)]
    before = gpu.path_stats()["gpu_launches"]
    gpu.digest_device(buf.ptr + at, PS4, off, result=rb.ptr + BAND, n=n)
    buf.sync()
    assert gpu.path_stats()["gpu_launches"] - before == 1
    info = gpu.last_launch()
    assert info["variant"] == 16 and info["bytes"] == n, info
    got = rb.download()
    assert (got[:BAND] == 0xEE).all() and (got[BAND + 32:] == 0xEE).all()
    want = ((n + 255 * n * (n + 1) // 2) % P) << 16 | (1 + 255 * n) % P
    assert record(got[BAND:BAND + 32].view(gpu.DIGEST_RESULT_DTYPE)[0]) == (n, want)
    assert np.array_equal(buf.download(2 * BAND, offset=0), edges[0]) and np.array_equal(buf.download(2 * BAND + 16 - 5, offset=n + 5), edges[1])
    assert (edges[0][:BAND] == 0xFF).all() and (edges[1][-BAND:] == 0xFF).all()
    buf.free()
    rb.free()


def test_batch_of_seventeen(gpu, oracle):
    """17 non-empty entries and two empty ones (two launches): 1-byte, unaligned, multi-chunk, some with a destination and some without,
    sources that overlap where nothing is written, an offset per entry.  Every record is its own entry's; destinations are the oracle's
    bytes; a second call onto the same records, not cleared in between, gives the same values."""
    rng = np.random.default_rng(5)
    sizes = [int(x) for x in rng.integers(2, 2 * CHUNK, size=19)]
    for i, s in ((0, 1), (3, 0), (5, 5 * CHUNK + 9), (8, 15), (12, 0), (18, 3 * CHUNK)):
        sizes[i] = s
    part_n = 6 * CHUNK
    plain = oracle.splitmix_bytes(part_n, 55)
    part = gpu.DeviceBuffer(part_n + 2 * BAND)
    p_img = np.full(part_n + 2 * BAND, 0xA5, np.uint8)
    p_img[BAND:BAND + part_n] = plain
    part.upload(p_img)
    src_offs = [int(rng.integers(0, part_n - s + 1)) for s in sizes]
    stream_offs = [o + (i << 33) for i, o in enumerate(src_offs)]
    with_dst = [i % 3 != 1 for i in range(19)]
    d_offs, at = [], BAND
    for i, s in enumerate(sizes):
        at += 1 + (5 * i) % 16
        d_offs.append(at)
        at += s if with_dst[i] else 0
    d_img = np.full(at + BAND, 0x5A, np.uint8)
    dst = gpu.DeviceBuffer(d_img.size)
    dst.upload(d_img)
    want = []
    for i, (s, o, q, so) in enumerate(zip(sizes, src_offs, d_offs, stream_offs)):
        out = cipher(oracle, plain[o:o + s], PS4, so)
        if with_dst[i]:
            d_img[q:q + s] = out
        want.append((s, adler(out)))
    res = gpu.DeviceBuffer(32 * 19 + 2 * BAND)
    res.upload(np.full(32 * 19 + 2 * BAND, 0xEE, np.uint8))
    for again in range(2):
        before = gpu.path_stats()["gpu_launches"]
        gpu.digest_batch_device([part.ptr + BAND + o for o in src_offs], sizes, PS4, res.ptr + BAND,
                                dst_ptrs=[dst.ptr + q if w else None for q, w in zip(d_offs, with_dst)], stream_offs=stream_offs)
        res.sync()
        assert gpu.path_stats()["gpu_launches"] - before == 2
        recs, adlers = gpu.digest_results(res.ptr + BAND, 19)
        assert [record(r) for r in recs] == want and [int(a) for a in adlers] == [w[1] for w in want], again
        got = res.download()
        assert (got[:BAND] == 0xEE).all() and (got[BAND + 32 * 19:] == 0xEE).all()
        assert np.array_equal(dst.download(), d_img) and np.array_equal(part.download(), p_img)
    for b in (part, dst, res):
        b.free()


def test_graph_replay_pinned_source_and_the_binding(gpu, oracle):
    """A captured call (memset node + launch) starts from a clean record on every replay: the source is rewritten between replays and
    each replay gives that source's value.  A page-locked source works.  digest_device and DeviceBuffer.digest with a record of the
    binding's own return the Adler-32 as an int."""
    n = (2 << 20) + 77
    src = [oracle.splitmix_bytes(n, 21), oracle.splitmix_bytes(n, 22)]
    want = [adler(cipher(oracle, s, PS3, 5)) for s in src]
    sb, res = gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(32)
    res.upload(np.full(32, 0xEE, np.uint8))
    st = Stream()
    sb.upload(src[0], offset=3)
    with Graph.capture(st) as g:
        gpu.digest_device(sb.ptr + 3, PS3, 5, result=res, n=n, stream=st.handle)
    for k in (0, 1, 1, 0):
        sb.upload(src[k], offset=3)
        g.launch(st)
        st.sync()
        recs, adlers = gpu.digest_results(res)
        assert record(recs[0]) == (n, want[k]) and int(adlers[0]) == want[k], ("graph replay", k)
    g.destroy()
    st.destroy()
    assert gpu.digest_device(sb.ptr + 3, PS3, 5, n=n) == want[0]
    assert sb.digest(PS3, n=n, offset=3, stream_off=5) == want[0]
    assert sb.digest(0, n=n, offset=3) == adler(src[0])
    assert sb.digest(PS3, n=0) == 1
    pb = gpu.PinnedBuffer(n + 8)
    pb.array[:] = 0
    pb.array[5:5 + n] = src[1]
    assert gpu.digest_device(pb.ptr + 5, PS3, 5, n=n) == want[1]
    pb.free()
    sb.free()
    res.free()


def test_reporting(gpu, oracle):
    """modgpu_last_launch: variant 16, the grid, `bytes` = n, the out-of-place TU's hash -- the digest loop is that TU's kernel."""
    n = 9 * CHUNK + 1
    sb, res = gpu.DeviceBuffer(n), gpu.DeviceBuffer(32)
    data = oracle.splitmix_bytes(n, 9)
    sb.upload(data)
    gpu.digest_device(sb, PS4, 0, result=res)
    sb.sync()
    info = gpu.last_launch()
    assert info["variant"] == 16 and info["bytes"] == n and info["grid"] == 9 and info["block"] == 1024 and info["chunk_bytes"] == CHUNK, info
    assert info["source_hash"] == gpu.to_kernel_source_hash() and info["kernel"] == "modgpu_cycle_to_kernel<4, 1024, false>", info
    assert int(gpu.digest_results(res)[1][0]) == adler(cipher(oracle, data, PS4, 0))
    sb.free()
    res.free()
