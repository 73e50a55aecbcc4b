"""GPU: the verify entry points (modgpu_verify_device / modgpu_verify_batch_device / modgpu_verify_results) against the CPU oracle.

The bytes a call is expected to find clean are computed by the oracle on the CPU and uploaded, never taken from the library; every case
states the exact (mismatches, first_mismatch, n) it expects.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every
number compared here came from a kernel."""
import math

import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
KEYS = [PS4, PS3, 1, 0xFFFFFFFF, 0x80000000, 12345, (-127772) & 0xFFFFFFFF, 0xDEADBEEF]  # test_gpu_rekey.py's, and its ZERO_KEYS and EDGE_SIZES
ZERO_KEYS = [0, 0x7FFFFFFF, 0x80000001]
CHUNK = 65536
EDGE_SIZES = [0, 1, 15, 16, 17, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5]
NONE = 0xFFFFFFFFFFFFFFFF
BAND = 4096
BIG = (48 << 20) + 3
OFFSETS = [(1 << 32) - 17, (1 << 32) + 5, (1 << 63) - 9, (1 << 63) + 11, (1 << 64) - 3]  # test_gpu_rekey.py's


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def cipher(oracle, data, key, off):
    w = data.copy()
    oracle.cycle_at(w, key, off)
    return w


def triple(r):
    assert int(r["reserved"]) == 0
    return int(r["mismatches"]), int(r["first_mismatch"]), int(r["n"])


class Rig:
    """An `expect` and a `src` allocation with room for any phase and a 4 KiB band on both sides, and a result with a 4 KiB band on both
    sides (0xEE: a result nobody initialised shows).  check() runs one call and returns its triple; with strict it also proves that
    nothing but the result was written."""

    def __init__(self, M, cap):
        self.M = M
        self.eb = M.DeviceBuffer(cap + 2 * BAND + 16)
        self.sb = M.DeviceBuffer(cap + 2 * BAND + 16)
        self.rb = M.DeviceBuffer(2 * BAND + 32)
        self.res = self.rb.ptr + BAND

    def put(self, buf, data, phase, fill):
        img = np.full(data.size + 2 * BAND + 16, fill, np.uint8)
        img[BAND + phase:BAND + phase + data.size] = data
        buf.upload(img)
        return img

    def call(self, n, pe, ps, key, off, launches=None):
        M = self.M
        self.rb.upload(np.full(2 * BAND + 32, 0xEE, np.uint8))
        before = M.path_stats()["gpu_launches"]
        M.verify_device(self.eb.ptr + BAND + pe, self.sb.ptr + BAND + ps, key, off, result=self.res, n=n)
        self.rb.sync()
        assert M.path_stats()["gpu_launches"] - before == (launches if launches is not None else 2 if n else 1)
        got = self.rb.download()
        assert (got[:BAND] == 0xEE).all() and (got[BAND + 32:] == 0xEE).all(), "the bands around the result were written"
        assert np.array_equal(got[BAND:BAND + 32], M.verify_results(self.res)[0:1].view(np.uint8))
        return triple(got[BAND:BAND + 32].view(M.VERIFY_RESULT_DTYPE)[0])

    def check(self, expect, src, pe, ps, key, off, strict=True):
        e_img = self.put(self.eb, expect, pe, 0x5A)
        s_img = self.put(self.sb, src, ps, 0xA5)
        got = self.call(src.size, pe, ps, key, off)
        if strict:
            assert np.array_equal(self.eb.download(e_img.size), e_img), "expect or its bands changed"
            assert np.array_equal(self.sb.download(s_img.size), s_img), "src or its bands changed"
        return got

    def free(self):
        for b in (self.eb, self.sb, self.rb):
            b.free()


def test_clean_at_edge_sizes_and_phases(gpu, oracle):
    """expect = the oracle's output: (0, NONE, n) at the sizes where heads, tails and chunk edges meet and at 48 MiB + 3, every src
    phase against expect phase 0 and every expect phase against src phase 5 (both forms of the reader); nothing but the result is
    written (4 KiB bands around expect, src and the result, and the buffers themselves, bit-identical afterwards)."""
    rig = Rig(gpu, BIG)
    rng = np.random.default_rng(7)
    for n in EDGE_SIZES + [BIG]:
        src = rng.integers(0, 256, size=n, dtype=np.uint8)
        off = 3 + n % 16
        want = cipher(oracle, src, PS3, off)
        for pe, ps in [(0, p) for p in range(16)] + [(p, 5) for p in range(16)]:
            strict = n < BIG or (pe, ps) in ((0, 0), (0, 7), (9, 5))
            assert rig.check(want, src, pe, ps, PS3, off, strict=strict) == (0, NONE, n), (n, pe, ps)
            if n > 32:
                info = gpu.last_launch()
                assert info["variant"] == 10 and info["source_hash"] == gpu.verify_kernel_source_hash() and info["bytes"] == n, info
                assert info["kernel"].startswith("modgpu_cycle_verify_kernel<4, 1024, " + ("true" if (ps - pe) % 4 else "false") + ", true>"), info
    rig.free()


def test_clean_under_keys_and_offsets(gpu, oracle):
    n = 3 * CHUNK + 5
    rig = Rig(gpu, n)
    src = oracle.splitmix_bytes(n, 3)
    for i, key in enumerate(KEYS):
        assert rig.check(cipher(oracle, src, key, 7 * i + 1), src, 0, 5, key, 7 * i + 1) == (0, NONE, n), hex(key)
    for key in ZERO_KEYS:  # the identity keystream: a plain compare
        assert rig.check(src, src, 3, 6, key, 11) == (0, NONE, n), hex(key)
        assert "false>" in gpu.last_launch()["kernel"]
        other = src.copy()
        other[[5, n - 2]] ^= 0xFF
        assert rig.check(other, src, 3, 7, key, 11) == (2, 5, n), hex(key)
    for off in OFFSETS:
        assert rig.check(cipher(oracle, src, PS4, off), src, 9, 0, PS4, off) == (0, NONE, n), off
        assert rig.check(cipher(oracle, src, PS3, off), src, 0, 4, PS3, off) == (0, NONE, n), off
    rig.free()


def test_planted_mismatches(gpu, oracle):
    """Bytes of `expect` flipped on the device: the exact count and the exact lowest index each time; a flipped byte just outside
    [expect, expect + n) or [src, src + n) changes nothing."""
    n = 5 * CHUNK + 21
    rig = Rig(gpu, n)
    src = oracle.splitmix_bytes(n, 8)
    off = (1 << 40) + 9
    want = cipher(oracle, src, PS4, off)
    rng = np.random.default_rng(1000)
    thousand = sorted(int(x) for x in rng.choice(n, size=1000, replace=False))
    for pe, ps in ((0, 0), (5, 3), (11, 11), (15, 2)):
        e0 = BAND + pe
        head = (16 - (rig.eb.ptr + e0) % 16) % 16                              # bytes in front of the aligned body
        cut = CHUNK - (rig.eb.ptr + e0 + head) % CHUNK                         # bytes of the body in its cut first chunk
        boundary = head + cut + CHUNK                                          # the first byte of a later whole chunk
        tail_at = n - 1 - ((rig.eb.ptr + e0 + n) % 16) // 2                    # inside the ragged tail (or the last byte)
        plants = [[0], [n - 1], [max(head - 1, 0)], [tail_at], [head + cut // 2], [head + cut - 1], [head + cut], [boundary - 1, boundary],
                  [boundary + 33, boundary + 35], [boundary + 16 * 1024 - 1, boundary + 16 * 1024], thousand]
        rig.put(rig.eb, want, pe, 0x5A)
        rig.put(rig.sb, src, ps, 0xA5)
        assert rig.call(n, pe, ps, PS4, off) == (0, NONE, n)
        for js in plants:
            js = sorted(set(js))
            bad = want.copy()
            bad[js] ^= 0x01
            for lo in range(min(js) // 4096 * 4096, max(js) + 1, 1 << 20):  # flip on the device: rewrite only the pages that changed
                hi = min(n, lo + (1 << 20))
                rig.eb.upload(bad[lo:hi], offset=e0 + lo)
            assert rig.call(n, pe, ps, PS4, off) == (len(js), js[0], n), (pe, ps, js[:4])
            rig.eb.upload(want, offset=e0)
        # just outside both ranges: one byte in front and one behind, on either side
        for buf, base in ((rig.eb, e0), (rig.sb, BAND + ps)):
            for at in (base - 1, base + n):
                keep = buf.download(1, offset=at)
                buf.upload(keep ^ 0xFF, offset=at)
                assert rig.call(n, pe, ps, PS4, off) == (0, NONE, n), (pe, ps, at - base)
                buf.upload(keep, offset=at)
    rig.free()


def test_everything_wrong(gpu, oracle):
    """Right data, wrong key, 64 MiB: the count and the lowest index numpy gives for the oracle's two keystreams XORed."""
    n = 64 << 20
    rig = Rig(gpu, n)
    src = oracle.splitmix_bytes(n, 17)
    want = cipher(oracle, src, PS3, 5)
    wrong = cipher(oracle, src, PS4, 5)
    diff = np.flatnonzero(want != wrong)
    assert diff.size > n * 0.99
    assert rig.check(want, src, 0, 0, PS4, 5, strict=False) == (diff.size, int(diff[0]), n)
    assert rig.check(want, src, 6, 1, PS4, 5, strict=True) == (diff.size, int(diff[0]), n)
    rig.free()


def test_aliases(gpu, oracle):
    """expect == src: clean under the identity key, the count of nonzero keystream bytes under a real one; a partial overlap is legal."""
    n = 3 * CHUNK + 5
    a = gpu.DeviceBuffer(n + 64)
    res = gpu.DeviceBuffer(32)
    data = oracle.splitmix_bytes(n + 64, 12)
    a.upload(data)
    for key in ZERO_KEYS:
        gpu.verify_device(a.ptr + 3, a.ptr + 3, key, 9, result=res, n=n)
        a.sync()
        assert triple(gpu.verify_results(res)[0]) == (0, NONE, n)
    ks = cipher(oracle, np.zeros(n, np.uint8), PS4, 9)
    nz = np.flatnonzero(ks)
    gpu.verify_device(a.ptr + 3, a.ptr + 3, PS4, 9, result=res, n=n)
    a.sync()
    assert triple(gpu.verify_results(res)[0]) == (nz.size, int(nz[0]), n)
    diff = np.flatnonzero(data[3:3 + n] != cipher(oracle, data[10:10 + n], PS3, 0))
    assert triple(gpu.verify_device(a.ptr + 3, a.ptr + 10, PS3, n=n)) == (diff.size, int(diff[0]), n)  # (a result buffer of the binding's own)
    assert np.array_equal(a.download(), data)
    a.free()
    res.free()


def test_batch_of_forty(gpu, oracle):
    """40 entries (three compare launches), sizes 0 .. 8 MiB, mixed phases, own offsets, overlapping sources; three entries corrupted;
    every result exact, and the launches as the header states: 1 + ceil(non_empty / 16)."""
    rng = np.random.default_rng(40)
    sizes = [int(x) for x in rng.integers(0, 3 * CHUNK, size=40)]
    for i, s in ((2, 8 << 20), (7, 0), (11, (8 << 20) - 3), (19, 1), (30, 0), (39, 15)):
        sizes[i] = s
    part_n = (8 << 20) + 999
    plain = oracle.splitmix_bytes(part_n, 5)
    src_offs = [int(rng.integers(0, part_n - s + 1)) for s in sizes]  # the sources overlap each other
    part = gpu.DeviceBuffer(part_n + 16)
    part.upload(plain, offset=3)
    e_offs, at = [], 0
    for i, s in enumerate(sizes):
        at += (7 * i) % 16
        e_offs.append(at)
        at += s
    stream_offs = [o + (i << 33) for i, o in enumerate(src_offs)]
    image = np.zeros(at + 16, np.uint8)
    for s, o, q, so in zip(sizes, src_offs, e_offs, stream_offs):
        image[q:q + s] = cipher(oracle, plain[o:o + s], PS4, so)
    want = [(0, NONE, s) for s in sizes]
    for i, js in ((2, [CHUNK, 5 << 20]), (19, [0]), (33, [sizes[33] - 1])):
        for j in js:
            image[e_offs[i] + j] ^= 0x10
        want[i] = (len(js), js[0], sizes[i])
    exp = gpu.DeviceBuffer(image.size)
    exp.upload(image)
    res = gpu.DeviceBuffer(32 * 41)
    res.upload(np.full(32 * 41, 0xEE, np.uint8))
    before = gpu.path_stats()["gpu_launches"]
    gpu.verify_batch_device([exp.ptr + q for q in e_offs], [part.ptr + 3 + o for o in src_offs], sizes, PS4, res, stream_offs=stream_offs)
    res.sync()
    non_empty = sum(1 for s in sizes if s)
    assert gpu.path_stats()["gpu_launches"] - before == 1 + math.ceil(non_empty / 16) == 4
    assert [triple(r) for r in gpu.verify_results(res, 40)] == want
    assert (res.download(32, offset=32 * 40) == 0xEE).all()
    assert np.array_equal(exp.download(), image) and np.array_equal(part.download(part_n, offset=3), plain)
    for b in (part, exp, res):
        b.free()


def test_graph_replay_and_streams(gpu, oracle):
    """A captured call starts from a clean result on every replay: clean -> clean, one byte corrupted between replays -> that byte,
    restored -> clean again.  Eight streams at once with results of their own.  A page-locked source works."""
    n = (2 << 20) + 77
    src = oracle.splitmix_bytes(n, 21)
    want = cipher(oracle, src, PS3, 5)
    eb, sb, res = gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(32)
    eb.upload(want, offset=1)
    sb.upload(src, offset=3)
    res.upload(np.full(32, 0xEE, np.uint8))
    st = Stream()
    with Graph.capture(st) as g:
        gpu.verify_device(eb.ptr + 1, sb.ptr + 3, PS3, 5, result=res, n=n, stream=st.handle)
    at = CHUNK + 12345
    for k, (flip, expect) in enumerate(((0, (0, NONE, n)), (0, (0, NONE, n)), (0x20, (1, at, n)), (0x20, (1, at, n)), (0, (0, NONE, n)))):
        eb.upload(want[at:at + 1] ^ flip, offset=1 + at)
        g.launch(st)
        st.sync()
        assert triple(gpu.verify_results(res)[0]) == expect, ("graph replay", k)
    g.destroy()
    st.destroy()

    streams = [Stream() for _ in range(8)]
    results = gpu.DeviceBuffer(32 * 8)
    results.upload(np.full(32 * 8, 0xEE, np.uint8))
    bufs = []
    for i in range(8):
        e = gpu.DeviceBuffer(n + 16)
        img = cipher(oracle, src, PS4, i << 32)
        if i % 2:
            img[[1000 * i, n - i]] ^= 0x80
        e.upload(img, offset=2 * i)
        bufs.append(e)
    for i, s in enumerate(streams):
        gpu.verify_device(bufs[i].ptr + 2 * i, sb.ptr + 3, PS4, i << 32, result=results.ptr + 32 * i, n=n, stream=s.handle)
    for s in streams:
        s.sync()
    got = [triple(r) for r in gpu.verify_results(results, 8)]
    assert got == [(2, 1000 * i, n) if i % 2 else (0, NONE, n) for i in range(8)]
    for s in streams:
        s.destroy()
    for b in bufs + [results]:
        b.free()

    pb = gpu.PinnedBuffer(n + 8)
    pb.array[:] = 0
    pb.array[5:5 + n] = src
    gpu.verify_device(eb.ptr + 1, pb.ptr + 5, PS3, 5, result=res, n=n)
    eb.sync()
    assert triple(gpu.verify_results(res)[0]) == (0, NONE, n)
    pb.free()
    for b in (eb, sb, res):
        b.free()


def test_small_grids_give_the_same_numbers(gpu, oracle):
    """The static chunk assignment on 1, 3 and 200 workgroups (testing flavour): a workgroup then walks through several entries of a
    batch and leaves each of them with a flush of its own."""
    sizes = [5 * CHUNK + 1, 0, 17, 9 * CHUNK, 3]
    plain = oracle.splitmix_bytes(sum(sizes) + 64, 77)
    with gpu.testing_flavour():
        eb, sb, res = gpu.DeviceBuffer(plain.size + 64), gpu.DeviceBuffer(plain.size), gpu.DeviceBuffer(32 * len(sizes))
        sb.upload(plain)
        offs, at = [], 0
        for s in sizes:
            offs.append(at)
            at += s + 3
        image = np.zeros(plain.size + 64, np.uint8)
        want = []
        for i, (s, o) in enumerate(zip(sizes, offs)):
            image[o + 1:o + 1 + s] = cipher(oracle, plain[o:o + s], PS3, i)
            js = sorted({s // 3, s - 1}) if s else []
            image[[o + 1 + j for j in js]] ^= 0x04
            want.append((len(js), js[0], s) if s else (0, NONE, 0))
        eb.upload(image)
        try:
            for grid in (1, 3, 200, 0):
                gpu.debug_set_verify_form(grid)
                res.upload(np.full(32 * len(sizes), 0xEE, np.uint8))
                gpu.verify_batch_device([eb.ptr + o + 1 for o in offs], [sb.ptr + o for o in offs], sizes, PS3, res, stream_offs=list(range(len(sizes))))
                res.sync()
                assert [triple(r) for r in gpu.verify_results(res, len(sizes))] == want, grid
                if grid:
                    assert gpu.last_launch()["grid"] <= grid, grid
        finally:
            gpu.debug_set_verify_form(0)
        for b in (eb, sb, res):
            b.free()


def test_4gib_part_whole(gpu):
    """The benchmark's launch checked whole: a 4 GiB part after one modgpu_cycle_device pass, verified against the plaintext kept in a
    second buffer -> clean; then one byte flipped at a seeded position in each of the 16 256-MiB slices -> 16, the lowest of them."""
    n = 4 << 30
    part, plain, res = gpu.DeviceBuffer(n), gpu.DeviceBuffer(n), gpu.DeviceBuffer(32)
    tile = np.random.default_rng(4).integers(0, 256, size=(16 << 20) + 13, dtype=np.uint8)
    for off in range(0, n, tile.size):
        piece = tile[:min(tile.size, n - off)]
        part.upload(piece, offset=off)
        plain.upload(piece, offset=off)
    gpu.cycle_device(part.ptr, n, PS4, 0)
    part.sync()
    gpu.verify_device(part, plain, PS4, 0, result=res)
    part.sync()
    info = gpu.last_launch()
    assert info["variant"] == 10 and info["bytes"] == n, info
    assert triple(gpu.verify_results(res)[0]) == (0, NONE, n)
    rng = np.random.default_rng(16)
    spots = [(k << 28) + int(rng.integers(0, 1 << 28)) for k in range(16)]
    for at in spots:
        part.upload(part.download(1, offset=at) ^ 0x01, offset=at)
    gpu.verify_device(part, plain, PS4, 0, result=res)
    part.sync()
    assert triple(gpu.verify_results(res)[0]) == (16, min(spots), n)
    for b in (part, plain, res):
        b.free()
