"""GPU: the rekey verify entry points (modgpu_verify_rekey_device / modgpu_verify_rekey_batch_device) against the CPU oracle.

The bytes a call is expected to find clean are the oracle's: cycle_at under key_from at off_from, then under key_to at off_to, computed on
the CPU and uploaded, never taken from the library; every case states the exact (mismatches, first_mismatch, n) it expects.  conftest.py
sets MODGPU_REQUIRE_GPU=1 before the library loads, so every number compared here came from a kernel."""
import math

import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
KEYS = [PS4, PS3, 1, 0xFFFFFFFF, 0x80000000, 12345, (-127772) & 0xFFFFFFFF, 0xDEADBEEF]  # test_gpu_rekey.py's, and its ZERO_KEYS
ZERO_KEYS = [0, 0x7FFFFFFF, 0x80000001]
OFFSETS = [(1 << 32) - 17, (1 << 32) + 5, (1 << 63) - 9, (1 << 63) + 11, (1 << 64) - 3]  # test_gpu_rekey.py's
PERIOD = (1 << 31) - 2
CHUNK = 65536
EDGE_SIZES = [0, 1, 15, 16, 17, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5]
NONE = 0xFFFFFFFFFFFFFFFF
BAND = 4096
BIG = (17 << 20) + 3  # 273 chunks: more than one per workgroup at the shipped grid
TWO = "modgpu_cycle_rekey_verify_kernel<4, 1024, "
ONE = "modgpu_cycle_verify_kernel<4, 1024, "


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def rekeyed(oracle, data, key_from, off_from, key_to, off_to):
    """what a rekey makes of `data`, by the oracle: two passes of the cipher on the CPU"""
    w = data.copy()
    oracle.cycle_at(w, key_from, off_from)
    oracle.cycle_at(w, key_to, off_to)
    return w


def triple(r):
    assert int(r["reserved"]) == 0
    return int(r["mismatches"]), int(r["first_mismatch"]), int(r["n"])


def numpy_says(a, b):
    d = np.flatnonzero(a != b)
    return (int(d.size), int(d[0]) if d.size else NONE, int(a.size))


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

    def call(self, n, pe, ps, keys, offs, launches=None):
        M = self.M
        self.rb.upload(np.full(2 * BAND + 32, 0xEE, np.uint8))
        before = M.path_stats()["gpu_launches"]
        M.verify_rekey_device(self.eb.ptr + BAND + pe, self.sb.ptr + BAND + ps, keys[0], keys[1], offs[0], offs[1], result=self.res, n=n)
        self.rb.sync()
        assert M.path_stats()["gpu_launches"] - before == (launches if launches is not None else 2 if n else 1)
        got = self.rb.download()
        assert (got[:BAND] == 0xEE).all() and (got[BAND + 32:] == 0xEE).all(), "the bands around the result were written"
        assert np.array_equal(got[BAND:BAND + 32], M.verify_results(self.res)[0:1].view(np.uint8))
        return triple(got[BAND:BAND + 32].view(M.VERIFY_RESULT_DTYPE)[0])

    def check(self, expect, src, pe, ps, keys, offs, strict=True):
        e_img = self.put(self.eb, expect, pe, 0x5A)
        s_img = self.put(self.sb, src, ps, 0xA5)
        got = self.call(src.size, pe, ps, keys, offs)
        if strict:
            assert np.array_equal(self.eb.download(e_img.size), e_img), "expect or its bands changed"
            assert np.array_equal(self.sb.download(s_img.size), s_img), "src or its bands changed"
        return got

    def free(self):
        for b in (self.eb, self.sb, self.rb):
            b.free()


def test_clean_at_edge_sizes_and_phases(gpu, oracle):
    """expect = the oracle's rekey PS3 -> PS4: (0, NONE, n) at the sizes where heads, tails and chunk edges meet, every src phase against
    expect phase 0 and every expect phase against src phase 5 (both forms of the reader), and at 17 MiB + 3 (273 chunks: more than one
    per workgroup) at three phase pairs; nothing but the result is written (4 KiB bands around expect, src and the result, and the
    buffers themselves, bit-identical afterwards)."""
    rig = Rig(gpu, BIG)
    rng = np.random.default_rng(7)
    for n in EDGE_SIZES + [BIG]:
        src = rng.integers(0, 256, size=n, dtype=np.uint8)
        offs = (3 + n % 16, 11 + n % 7)
        want = rekeyed(oracle, src, PS3, offs[0], PS4, offs[1])
        pairs = [(0, p) for p in range(16)] + [(p, 5) for p in range(16)] if n < BIG else [(0, 0), (0, 7), (9, 5)]
        for pe, ps in pairs:
            assert rig.check(want, src, pe, ps, (PS3, PS4), offs) == (0, NONE, n), (n, pe, ps)
            if n > 32:
                info = gpu.last_launch()
                assert info["variant"] == 12 and info["source_hash"] == gpu.rekey_verify_kernel_source_hash() and info["bytes"] == n, info
                assert info["kernel"] == TWO + ("true" if (ps - pe) % 4 else "false") + ">", info
    rig.free()


def test_keys_and_offsets(gpu, oracle):
    """Pairs of keys, offsets around 2^32, 2^63 and 2^64 on either side; the degenerate keystreams run on the verify kernels (variant 10):
    a zero key on one side leaves the other keystream (keyed form), on both a plain compare (identity form); the same key at offsets
    equal mod 2^31-2 is a plain compare."""
    n = 3 * CHUNK + 5
    rig = Rig(gpu, n)
    src = oracle.splitmix_bytes(n, 3)
    for i, (kf, kt) in enumerate(zip(KEYS, KEYS[1:] + KEYS[:1])):
        offs = (7 * i + 1, 5 * i + 2)
        assert rig.check(rekeyed(oracle, src, kf, offs[0], kt, offs[1]), src, 0, 5, (kf, kt), offs) == (0, NONE, n), (hex(kf), hex(kt))
        assert gpu.last_launch()["variant"] == 12
    for off in OFFSETS:
        assert rig.check(rekeyed(oracle, src, PS3, off, PS4, 9), src, 9, 0, (PS3, PS4), (off, 9)) == (0, NONE, n), off
        assert rig.check(rekeyed(oracle, src, PS3, 9, PS4, off), src, 0, 4, (PS3, PS4), (9, off)) == (0, NONE, n), off
        assert rig.check(rekeyed(oracle, src, PS4, off, PS4, off + 1), src, 2, 3, (PS4, PS4), (off, (off + 1) % (1 << 64))) == (0, NONE, n), off
        assert gpu.last_launch()["variant"] == 12
    other = src.copy()
    other[[5, n - 2]] ^= 0xFF
    for z in ZERO_KEYS:
        for keys, offs, form in (((z, PS4), (11, 13), "true>"), ((PS3, z), (11, 13), "true>"), ((z, ZERO_KEYS[0]), (11, 13), "false>")):
            want = rekeyed(oracle, src, keys[0], offs[0], keys[1], offs[1])
            assert rig.check(want, src, 3, 6, keys, offs) == (0, NONE, n), (hex(z), form)
            info = gpu.last_launch()
            assert info["variant"] == 10 and info["kernel"] == ONE + "true, " + form and info["bytes"] == n, info
            want[[5, n - 2]] ^= 0xFF
            assert rig.check(want, src, 3, 7, keys, offs) == (2, 5, n), (hex(z), form)
    # the same reduced key at the same stream position: ks ^ ks = 0, a plain compare
    for keys, offs in (((PS4, PS4), (77, 77)), ((PS3, PS3), (5, 5 + PERIOD)), ((PS3, PS3), (OFFSETS[2] + PERIOD, OFFSETS[2])),
                       ((12345, (12345 - ((1 << 31) - 1)) & 0xFFFFFFFF), (3, 3))):
        assert rig.check(src, src, 4, 4, keys, offs) == (0, NONE, n), (keys, offs)
        info = gpu.last_launch()
        assert info["variant"] == 10 and info["kernel"] == ONE + "false, false>", info
        assert rig.check(other, src, 1, 2, keys, offs) == (2, 5, n), (keys, offs)
        assert gpu.last_launch()["kernel"] == ONE + "true, false>"
    rig.free()


def test_planted_mismatches(gpu, oracle):
    """Bytes flipped on the device at every place where the kernel changes hands -- index 0, the last head byte, the first body byte, the
    last byte of the cut first chunk, the first byte of a later whole chunk, the first byte of the ragged last chunk, the first tail byte,
    n - 1 --, a pair (the lowest wins), a thousand at once, a flip in src instead of expect: the exact count and the exact lowest index
    each time, at the shipped grid and on 1 and 3 workgroups; a flipped byte just outside either range changes nothing."""
    n = 5 * CHUNK + 21
    src = oracle.splitmix_bytes(n, 8)
    offs = ((1 << 40) + 9, (1 << 33) + 2)
    keys = (PS3, PS4)
    want = rekeyed(oracle, src, keys[0], offs[0], keys[1], offs[1])
    rng = np.random.default_rng(1000)
    thousand = sorted(int(x) for x in rng.choice(n, size=1000, replace=False))
    with gpu.testing_flavour():
        rig = Rig(gpu, n)
        try:
            for pe, ps in ((0, 0), (5, 3), (11, 11), (15, 2)):
                e0, s0 = BAND + pe, BAND + ps
                head = (16 - (rig.eb.ptr + e0) % 16) % 16                  # bytes in front of the aligned body
                body = (n - head) // 16 * 16
                cut = CHUNK - (rig.eb.ptr + e0 + head) % CHUNK             # bytes of the body in its first chunk
                later = head + cut + CHUNK                                 # the first byte of a later whole chunk
                ragged = head + cut + (body - cut - 1) // CHUNK * CHUNK    # the first byte of the body's last chunk
                tail = head + body                                         # the first tail byte (or n: no tail at this phase)
                assert 0 < cut <= CHUNK and later + CHUNK <= ragged < tail <= n
                spots = sorted({0, max(head - 1, 0), head, head + cut - 1, later, ragged, min(tail, n - 1), n - 1})
                plants = [[j] for j in spots] + [[later + 35, later + 33], [head + cut - 1, ragged], thousand]
                rig.put(rig.eb, want, pe, 0x5A)
                rig.put(rig.sb, src, ps, 0xA5)
                for grid in (0, 1, 3):
                    gpu.debug_set_verify_form(grid)
                    assert rig.call(n, pe, ps, keys, offs) == (0, NONE, n)
                    assert gpu.last_launch()["grid"] == (grid or gpu.last_launch()["grid"]) and gpu.last_launch()["variant"] == 12
                    for js in plants:
                        js = sorted(set(js))
                        bad = want.copy()
                        bad[js] ^= 0x01
                        for lo in range(min(js) // 4096 * 4096, max(js) + 1, 1 << 20):  # rewrite only the pages that changed
                            rig.eb.upload(bad[lo:min(n, lo + (1 << 20))], offset=e0 + lo)
                        assert rig.call(n, pe, ps, keys, offs) == (len(js), js[0], n), (pe, ps, grid, js[:4])
                        rig.eb.upload(want, offset=e0)
                    # the same found when it is src that differs
                    for j in (later + 7, n - 1):
                        rig.sb.upload(src[j:j + 1] ^ 0x80, offset=s0 + j)
                        assert rig.call(n, pe, ps, keys, offs) == (1, j, n), (pe, ps, grid, j)
                        rig.sb.upload(src[j:j + 1], offset=s0 + j)
                # just outside both ranges: one byte in front and one behind, on either side
                gpu.debug_set_verify_form(0)
                for buf, base in ((rig.eb, e0), (rig.sb, s0)):
                    for at in (base - 1, base + n):
                        keep = buf.download(1, offset=at)
                        buf.upload(keep ^ 0xFF, offset=at)
                        assert rig.call(n, pe, ps, keys, offs) == (0, NONE, n), (pe, ps, at - base)
                        buf.upload(keep, offset=at)
        finally:
            gpu.debug_set_verify_form(0)
            rig.free()


def test_everything_wrong(gpu, oracle):
    """Right data, a wrong key_to, then off_to off by one: the count and the lowest index numpy gives over the oracle's bytes."""
    n = (2 << 20) + 77
    rig = Rig(gpu, n)
    src = oracle.splitmix_bytes(n, 17)
    want = rekeyed(oracle, src, PS3, 5, PS4, 6)
    for keys, offs in (((PS3, 12345), (5, 6)), ((PS3, PS4), (5, 7))):
        told = numpy_says(want, rekeyed(oracle, src, keys[0], offs[0], keys[1], offs[1]))
        assert told[0] > n * 0.99
        assert rig.check(want, src, 0, 0, keys, offs) == told
        assert rig.check(want, src, 6, 1, keys, offs) == told
    rig.free()


def test_aliases(gpu, oracle):
    """expect == src and a partial overlap are legal: the result is the oracle's, and nothing is written."""
    n = 3 * CHUNK + 5
    a = gpu.DeviceBuffer(n + 64)
    res = gpu.DeviceBuffer(32)
    data = oracle.splitmix_bytes(n + 64, 12)
    a.upload(data)
    told = numpy_says(data[3:3 + n], rekeyed(oracle, data[3:3 + n], PS3, 9, PS4, 4))
    gpu.verify_rekey_device(a.ptr + 3, a.ptr + 3, PS3, PS4, 9, 4, result=res, n=n)
    a.sync()
    assert triple(gpu.verify_results(res)[0]) == told and told[0] > 0
    told = numpy_says(data[3:3 + n], rekeyed(oracle, data[10:10 + n], PS4, 1, PS3, 0))
    assert triple(gpu.verify_rekey_device(a.ptr + 3, a.ptr + 10, PS4, PS3, 1, 0, n=n)) == told  # (a result buffer of the binding's own)
    told = numpy_says(data[40:40 + n], rekeyed(oracle, data[0:n], PS4, 1, PS3, 0))
    assert triple(gpu.verify_rekey_device(a.ptr + 40, a.ptr, PS4, PS3, 1, 0, n=n)) == told
    assert np.array_equal(a.download(), data)
    a.free()
    res.free()


def test_batch_of_forty(gpu, oracle):
    """40 entries under one key on both sides, sizes 0 .. 1 MiB, mixed phases, own offsets, overlapping sources; nine of them with
    coinciding streams (the verify kernels' share), four corrupted; every result exact and equal to the single call's, and the
    launches as the header states: 1 + ceil(two_stream / 16) + ceil(coinciding / 16)."""
    rng = np.random.default_rng(40)
    sizes = [int(x) for x in rng.integers(0, 3 * CHUNK, size=40)]
    for i, s in ((2, 1 << 20), (7, 0), (11, (1 << 20) - 3), (19, 1), (30, 0), (36, 0), (39, 15)):
        sizes[i] = s
    same = {1, 5, 7, 8, 13, 21, 22, 34, 38}  # entries whose two streams coincide (7 is empty)
    part_n = (1 << 20) + 999
    plain = oracle.splitmix_bytes(part_n, 5)
    src_offs = [int(rng.integers(0, part_n - s + 1)) for s in sizes]  # the sources overlap each other
    part = gpu.DeviceBuffer(part_n + 16)
    part.upload(plain, offset=3)
    e_offs, at = [], 0
    for i, s in enumerate(sizes):
        at += (7 * i) % 16
        e_offs.append(at)
        at += s
    offs_from = [o + (i << 33) for i, o in enumerate(src_offs)]
    offs_to = [f + (PERIOD * (i % 3) if i in same else 1 + 5 * i) for i, f in enumerate(offs_from)]
    image = np.zeros(at + 16, np.uint8)
    for s, o, q, f, t in zip(sizes, src_offs, e_offs, offs_from, offs_to):
        image[q:q + s] = rekeyed(oracle, plain[o:o + s], PS4, f, PS4, t)
    want = [(0, NONE, s) for s in sizes]
    for i, js in ((2, [CHUNK, 900000]), (19, [0]), (33, [sizes[33] - 1]), (13, [sizes[13] // 2, 3])):
        for j in js:
            image[e_offs[i] + j] ^= 0x10
        want[i] = (len(js), min(js), sizes[i])
    exp = gpu.DeviceBuffer(image.size)
    exp.upload(image)
    res = gpu.DeviceBuffer(2 * BAND + 32 * 40)
    res.upload(np.full(2 * BAND + 32 * 40, 0xEE, np.uint8))
    e_ptrs, s_ptrs = [exp.ptr + q for q in e_offs], [part.ptr + 3 + o for o in src_offs]
    before = gpu.path_stats()["gpu_launches"]
    gpu.verify_rekey_batch_device(e_ptrs, s_ptrs, sizes, PS4, PS4, res.ptr + BAND, offs_from=offs_from, offs_to=offs_to)
    res.sync()
    two = sum(1 for i, s in enumerate(sizes) if s and i not in same)
    one = sum(1 for i, s in enumerate(sizes) if s and i in same)
    assert (two, one) == (29, 8)
    assert gpu.path_stats()["gpu_launches"] - before == 1 + math.ceil(two / 16) + math.ceil(one / 16) == 4
    got = [triple(r) for r in gpu.verify_results(res.ptr + BAND, 40)]
    assert got == want
    bands = res.download()
    assert (bands[:BAND] == 0xEE).all() and (bands[BAND + 32 * 40:] == 0xEE).all(), "the bands around the results were written"
    single = gpu.DeviceBuffer(32)
    for i in range(40):
        gpu.verify_rekey_device(e_ptrs[i], s_ptrs[i], PS4, PS4, offs_from[i], offs_to[i], result=single, n=sizes[i])
        single.sync()
        assert triple(gpu.verify_results(single)[0]) == got[i], i
    assert np.array_equal(exp.download(), image) and np.array_equal(part.download(part_n, offset=3), plain)
    # NULL offset arrays mean 0 for every entry
    zero = rekeyed(oracle, plain[:CHUNK + 9], PS3, 0, PS4, 0)
    exp.upload(zero)
    gpu.verify_rekey_batch_device([exp.ptr, exp.ptr], [part.ptr + 3, part.ptr + 4], [CHUNK + 9, 0], PS3, PS4, res.ptr + BAND)
    res.sync()
    assert [triple(r) for r in gpu.verify_results(res.ptr + BAND, 2)] == [(0, NONE, CHUNK + 9), (0, NONE, 0)]
    for b in (part, exp, res, single):
        b.free()


def test_graph_replay_and_streams(gpu, oracle):
    """A captured call starts from a clean result on every replay: clean, one byte corrupted between replays -> that byte, restored ->
    clean again.  Two eager calls on two streams with results of their own are both exact."""
    n = (2 << 20) + 77
    src = oracle.splitmix_bytes(n, 21)
    want = rekeyed(oracle, src, PS3, 5, PS4, 8)
    eb, sb, res = gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(64)
    eb.upload(want, offset=1)
    sb.upload(src, offset=3)
    res.upload(np.full(64, 0xEE, np.uint8))
    st = Stream()
    with Graph.capture(st) as g:
        gpu.verify_rekey_device(eb.ptr + 1, sb.ptr + 3, PS3, PS4, 5, 8, result=res, n=n, stream=st.handle)
    at = CHUNK + 12345
    for k, (flip, expect) in enumerate(((0, (0, NONE, n)), (0x20, (1, at, n)), (0, (0, NONE, n)))):
        eb.upload(want[at:at + 1] ^ flip, offset=1 + at)
        g.launch(st)
        st.sync()
        assert triple(gpu.verify_results(res)[0]) == expect, ("graph replay", k)
    g.destroy()

    st2 = Stream()
    e2 = gpu.DeviceBuffer(n + 16)
    img = rekeyed(oracle, src, PS4, 1 << 32, PS3, 3)
    img[[1000, n - 1]] ^= 0x80
    e2.upload(img, offset=6)
    res.upload(np.full(64, 0xEE, np.uint8))
    gpu.verify_rekey_device(eb.ptr + 1, sb.ptr + 3, PS3, PS4, 5, 8, result=res.ptr, n=n, stream=st.handle)
    gpu.verify_rekey_device(e2.ptr + 6, sb.ptr + 3, PS4, PS3, 1 << 32, 3, result=res.ptr + 32, n=n, stream=st2.handle)
    st.sync()
    st2.sync()
    assert [triple(r) for r in gpu.verify_results(res, 2)] == [(0, NONE, n), (2, 1000, n)]
    st.destroy()
    st2.destroy()
    for b in (eb, sb, e2, res):
        b.free()


def test_against_the_products_own_rekey(gpu, oracle):
    """What modgpu_rekey_device_to and modgpu_rekey_batch_device_to wrote verifies clean under the same keys and offsets; one flipped
    byte of it is found."""
    n = 4 * CHUNK + 123
    src = oracle.splitmix_bytes(n, 31)
    sb, db, res = gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(32 * 3)
    sb.upload(src, offset=5)
    offs = ((1 << 35) + 7, 12)
    gpu.rekey_device_to(db.ptr + 2, sb.ptr + 5, PS3, PS4, offs[0], offs[1], n=n)
    gpu.verify_rekey_device(db.ptr + 2, sb.ptr + 5, PS3, PS4, offs[0], offs[1], result=res, n=n)
    db.sync()
    assert triple(gpu.verify_results(res)[0]) == (0, NONE, n)
    at = 2 * CHUNK + 77
    db.upload(db.download(1, offset=2 + at) ^ 0x04, offset=2 + at)
    gpu.verify_rekey_device(db.ptr + 2, sb.ptr + 5, PS3, PS4, offs[0], offs[1], result=res, n=n)
    db.sync()
    assert triple(gpu.verify_results(res)[0]) == (1, at, n)
    # the batch: three entries cut from the same buffers
    sizes = [CHUNK + 1, 0, n - 2 * CHUNK - 40]
    starts = [0, CHUNK + 20, 2 * CHUNK + 40]
    d_ptrs, s_ptrs = [db.ptr + 2 + q for q in starts], [sb.ptr + 5 + q for q in starts]
    offs_from, offs_to = [9, 0, (1 << 63) + 1], [9 + PERIOD, 5, 44]
    gpu.rekey_batch_device_to(d_ptrs, s_ptrs, sizes, PS4, PS4, offs_from=offs_from, offs_to=offs_to)
    gpu.verify_rekey_batch_device(d_ptrs, s_ptrs, sizes, PS4, PS4, res, offs_from=offs_from, offs_to=offs_to)
    db.sync()
    assert [triple(r) for r in gpu.verify_results(res, 3)] == [(0, NONE, s) for s in sizes]
    at = sizes[2] - 1
    db.upload(db.download(1, offset=2 + starts[2] + at) ^ 0x40, offset=2 + starts[2] + at)
    gpu.verify_rekey_batch_device(d_ptrs, s_ptrs, sizes, PS4, PS4, res, offs_from=offs_from, offs_to=offs_to)
    db.sync()
    assert [triple(r) for r in gpu.verify_results(res, 3)] == [(0, NONE, sizes[0]), (0, NONE, 0), (1, at, sizes[2])]
    for b in (sb, db, res):
        b.free()
