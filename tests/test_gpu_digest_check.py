"""GPU: the digest check (modgpu_digest_check_device: digest records against a manifest of Adler-32 values, on the device, in two
launches).  The shapes are the smallest at which one thread per entry can go wrong -- lane, wave and workgroup edges -- not workload
sizes.  Synthetic records are closed here with Python's big integers (an independent restatement of include/modgpu.h, not
modgpu_digest_adler32); the records of the real producers are checked against zlib.adler32 of the oracle's cycle_at.  conftest.py sets
MODGPU_REQUIRE_GPU=1 before the library loads, so every record compared here came from a kernel."""
import ctypes
import zlib

import numpy as np
import pytest

from hip_rt import Graph, Stream
from test_gpu_digest_table import CHUNK, KEYS, OFFS, PS3, PS4, SIZES, Arena, Records, resident

pytestmark = pytest.mark.gpu

MOD = 65521
NONE = (1 << 64) - 1
GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def close(s1, s2, n):
    """the Adler-32 of a record, as include/modgpu.h defines it, in integers of any size"""
    s1, s2, n = s1 % MOD, s2 % MOD, n % MOD
    return ((n + n * s1 - s2) % MOD) << 16 | (1 + s1) % MOD


class Out:
    """the summary and the bitmap of a check, each between 64 guard bytes, everything pre-filled with 0xA5"""

    def __init__(self, M, n):
        self.M, self.n, self.words = M, n, (n + 63) // 64
        self.buf = M.DeviceBuffer(3 * GUARD + 32 + 8 * self.words)
        self.fill()

    def fill(self):
        self.buf.upload(np.full(self.buf.nbytes, FILL, np.uint8))

    @property
    def summary(self):
        return self.buf.ptr + GUARD

    @property
    def bits(self):
        return self.buf.ptr + 2 * GUARD + 32

    def read(self, what):
        """(the summary's four fields, the bitmap's words) after checking the guard bytes"""
        raw = self.buf.download()
        for at in (0, GUARD + 32, 2 * GUARD + 32 + 8 * self.words):
            assert (raw[at:at + GUARD] == FILL).all(), (what, "guard bytes were written", at)
        s = raw[GUARD:GUARD + 32].view("<u8")
        return [int(x) for x in s], raw[2 * GUARD + 32:2 * GUARD + 32 + 8 * self.words].view("<u8")

    def free(self):
        self.buf.free()


def expect_outcome(out, n, bad, what, with_bits=True):
    """the summary, every word of the bitmap (zero tail bits included) or its untouched pattern, the guards, and the wrapper's triple"""
    bad = sorted(bad)
    summary, words = out.read(what)
    assert summary == [len(bad), bad[0] if bad else NONE, n, 0], (what, summary)
    if with_bits:
        want = np.zeros(out.words, dtype="<u8")
        for i in bad:
            want[i // 64] |= np.uint64(1 << (i % 64))
        assert np.array_equal(words, want), (what, "bitmap")
        got = out.M.digest_check_result(out.summary, n, out.bits)
        assert (got[0], got[1], got[2].tolist()) == (len(bad), bad[0] if bad else None, bad), what
    else:
        assert (words.view(np.uint8) == FILL).all(), (what, "a bitmap that was not asked for was written")
        assert out.M.digest_check_result(out.summary, n) == (len(bad), bad[0] if bad else None, None), what


def sync(M, stream=None):
    assert M.lib().modgpu_sync(-1, ctypes.c_void_p(stream or 0)) == 0


# ---- 1. synthetic records, no producer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049, 3079])
def test_synthetic_records(gpu, n):
    rng = np.random.default_rng(n)
    planted = [0, 65520, 65521, 1 << 63, (1 << 64) - 1]
    ns = [0, 1, 65520, 65521, 65522, (1 << 32) + 5, (1 << 40) - 1]
    rec = np.zeros(n, dtype=gpu.DIGEST_RESULT_DTYPE)
    rec["s1"] = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    rec["s2"] = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    for i in range(n):
        if i % 3 == 1:
            rec["s1"][i] = planted[i // 3 % 5]
        if i % 4 == 2:
            rec["s2"][i] = planted[i // 4 % 5]
        rec["n"][i] = ns[(i + i // 7) % 7]
    if n >= 63:
        assert {int(x) for x in rec["s1"]} >= set(planted) and {int(x) for x in rec["s2"]} >= set(planted) and {int(x) for x in rec["n"]} == set(ns)
    good = np.array([close(int(r["s1"]), int(r["s2"]), int(r["n"])) for r in rec], dtype=np.uint32)
    records, expect = gpu.DeviceBuffer(32 * n), gpu.DeviceBuffer(4 * n)
    records.upload(rec.view(np.uint8))
    sets = [set(), {0}, {n - 1}] + [{i} for i in (63, 64, 1023, 1024) if i < n] + [set(range(n)), {int(i) for i in np.flatnonzero(rng.random(n) < 0.05)}]
    for bad in sets:
        want = good.copy()
        for k, i in enumerate(sorted(bad)):  # by turns a value that differs in the A half only, and in the B half only
            want[i] ^= np.uint32(1 << (k // 2 % 16 + (16 if k % 2 else 0)))
        expect.upload(want.view(np.uint8))
        for with_bits in (True, False):
            out = Out(gpu, n)
            before = gpu.path_stats()["gpu_launches"]
            assert gpu.digest_check_device(records, expect, n, None, out.summary, out.bits if with_bits else None) is None
            sync(gpu)
            assert gpu.path_stats()["gpu_launches"] - before == 2
            info = gpu.last_launch()
            assert info["variant"] == 19 and info["bytes"] == 0 and info["kernel"] == "modgpu_cycle_verify_table_finish", info
            assert info["grid"] == (n + 1023) // 1024 and info["block"] == 1024 and info["source_hash"] == gpu.verify_table_kernel_source_hash(), info
            expect_outcome(out, n, bad, (n, len(bad), with_bits), with_bits)
            out.free()
        assert np.array_equal(records.download(), rec.view(np.uint8)) and np.array_equal(expect.download(), want.view(np.uint8)), "the inputs changed"
    # the wrapper that makes its own summary and bitmap and takes a host manifest
    got = gpu.digest_check_device(records, want, n)
    assert (got[0], got[1], got[2].tolist()) == (len(bad), min(bad) if bad else None, sorted(bad))
    records.free()
    expect.free()


# ---- 2. real producers -------------------------------------------------------------------------------------------------------------
N_REAL, BIG = 40, 10  # entry BIG is 3 chunks + 5 bytes


@pytest.fixture(scope="module")
def part(gpu, oracle):
    """one arena for the table producers -- SIZES times KEYS and OFFS in rotation -- and its reference, computed once"""
    a = Arena(gpu, oracle, (SIZES * 4)[:N_REAL], seed=5)
    assert len({int(k) for k in a.keys}) == len(KEYS) and len({int(o) for o in a.offs}) == len(OFFS) and int(a.sizes[BIG]) == 3 * CHUNK + 5
    a.want()
    yield a
    a.free()


def flipped(a, k, at):
    """context: byte `at` of entry k's source flipped in the device arena, and put back"""
    class Flip:
        def __enter__(self):
            o = int(a.off[k]) + at
            a.buf.upload(a.img[o:o + 1] ^ np.uint8(0x40), offset=a.base + o)

        def __exit__(self, *exc):
            o = int(a.off[k]) + at
            a.buf.upload(a.img[o:o + 1], offset=a.base + o)
    return Flip()


def edge_byte(a, k):
    """a byte of entry k that lies in the < 16 ragged bytes at one of its ends (the finish launch sums it), from the source's phase"""
    n = int(a.sizes[k])
    at = 0 if a.addr(k) % 16 else n - 1
    assert a.addr(k) % 16 or (a.addr(k) + n) % 16
    return at


@pytest.mark.parametrize("producer", ["digest_table", "cycle_digest_table_output", "cycle_digest_table_input", "digest_batch"])
def test_real_producers(gpu, oracle, part, producer):
    if producer == "digest_batch":  # one key for all entries, 17 of them: two launches of the producer
        a = Arena(gpu, oracle, (SIZES * 2)[:17], seed=17, keys=[PS4] * 17)
        big = BIG
    else:
        a, big = part, BIG
    n = len(a.sizes)
    t = a.table()
    want = np.array([row[0] for row in a.want()], dtype=np.uint32)
    own = []
    if producer.startswith("cycle_digest_table"):
        dst = gpu.DeviceBuffer(int(a.sizes.sum()) + 16 * n + 64)
        own.append(dst)
        at, cur = [], 7
        for s in a.sizes:
            at.append(cur)
            cur += int(s) + 13
        t["dst"] = dst.ptr + np.array(at, dtype=np.uint64)
        if producer.endswith("input"):
            want = np.array([zlib.adler32(a.img[int(o):int(o) + int(s)].tobytes()) & 0xFFFFFFFF for o, s in zip(a.off, a.sizes)], dtype=np.uint32)
    tb, ws = resident(gpu, t)
    res = Records(gpu, n)
    expect = gpu.DeviceBuffer(4 * n)
    expect.upload(want.view(np.uint8))
    own += [tb, ws, res, expect]

    def produce_and_check(what, bad):
        res.fill()
        out = Out(gpu, n)
        if producer == "digest_table":
            gpu.digest_table_device(tb, res.ptr, ws, n=n)
        elif producer == "digest_batch":
            gpu.digest_batch_device([int(x) for x in t["src"]], [int(x) for x in t["n"]], PS4, res.ptr, stream_offs=[int(x) for x in t["stream_off"]])
        else:
            gpu.cycle_digest_table_device(tb, res.ptr, gpu.DIGEST_INPUT if producer.endswith("input") else gpu.DIGEST_OUTPUT, ws, n=n)
        before = gpu.path_stats()["gpu_launches"]
        gpu.digest_check_device(res.ptr, expect, n, None if producer == "digest_batch" else ws, out.summary, out.bits)
        sync(gpu)
        assert gpu.path_stats()["gpu_launches"] - before == 2
        res.raw(what)  # (the guard bytes around the records)
        expect_outcome(out, n, bad, (producer, what))
        out.free()

    produce_and_check("clean", [])
    with flipped(a, big, edge_byte(a, big)):
        produce_and_check("an edge byte flipped", [big])
    with flipped(a, big, CHUNK + 100):
        produce_and_check("a body byte flipped", [big])
    produce_and_check("put back", [])
    a.unchanged(producer)
    # the wrapper with its own buffers and a host manifest: (0, None, [])
    got = gpu.digest_check_device(res.ptr, want, n, None if producer == "digest_batch" else ws)
    assert got[0] == 0 and got[1] is None and got[2].size == 0 and got[2].dtype == np.uint64
    for b in own:
        b.free()
    if a is not part:
        a.free()


# ---- 3. a refused producer ---------------------------------------------------------------------------------------------------------
def test_refused_producer(gpu, oracle, part):
    n = N_REAL
    t = part.table()
    t["flags"][5] = 1
    tb, ws = resident(gpu, t)
    res = Records(gpu, n)
    expect = gpu.DeviceBuffer(4 * n)
    expect.upload(np.array([row[0] for row in part.want()], dtype=np.uint32).view(np.uint8))
    out = Out(gpu, n)
    gpu.digest_table_device(tb, res.ptr, ws, n=n)
    before = gpu.path_stats()["gpu_launches"]
    gpu.digest_check_device(res.ptr, expect, n, ws, out.summary, out.bits)
    sync(gpu)
    assert gpu.path_stats()["gpu_launches"] - before == 2 and gpu.table_status(ws) == 5
    summary, words = out.read("refused")
    assert summary == [0, NONE, n, 1] and (words.view(np.uint8) == FILL).all(), summary
    assert (res.raw("refused") == FILL).all()
    host = np.zeros(1, dtype=gpu.DIGEST_CHECK_SUMMARY_DTYPE)
    assert gpu.lib().modgpu_digest_check_summary(out.summary, -1, host.ctypes.data) == 1  # MODGPU_ERR_INVALID
    assert [int(host[k][0]) for k in host.dtype.names] == [0, NONE, n, 1]
    with pytest.raises(gpu.ModGpuError, match="was refused"):
        gpu.digest_check_result(out.summary, n, out.bits)
    with pytest.raises(gpu.ModGpuError, match="was refused"):
        gpu.digest_check_device(res.ptr, expect, n, ws)
    # without the workspace the same records are taken as they are: the pattern closes to no entry's checksum
    out.fill()
    gpu.digest_check_device(res.ptr, expect, n, None, out.summary, out.bits)
    sync(gpu)
    expect_outcome(out, n, range(n), "pattern records")
    for b in (tb, ws, res, expect, out):
        b.free()


# ---- 4. one captured graph: digest table + check -----------------------------------------------------------------------------------
def test_graph_of_digest_table_and_check(gpu, oracle, part):
    n = N_REAL
    t = part.table()
    want = np.array([row[0] for row in part.want()], dtype=np.uint32)
    tb, ws = resident(gpu, t)
    res = Records(gpu, n)
    expect = gpu.DeviceBuffer(4 * n)
    expect.upload(want.view(np.uint8))
    out = Out(gpu, n)
    st = Stream()
    with Graph.capture(st) as g:  # (linear: one stream, no parallel branch)
        gpu.digest_table_device(tb, res.ptr, ws, n=n, stream=st.handle)
        gpu.digest_check_device(res.ptr, expect, n, ws, out.summary, out.bits, stream=st.handle)

    def replay():
        g.launch(st)
        st.sync()
    replay()
    expect_outcome(out, n, [], "first replay")
    expect.upload((want[7:8] ^ np.uint32(1 << 20)).view(np.uint8), offset=4 * 7)
    replay()
    expect_outcome(out, n, [7], "expect[7] rewritten")
    bad_table = t.copy()
    bad_table["flags"][3] = 2
    tb.upload(bad_table.view(np.uint8))
    before, _ = out.read("before the refused replay")
    replay()
    summary, words = out.read("refused replay")
    assert summary == [0, NONE, n, 1] and np.array_equal(words, np.array([1 << 7], dtype="<u8")), "a refused replay leaves the bitmap as it was"
    tb.upload(t.view(np.uint8))
    expect.upload(want.view(np.uint8))
    replay()
    expect_outcome(out, n, [], "both restored")
    assert gpu.table_status(ws) is None and before == [1, 7, n, 0]
    g.destroy()
    st.destroy()
    for b in (tb, ws, res, expect, out):
        b.free()


# ---- 5. tier 1 on the device -------------------------------------------------------------------------------------------------------
def test_host_tier_queues_nothing(gpu):
    n = 70
    records, expect, ws = gpu.DeviceBuffer(32 * n), gpu.DeviceBuffer(4 * n), gpu.DeviceBuffer(64)
    out = Out(gpu, n)
    host = np.zeros(4 * n + 8, np.uint64)
    L = gpu.lib()
    r, e, w, s, b, h = records.ptr, expect.ptr, ws.ptr, out.summary, out.bits, host.ctypes.data
    before = gpu.path_stats()["gpu_launches"]
    texts = []

    def refused(*args):
        assert L.modgpu_digest_check_device(*args, -1, None) == 1, args
        texts.append(L.modgpu_last_error().decode().split(": ")[-1])
    foreign = "the records, the manifest, the summary or the bits are not device memory of the call's device"
    meet = "the summary or the bits overlap the records, the manifest or each other"
    for args, text in (((None, e, n, w, s, b), "null records, manifest or summary"), ((r, None, n, w, s, b), "null records, manifest or summary"),
                       ((r, e, n, w, None, b), "null records, manifest or summary"), ((r + 4, e, n - 1, w, s, b), "records, summary or bits not 8-byte aligned"),
                       ((r, e, n, w, s + 4, b), "records, summary or bits not 8-byte aligned"), ((r, e, n, w, s, b + 4), "records, summary or bits not 8-byte aligned"),
                       ((r, e + 2, n - 1, w, s, b), "manifest not 4-byte aligned"), ((r, e, n, w + 4, s, b), "table workspace not 8-byte aligned"),
                       ((r, e, (1 << 22) + 1, w, s, b), "more entries than a table call takes (4194304)"),
                       ((r, e, n, w, r + 64, b), meet), ((r, e, n, w, e + 8, b), meet), ((r, e, n, w, s, r + 32 * n - 8), meet), ((r, e, n, w, s, e), meet),
                       ((r, e, n, w, s, s + 24), meet),
                       ((h, e, n, w, s, b), foreign), ((r, h, n, w, s, b), foreign), ((r, e, n, w, h, b), foreign), ((r, e, n, w, s, h), foreign),
                       ((r, e, n, h, s, b), "the table workspace is not device memory of the call's device")):
        refused(*args)
        assert texts[-1] == text, (args, texts[-1])
    assert L.modgpu_digest_check_summary(h, -1, h + 64) == 1 and L.modgpu_digest_check_summary(None, -1, h) == 1
    # no entries: nothing queued, nothing touched
    assert L.modgpu_digest_check_device(r, e, 0, w, s, b, -1, None) == 0 and L.modgpu_digest_check_device(None, None, 0, None, None, None, -1, None) == 0
    sync(gpu)
    assert gpu.path_stats()["gpu_launches"] == before
    assert (out.buf.download() == FILL).all(), "a refused call, or one over no entries, wrote something"
    got = gpu.digest_check_device(r, e, 0)
    assert got[0] == 0 and got[1] is None and got[2].size == 0
    for x in (records, expect, ws, out):
        x.free()


# ---- 6. DeviceBuffer.check and extract_checked -------------------------------------------------------------------------------------
def test_device_buffer_check_and_extract_checked(gpu, oracle):
    n = 1 << 20
    rng = np.random.default_rng(66)
    img = rng.integers(0, 256, size=n, dtype=np.uint8)
    d = gpu.DeviceBuffer(n)
    d.upload(img)
    cuts = np.sort(rng.choice(np.arange(1, n), size=19, replace=False))
    ranges = [(int(o), int(e - o)) for o, e in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [n]]))]
    assert len(ranges) == 20 and sum(m for _, m in ranges) == n
    part_off = (1 << 33) + 5
    adlers = []
    for o, m in ranges:
        seg = img[o:o + m].copy()
        oracle.cycle_at(seg, PS3, part_off + o)
        adlers.append(zlib.adler32(seg.tobytes()) & 0xFFFFFFFF)
    adlers = np.array(adlers, dtype=np.uint32)
    before = gpu.path_stats()["gpu_launches"]
    got = d.check(ranges, PS3, adlers, part_off)
    assert (got[0], got[1], got[2].tolist()) == (0, None, []) and gpu.path_stats()["gpu_launches"] - before == 5
    out = gpu.DeviceBuffer(n)
    plain = d.extract(ranges, PS3, out, part_off)
    assert np.array_equal(plain, adlers) and plain.dtype == np.uint32, "extract returns what it returned"
    got_adlers, got = d.extract_checked(ranges, PS3, out, adlers, part_off)
    assert np.array_equal(got_adlers, adlers) and (got[0], got[1], got[2].tolist()) == (0, None, [])
    k = 13
    at = ranges[k][0] + ranges[k][1] // 2
    d.upload(img[at:at + 1] ^ np.uint8(1), offset=at)
    got = d.check(ranges, PS3, adlers, part_off)
    assert (got[0], got[1], got[2].tolist()) == (1, k, [k])
    got_adlers, got = d.extract_checked(ranges, PS3, out, adlers, part_off)
    assert (got[0], got[1], got[2].tolist()) == (1, k, [k]) and np.array_equal(np.flatnonzero(got_adlers != adlers), [k])
    wrong = adlers.copy()
    wrong[[0, 19]] ^= np.uint32(1)
    got = d.check(ranges, PS3, wrong, part_off)
    assert (got[0], got[1], got[2].tolist()) == (3, 0, [0, k, 19])
    d.free()
    out.free()
