"""GPU: the digest table call (modgpu_digest_table_device: a device-resident table of entries whose `dst` is ignored, three launches,
one 32-byte record per entry) against zlib.adler32 of the oracle's cycle_at of each entry's source slice, and s1, s2 and n of every
record against numpy.  Every case checks that the source arena is byte-identical afterwards, that the 64 guard bytes on either side of
the records did not change and that table_status is None.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every
number compared here came from a kernel."""
import ctypes
import zlib

import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
KEYS = [PS4, PS3, 1, 0xFFFFFFFF, 0x80000000, 12345, 0x7FFFFFFF, 0, 0x80000001, 0xDEADBEEF]  # test_gpu_verify_table.py's: INT_MIN, -1, identity keys
CHUNK = 65536
MOD = 65521
SIZES = [0, 1, 5, 15, 16, 17, 4095, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
PERIOD = (1 << 31) - 2
OFFS = [0, 1 << 32, PERIOD - 3, PERIOD, (1 << 64) - 1, 77, (5 << 40) + 3, (1 << 63) + 12345]
GUARD = 64


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def sums(out):
    """(Adler-32 as zlib computes it, s1 mod 65521, s2 mod 65521) of the bytes `out`"""
    j = np.arange(out.size, dtype=np.uint64) % np.uint64(MOD)
    return zlib.adler32(out.tobytes()) & 0xFFFFFFFF, int(out.sum(dtype=np.uint64)) % MOD, int((j * out.astype(np.uint64)).sum(dtype=np.uint64) % np.uint64(MOD))


class Arena:
    """Sources of the given sizes laid one behind the other in one buffer of random bytes, entry i at phase phases[i] (mod 64 KiB, from
    a chunk-aligned base) or at a random gap; keys from KEYS and offsets from OFFS in rotation, or as given.  `dst` of every third entry
    is NULL and of every third a garbage address: the call must not look at it."""

    def __init__(self, M, oracle, sizes, seed, phases=None, keys=None, offs=None):
        rng = np.random.default_rng(seed)
        n = len(sizes)
        self.M, self.oracle = M, oracle
        self.sizes = np.array(sizes, dtype=np.uint64)
        cur, at = CHUNK, []
        for i, s in enumerate(sizes):
            if phases is not None:
                cur = (cur + CHUNK - 1) // CHUNK * CHUNK + phases[i]
            else:
                cur += int(rng.integers(0, 48))
            at.append(cur)
            cur += int(s)
        self.nbytes = cur + 64
        self.buf = M.DeviceBuffer(self.nbytes + CHUNK)
        self.base = (self.buf.ptr + CHUNK - 1) // CHUNK * CHUNK - self.buf.ptr  # the arena starts on a chunk edge
        self.off = np.array(at, dtype=np.uint64)
        self.img = rng.integers(0, 256, size=self.nbytes, dtype=np.uint8)
        self.buf.upload(self.img, offset=self.base)
        self.keys = np.array([KEYS[(i + seed) % len(KEYS)] for i in range(n)] if keys is None else keys, dtype=np.uint32).view(np.int32)
        self.offs = np.array([OFFS[(i + 3 * seed) % len(OFFS)] for i in range(n)] if offs is None else offs, dtype=np.uint64)
        self._want = None

    def addr(self, i):
        return self.buf.ptr + self.base + int(self.off[i])

    def table(self):
        t = self.M.table(len(self.sizes))
        t["src"] = np.uint64(self.buf.ptr + self.base) + self.off
        t["dst"] = np.array([0 if i % 3 == 0 else 0xDEAD0000BEEF0001 + 8 * i if i % 3 == 1 else self.buf.ptr + i for i in range(len(t))], dtype=np.uint64)
        t["n"], t["stream_off"], t["key"] = self.sizes, self.offs, self.keys
        return t

    def want(self):
        """the reference, computed once: per entry (adler32, s1, s2, n)"""
        if self._want is None:
            rows = []
            for i, n in enumerate(self.sizes):
                seg = self.img[int(self.off[i]):int(self.off[i]) + int(n)].copy()
                if n:
                    self.oracle.cycle_at(seg, int(self.keys[i]) & 0xFFFFFFFF, int(self.offs[i]))
                rows.append(sums(seg) + (int(n),))
            self._want = rows
        return self._want

    def unchanged(self, what):
        assert np.array_equal(self.buf.download(self.nbytes, offset=self.base), self.img), (what, "the source arena changed")

    def free(self):
        self.buf.free()


class Records:
    """n records between two guard bands, pre-filled with 0xA5"""

    def __init__(self, M, n):
        self.M, self.n = M, n
        self.buf = M.DeviceBuffer(2 * GUARD + 32 * n)
        self.fill()

    @property
    def ptr(self):
        return self.buf.ptr + GUARD

    def fill(self):
        self.buf.upload(np.full(2 * GUARD + 32 * self.n, 0xA5, np.uint8))

    def raw(self, what=""):
        got = self.buf.download()
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + 32 * self.n:] == 0xA5).all(), (what, "guard bytes around the records were written")
        return got[GUARD:GUARD + 32 * self.n]

    def read(self, what=""):
        self.raw(what)
        return self.M.digest_results(self.ptr, self.n)

    def free(self):
        self.buf.free()


def same(got, want, what):
    rec, adler = got
    assert len(rec) == len(want) == len(adler), what
    for i, (a, s1, s2, n) in enumerate(want):
        g = (int(adler[i]), int(rec["s1"][i]) % MOD, int(rec["s2"][i]) % MOD, int(rec["n"][i]))
        assert g == (a, s1, s2, n) and int(rec["reserved"][i]) == 0, f"{what}: entry {i}: got {g}, want {(a, s1, s2, n)}"
        if n == 0:
            assert int(rec["s1"][i]) == 0 and int(rec["s2"][i]) == 0 and a == 1, (what, i)


def resident(M, t):
    tb = M.DeviceBuffer(t.nbytes)
    tb.upload(t.view(np.uint8))
    return tb, M.DeviceBuffer(M.digest_table_workspace_bytes(len(t)))


def run(M, a, what, stream=None):
    """the arena's table resident, a caller's workspace and guarded records: everything every case checks"""
    t = a.table()
    tb, ws = resident(M, t)
    res = Records(M, len(t))
    before = M.path_stats()["gpu_launches"]
    assert M.digest_table_device(tb, res.ptr, ws, n=len(t), stream=stream) is None
    M.lib().modgpu_sync(-1, ctypes.c_void_p(stream or 0))
    assert M.path_stats()["gpu_launches"] - before == 3, what
    assert M.table_status(ws) is None, what
    same(res.read(what), a.want(), what)
    a.unchanged(what)
    for b in (tb, ws, res):
        b.free()


@pytest.mark.parametrize("phase", [0, 1, 5, 15, 65520 + 15])
def test_edge_sizes_keys_and_offsets_at_source_phases(gpu, oracle, phase):
    """Every edge size at one source phase (65520 + 15: a cut first chunk with a 1-byte head), each under several keys (two identity
    keys among them) and offsets (0, 2^32, around the period, 2^64 - 1); one entry whose body ends exactly on a chunk edge and one that
    is head and tail only."""
    sizes = SIZES * 3 + [2 * CHUNK - phase % CHUNK if phase else 2 * CHUNK, 20]
    phases = [phase] * (len(sizes) - 1) + [(phase & ~15) + 9]  # the last: 7 bytes of head, 13 of tail, no body
    a = Arena(gpu, oracle, sizes, seed=phase % 11, phases=phases)
    assert {int(k) & 0xFFFFFFFF for k in a.keys} >= {0, 0x7FFFFFFF, PS3, PS4} and {int(o) for o in a.offs} >= {0, 1 << 32, (1 << 64) - 1}
    e = len(sizes) - 2
    assert (a.addr(e) + int(a.sizes[e])) % CHUNK == 0 and (a.addr(e + 1) + 20) % 16 == 13 and a.addr(e + 1) % 16 == 9
    got = gpu.digest_table_device(a.table())  # uploaded by the wrapper, which waits and returns (records, adler)
    same(got, a.want(), ("wrapper", phase))
    run(gpu, a, ("resident", phase))
    a.free()


@pytest.mark.parametrize("n_entries", [1, 16, 17, 1024, 1025, 4097])
def test_table_lengths(gpu, oracle, n_entries):
    rng = np.random.default_rng(n_entries)
    a = Arena(gpu, oracle, [int(x) for x in rng.integers(0, 300, size=n_entries)], seed=n_entries)
    run(gpu, a, ("length", n_entries))
    a.free()


def test_seventy_thousand_entries(gpu, oracle):
    """70 000 entries of 16 .. 80 bytes: the entry index passes 16 bits and the search reaches its fifth level"""
    rng = np.random.default_rng(70000)
    a = Arena(gpu, oracle, [int(x) for x in rng.integers(16, 81, size=70000)], seed=7)
    run(gpu, a, "70 000")
    a.free()


def test_small_grids_flush_at_every_change_of_entry(gpu, oracle):
    """Grid forced to 1, 2 and 3: runs of one-chunk entries (a flush at every chunk), an 8-chunk entry split over the workgroups,
    entries without a chunk between them."""
    sizes = [CHUNK] * 5 + [0, 7, 8 * CHUNK - 100, 0, 3] + [CHUNK - 1, CHUNK + 1, 15, 2 * CHUNK, 40000, 0, CHUNK, CHUNK]
    phases = [0] * 5 + [3, 9, 50, 1, 2] + [1, 65535, 0, 0, 30000, 5, 16, 65520]
    a = Arena(gpu, oracle, sizes, seed=3, phases=phases)
    with gpu.testing_flavour():
        try:
            for grid in (1, 2, 3):
                gpu.debug_set_digest_table_grid(grid)
                run(gpu, a, ("grid", grid))
                assert gpu.last_launch()["grid"] == grid
        finally:
            gpu.debug_set_digest_table_grid(0)
        run(gpu, a, "shipped grid, testing flavour")
    a.free()


def closed_form(n):
    """Adler-32 of n bytes 0xFF"""
    return ((n + 255 * (n * (n + 1) // 2)) % MOD) << 16 | (1 + 255 * n) % MOD


@pytest.mark.parametrize("n,grid", [(CHUNK, 0), ((32 << 20) + 77, 1)])
def test_widths_on_all_ff_output(gpu, oracle, n, grid):
    """The output is all 0xFF (the source is cycle_at of 0xFF fill): at 65 536 bytes the per-chunk 32-bit sums are at their bounds;
    at 32 MiB + 77 on ONE workgroup every lane passes 512 chunks and its sums pass 2^32."""
    off, phase = (1 << 32) + 5, 16 if grid else 0
    src = np.full(n, 0xFF, np.uint8)
    oracle.cycle_at(src, PS3, off)
    buf = gpu.DeviceBuffer(n + 2 * CHUNK)
    at = (buf.ptr + CHUNK - 1) // CHUNK * CHUNK - buf.ptr + phase
    buf.upload(src, offset=at)
    t = gpu.table(1)
    t[0] = (0, buf.ptr + at, n, off, gpu.as_int32(PS3), 0)
    with gpu.testing_flavour():
        try:
            gpu.debug_set_digest_table_grid(grid)
            rec, adler = gpu.digest_table_device(t)
        finally:
            gpu.debug_set_digest_table_grid(0)
    assert int(adler[0]) == closed_form(n) and int(rec["n"][0]) == n and int(rec["s1"][0]) % MOD == 255 * n % MOD
    assert np.array_equal(buf.download(n, offset=at), src)
    buf.free()


def test_entry_beyond_4_gib(gpu):
    """One entry of 2^32 + 3 * 65536 + 77 bytes of 0xFF under the identity key against the closed form; the same bytes under PS4 at an
    odd phase against modgpu_digest_device on the same range (a cross-check: that call's own test pins it at this size)."""
    n = (1 << 32) + 3 * CHUNK + 77
    buf = gpu.DeviceBuffer(n + 64)
    filled = 1 << 26
    buf.upload(np.full(filled, 0xFF, np.uint8))
    while filled < n + 64:  # (the identity key of the out-of-place call is a copy)
        step = min(filled, n + 64 - filled)
        gpu.cycle_device_to(buf.ptr + filled, buf.ptr, step, 0)
        filled += step
    buf.sync()
    off = (1 << 64) - 12345
    t = gpu.table(2)
    t[0] = (0, buf.ptr, n, 9, 0x7FFFFFFF, 0)
    t[1] = (1, buf.ptr + 3, n, off, gpu.as_int32(PS4), 0)
    tb, ws = resident(gpu, t)
    res = Records(gpu, 2)
    gpu.digest_table_device(tb, res.ptr, ws, n=2)
    buf.sync()
    assert gpu.table_status(ws) is None
    rec, adler = res.read("big")
    assert int(adler[0]) == closed_form(n) and int(rec["n"][0]) == n and int(rec["n"][1]) == n
    assert int(adler[1]) == gpu.digest_device(buf.ptr + 3, PS4, off, n=n)
    assert (buf.download(1 << 20, offset=n - (1 << 20)) == 0xFF).all() and (buf.download(1 << 20) == 0xFF).all()
    for b in (tb, ws, res, buf):
        b.free()


def test_same_values_as_the_batch_call(gpu, oracle):
    """19 entries sharing one key: the residues and the Adler-32 values of modgpu_digest_batch_device"""
    a = Arena(gpu, oracle, (SIZES * 2)[:19], seed=19, keys=[PS4] * 19)
    t = a.table()
    res_b = Records(gpu, 19)
    gpu.digest_batch_device([int(x) for x in t["src"]], [int(x) for x in t["n"]], PS4, res_b.ptr, stream_offs=[int(x) for x in t["stream_off"]])
    a.buf.sync()
    rb, ab = res_b.read("batch")
    rt, at = gpu.digest_table_device(t)
    assert np.array_equal(ab, at) and np.array_equal(rb["s1"] % MOD, rt["s1"] % MOD) and np.array_equal(rb["s2"] % MOD, rt["s2"] % MOD)
    assert np.array_equal(rb["n"], rt["n"])
    same((rt, at), a.want(), "table")
    a.unchanged("batch")
    res_b.free()
    a.free()


def test_one_device_table_through_the_cycle_table_and_this_call(gpu, oracle):
    """The same device-resident table goes to cycle_table_device and then here: the Adler-32 of what the first call wrote"""
    a = Arena(gpu, oracle, [4097, CHUNK + 3, 0, 17, 2 * CHUNK + 9, 1000], seed=6)
    t = a.table()
    dst = gpu.DeviceBuffer(int(a.sizes.sum()) + 64 * len(t))
    at, cur = [], 5
    for s in a.sizes:
        at.append(cur)
        cur += int(s) + 11
    t["dst"] = dst.ptr + np.array(at, dtype=np.uint64)
    tb = gpu.DeviceBuffer(t.nbytes)
    tb.upload(t.view(np.uint8))
    ws = gpu.DeviceBuffer(gpu.table_workspace_bytes(len(t)))
    res = Records(gpu, len(t))
    gpu.cycle_table_device(tb, ws, n=len(t))
    gpu.digest_table_device(tb, res.ptr, ws, n=len(t))  # (one stream: the second call takes the workspace after the first)
    dst.sync()
    assert gpu.table_status(ws) is None
    rec, adler = res.read("cycle then digest")
    wrote = dst.download()
    for i, s in enumerate(a.sizes):
        assert int(adler[i]) == zlib.adler32(wrote[at[i]:at[i] + int(s)].tobytes()) & 0xFFFFFFFF, i
    same((rec, adler), a.want(), "cycle then digest")
    a.unchanged("cycle then digest")
    for b in (tb, ws, res, dst, a):
        b.free()


def test_device_buffer_digests(gpu, oracle):
    n = 5 * CHUNK + 100
    img = np.random.default_rng(55).integers(0, 256, size=n, dtype=np.uint8)
    d = gpu.DeviceBuffer(n)
    d.upload(img)
    ranges = [(0, 100), (100, CHUNK), (CHUNK + 7, 0), (CHUNK + 777, 3 * CHUNK + 1), (n - 15, 15)]
    part_off = (1 << 33) + 5
    got = d.digests(ranges, PS3, part_off)
    for (o, m), g in zip(ranges, got):
        seg = img[o:o + m].copy()
        if m:
            oracle.cycle_at(seg, PS3, part_off + o)
        assert int(g) == zlib.adler32(seg.tobytes()) & 0xFFFFFFFF, (o, m)
    assert np.array_equal(d.download(), img) and d.digests([], PS3).size == 0
    d.free()


def test_graph_replay_follows_the_source(gpu, oracle):
    """Captured once (a linear capture on one stream), replayed three times with the source changed between the replays: the records
    follow -- every replay starts clean, and there is no memset node to do it."""
    a = Arena(gpu, oracle, [int(x) for x in np.random.default_rng(8).integers(0, 3 * CHUNK, size=40)], seed=8)
    t = a.table()
    tb, ws = resident(gpu, t)
    res = Records(gpu, len(t))
    st = Stream()
    with Graph.capture(st) as g:
        gpu.digest_table_device(tb, res.ptr, ws, n=len(t), stream=st.handle)
    for k in range(3):
        a.img = np.random.default_rng(100 + k).integers(0, 256, size=a.nbytes, dtype=np.uint8)
        a._want = None
        a.buf.upload(a.img, offset=a.base)
        g.launch(st)
        st.sync()
        assert gpu.table_status(ws) is None
        same(res.read(("replay", k)), a.want(), ("replay", k))
        a.unchanged(("replay", k))
    g.destroy()
    st.destroy()
    for b in (tb, ws, res, a):
        b.free()


def test_two_streams_two_workspaces(gpu, oracle):
    arenas = [Arena(gpu, oracle, [int(x) for x in np.random.default_rng(90 + i).integers(0, 2 * CHUNK, size=60)], seed=90 + i) for i in range(2)]
    streams = [Stream() for _ in arenas]
    rigs = []
    for a in arenas:
        tb, ws = resident(gpu, a.table())
        rigs.append((tb, ws, Records(gpu, 60)))
    for (tb, ws, res), st in zip(rigs, streams):
        gpu.digest_table_device(tb, res.ptr, ws, n=60, stream=st.handle)
    for a, (tb, ws, res), st in zip(arenas, rigs, streams):
        st.sync()
        assert gpu.table_status(ws) is None
        same(res.read("two streams"), a.want(), "two streams")
        a.unchanged("two streams")
        for b in (tb, ws, res, a):
            b.free()
        st.destroy()


@pytest.mark.parametrize("what", ["null src", "flags", "1 TiB"])
def test_device_tier_refusal_writes_no_record(gpu, oracle, what):
    """A bad entry first, in the middle and last in a table of 1500 (and a second one above it): the records keep their 0xA5, the
    status names the lowest bad entry, the wrapper raises; the mended table runs clean on the same workspace."""
    rng = np.random.default_rng(15)
    a = Arena(gpu, oracle, [int(x) for x in rng.integers(1, 200, size=1500)], seed=15)
    good = a.table()
    tb, ws = resident(gpu, good)
    res = Records(gpu, 1500)
    for at in (0, 1027, 1499):
        t = good.copy()
        for i in {at, min(at + 300, 1499)}:
            if what == "null src":
                t["src"][i] = 0
            elif what == "flags":
                t["flags"][i] = 1 << (i % 32)
            else:
                t["n"][i] = (1 << 40) + CHUNK  # (2^24 + 1 chunks or more at any phase)
        tb.upload(t.view(np.uint8))
        res.fill()
        gpu.digest_table_device(tb, res.ptr, ws, n=1500)
        a.buf.sync()
        assert gpu.table_status(ws) == at
        assert (res.raw(("refused", at)) == 0xA5).all(), "a refused call wrote records"
        with pytest.raises(gpu.ModGpuError, match=f"entry {at};"):
            gpu.digest_table_device(t)
    tb.upload(good.view(np.uint8))
    gpu.digest_table_device(tb, res.ptr, ws, n=1500)
    a.buf.sync()
    assert gpu.table_status(ws) is None
    same(res.read("mended"), a.want(), "mended")
    a.unchanged("refusals")
    for b in (tb, ws, res, a):
        b.free()


def test_host_tier_queues_nothing(gpu, oracle):
    a = Arena(gpu, oracle, [100, 200, 300], seed=2)
    tb, ws = resident(gpu, a.table())
    res = Records(gpu, 3)
    host = np.zeros(3 * 4, np.uint64)
    L = gpu.lib()
    wb = gpu.digest_table_workspace_bytes(3)
    before = gpu.path_stats()["gpu_launches"]
    assert L.modgpu_digest_table_device(tb.ptr, 3, res.ptr + 4, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_digest_table_device(tb.ptr, 3, host.ctypes.data, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_digest_table_device(tb.ptr, 3, None, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_digest_table_device(tb.ptr, 3, res.ptr, ws.ptr, wb - 8, -1, None) == 1
    assert L.modgpu_digest_table_device(None, 3, res.ptr, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_digest_table_device(tb.ptr, (1 << 22) + 1, res.ptr, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_digest_table_device(None, 0, None, None, 0, -1, None) == 0
    assert gpu.path_stats()["gpu_launches"] == before
    assert (res.raw("tier 1") == 0xA5).all()
    rec, adler = gpu.digest_table_device(gpu.table(0))
    assert rec.size == 0 and adler.size == 0
    for b in (tb, ws, res):
        b.free()
    run(gpu, a, "after the refusals")
    a.free()


def test_reporting(gpu, oracle):
    a = Arena(gpu, oracle, [3 * CHUNK + 5, 17], seed=4)
    run(gpu, a, "reporting")
    info = gpu.last_launch()
    assert info["variant"] == 17 and info["bytes"] == 0 and info["kernel"] == "modgpu_cycle_verify_table_kernel<4, 1024>", info
    assert info["grid"] >= 1 and info["block"] == 1024 and info["chunk_bytes"] == CHUNK and info["source_hash"] == gpu.verify_table_kernel_source_hash(), info
    tb, ws = resident(gpu, a.table())
    res = Records(gpu, 2)
    assert gpu.time_digest_table_device(tb, 2, res.ptr, ws, iters=2) > 0
    same(res.read("timed"), a.want(), "timed")
    for b in (tb, ws, res, a):
        b.free()
