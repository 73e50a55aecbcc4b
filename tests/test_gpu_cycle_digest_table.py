"""GPU: the cycle digest table call (modgpu_cycle_digest_table_device: modgpu_cycle_table_device and one digest record per entry in the
same pass, three launches) against the oracle's cycle_at of each entry's source slice -- the destination arena byte for byte, with
everything around the entries untouched -- and zlib.adler32 of the stored bytes (DIGEST_OUTPUT) or of the source bytes (DIGEST_INPUT),
with s1, s2 and n of every record against numpy.  Every case runs a resident table on a caller's workspace with the records between
0xA5 guard bands, and checks 3 launches, a clean status and the source arena unchanged (unless it runs in place).  conftest.py sets
MODGPU_REQUIRE_GPU=1 before the library loads, so every number compared here came from a kernel."""
import ctypes
import zlib

import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
KEYS = [PS4, PS3, 1, 0xFFFFFFFF, 0x80000000, 12345, 0x7FFFFFFF, 0, 0x80000001, 0xDEADBEEF]  # test_gpu_digest_table.py's: two identity keys
CHUNK = 65536
MOD = 65521
SIZES = [0, 1, 5, 15, 16, 17, 4095, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
PERIOD = (1 << 31) - 2
OFFS = [0, 1 << 32, PERIOD - 3, PERIOD, (1 << 64) - 1, 77, (5 << 40) + 3, (1 << 63) + 12345]
GUARD = 64
SIDES = ["output", "input"]


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def side_of(M, name):
    return M.DIGEST_INPUT if name == "input" else M.DIGEST_OUTPUT


def sums(x):
    """(Adler-32 as zlib computes it, s1 mod 65521, s2 mod 65521, n) of the bytes x"""
    j = np.arange(x.size, dtype=np.uint64) % np.uint64(MOD)
    return (zlib.adler32(x.tobytes()) & 0xFFFFFFFF, int(x.sum(dtype=np.uint64)) % MOD,
            int((j * x.astype(np.uint64)).sum(dtype=np.uint64) % np.uint64(MOD)), int(x.size))


class Arena:
    """Entries of the given sizes: destinations laid one behind the other in a buffer of random bytes, entry i at phase phases[i] (mod
    64 KiB, from a chunk-aligned base) or at a random gap, each source `diffs[i]` bytes further into the chunk of a second buffer of
    random bytes (in_place: the destination itself).  Keys from KEYS and offsets from OFFS in rotation, or as given.  The reference is
    computed once: the destination image afterwards, and per entry the sums of both sides."""

    def __init__(self, M, oracle, sizes, seed, phases=None, diffs=None, keys=None, offs=None, in_place=False):
        rng = np.random.default_rng(seed)
        n = len(sizes)
        self.M, self.in_place = M, in_place
        self.sizes = np.array(sizes, dtype=np.uint64)
        diffs = [0 if in_place else int(rng.integers(0, 8)) for _ in sizes] if diffs is None else diffs
        cur, at = CHUNK, []
        for i, s in enumerate(sizes):
            if phases is not None:
                cur = (cur + CHUNK - 1) // CHUNK * CHUNK + phases[i]
            else:
                cur += int(rng.integers(0, 48))
            at.append(cur)
            cur += int(s)
        self.nbytes = cur + 64
        self.d_off = np.array(at, dtype=np.uint64)
        self.s_off = self.d_off + np.array(diffs, dtype=np.uint64)
        self.dst = M.DeviceBuffer(self.nbytes + CHUNK)
        self.d_base = (self.dst.ptr + CHUNK - 1) // CHUNK * CHUNK - self.dst.ptr  # both arenas start on a chunk edge
        self.src = self.dst if in_place else M.DeviceBuffer(self.nbytes + CHUNK + 16)
        self.s_base = self.d_base if in_place else (self.src.ptr + CHUNK - 1) // CHUNK * CHUNK - self.src.ptr
        self.keys = np.array([KEYS[(i + seed) % len(KEYS)] for i in range(n)] if keys is None else keys, dtype=np.uint32).view(np.int32)
        self.offs = np.array([OFFS[(i + 3 * seed) % len(OFFS)] for i in range(n)] if offs is None else offs, dtype=np.uint64)
        self.oracle = oracle
        self.fill(seed)

    def fill(self, seed):
        """new random bytes on both sides, uploaded; the reference follows"""
        rng = np.random.default_rng(1000 + seed)
        self.d_img = rng.integers(0, 256, size=self.nbytes, dtype=np.uint8)
        self.s_img = self.d_img if self.in_place else rng.integers(0, 256, size=self.nbytes + 16, dtype=np.uint8)
        self.reset()
        self.refer()

    def reset(self):
        self.dst.upload(self.d_img, offset=self.d_base)
        if not self.in_place:
            self.src.upload(self.s_img, offset=self.s_base)

    def refer(self):
        self.want_img = self.d_img.copy()
        self.want = {"output": [], "input": []}
        for i, n in enumerate(self.sizes):
            s, d, n = int(self.s_off[i]), int(self.d_off[i]), int(n)
            seg = self.s_img[s:s + n].copy()
            self.want["input"].append(sums(seg))
            if n:
                self.oracle.cycle_at(seg, int(self.keys[i]) & 0xFFFFFFFF, int(self.offs[i]))
            self.want["output"].append(sums(seg))
            self.want_img[d:d + n] = seg

    def table(self):
        t = self.M.table(len(self.sizes))
        t["dst"] = np.uint64(self.dst.ptr + self.d_base) + self.d_off
        t["src"] = np.uint64(self.src.ptr + self.s_base) + self.s_off
        t["n"], t["stream_off"], t["key"] = self.sizes, self.offs, self.keys
        return t

    def check(self, what):
        """the destination arena byte-identical to the reference, everything around the entries with it; the source arena unchanged"""
        got = self.dst.download(self.nbytes, offset=self.d_base)
        if not np.array_equal(got, self.want_img):
            at = int(np.flatnonzero(got != self.want_img)[0])
            raise AssertionError((what, "the destination arena differs first at", at, "entries start at", [int(x) for x in self.d_off[:12]]))
        if not self.in_place:
            assert np.array_equal(self.src.download(self.nbytes + 16, offset=self.s_base), self.s_img), (what, "the source arena changed")

    def untouched(self, what):
        assert np.array_equal(self.dst.download(self.nbytes, offset=self.d_base), self.d_img), (what, "a refused call wrote into a destination")
        if not self.in_place:
            assert np.array_equal(self.src.download(self.nbytes + 16, offset=self.s_base), self.s_img), (what, "the source arena changed")

    def free(self):
        self.dst.free()
        if not self.in_place:
            self.src.free()


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
    return tb, M.DeviceBuffer(M.cycle_digest_table_workspace_bytes(len(t)))


def run(M, a, side, what, stream=None):
    """the arena's table resident, a caller's workspace and guarded records: everything every case checks"""
    what = (what, side)
    a.reset()
    t = a.table()
    tb, ws = resident(M, t)
    res = Records(M, len(t))
    before = M.path_stats()["gpu_launches"]
    assert M.cycle_digest_table_device(tb, res.ptr, side_of(M, side), ws, n=len(t), stream=stream) is None
    M.lib().modgpu_sync(-1, ctypes.c_void_p(stream or 0))
    assert M.path_stats()["gpu_launches"] - before == 3, what
    assert M.table_status(ws) is None, what
    a.check(what)
    same(res.read(what), a.want[side], what)
    for b in (tb, ws, res):
        b.free()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("phase", [0, 1, 5, 15, 65520 + 15])
def test_edge_sizes_keys_and_offsets_at_phases(gpu, oracle, phase, side):
    """Every edge size at one destination phase (65520 + 15: a cut first chunk with a 1-byte head), the source 0, 1 and 3 bytes off it
    (funnel shifts 0, 1, 3), each under several keys (two identity keys among them) and offsets (0, 2^32, around the period, 2^64 - 1);
    one entry whose body ends exactly on a chunk edge and one that is head and tail only."""
    sizes = SIZES * 3 + [2 * CHUNK - phase % CHUNK if phase else 2 * CHUNK, 20]
    phases = [phase] * (len(sizes) - 1) + [(phase & ~15) + 9]  # the last: 7 bytes of head, 13 of tail, no body
    diffs = [0] * 11 + [1] * 11 + [3] * 11 + [3, 1]
    a = Arena(gpu, oracle, sizes, seed=phase % 11, phases=phases, diffs=diffs)
    assert {int(k) & 0xFFFFFFFF for k in a.keys} >= {0, 0x7FFFFFFF, PS3, PS4} and {int(o) for o in a.offs} >= {0, 1 << 32, (1 << 64) - 1}
    t, e = a.table(), len(sizes) - 2
    assert (int(t["dst"][e]) + int(a.sizes[e])) % CHUNK == 0 and (int(t["dst"][e + 1]) + 20) % 16 == 13 and int(t["dst"][e + 1]) % 16 == 9
    assert {(int(s) - int(d)) % 4 for s, d in zip(t["src"], t["dst"])} == {0, 1, 3}
    run(gpu, a, side, ("resident", phase))
    a.reset()
    same(gpu.cycle_digest_table_device(t, None, side_of(gpu, side)), a.want[side], ("wrapper", phase))  # uploaded by the wrapper, which waits
    a.check(("wrapper", phase))
    a.free()


@pytest.mark.parametrize("n_entries", [1, 16, 17, 1024, 1025, 4097])
def test_table_lengths(gpu, oracle, n_entries):
    rng = np.random.default_rng(n_entries)
    a = Arena(gpu, oracle, [int(x) for x in rng.integers(0, 300, size=n_entries)], seed=n_entries)
    run(gpu, a, SIDES[n_entries % 2], ("length", n_entries))
    a.free()


def test_seventy_thousand_entries(gpu, oracle):
    """70 000 entries of 16 .. 80 bytes: the entry index passes 16 bits and the search reaches its fifth level"""
    rng = np.random.default_rng(70000)
    a = Arena(gpu, oracle, [int(x) for x in rng.integers(16, 81, size=70000)], seed=7)
    run(gpu, a, "output", "70 000")
    run(gpu, a, "input", "70 000")
    a.free()


@pytest.mark.parametrize("side", SIDES)
def test_small_grids_flush_at_every_change_of_entry(gpu, oracle, side):
    """Grid forced to 1, 2 and 3 at mixed source phases: runs of one-chunk entries (a flush at every chunk), an 8-chunk entry split
    over the workgroups, empty entries and entries without a body between them."""
    sizes = [CHUNK] * 5 + [0, 7, 8 * CHUNK - 100, 0, 3] + [CHUNK - 1, CHUNK + 1, 15, 2 * CHUNK, 40000, 0, CHUNK, CHUNK]
    phases = [0] * 5 + [3, 9, 50, 1, 2] + [1, 65535, 0, 0, 30000, 5, 16, 65520]
    diffs = [0, 1, 2, 3, 5, 0, 1, 3, 0, 2, 1, 3, 0, 4, 7, 0, 2, 1]
    a = Arena(gpu, oracle, sizes, seed=3, phases=phases, diffs=diffs)
    with gpu.testing_flavour():
        try:
            for grid in (1, 2, 3):
                gpu.debug_set_cycle_digest_table_grid(grid)
                run(gpu, a, side, ("grid", grid))
                assert gpu.last_launch()["grid"] == grid
        finally:
            gpu.debug_set_cycle_digest_table_grid(0)
        run(gpu, a, side, "shipped grid, testing flavour")
    a.free()


def closed_form(n):
    """Adler-32 of n bytes 0xFF"""
    return ((n + 255 * (n * (n + 1) // 2)) % MOD) << 16 | (1 + 255 * n) % MOD


@pytest.mark.parametrize("n,grid", [(CHUNK, 0), ((32 << 20) + 77, 1)])
def test_widths_on_all_ff(gpu, oracle, n, grid):
    """The output is all 0xFF (the source is cycle_at of 0xFF fill), the destination at phase 16 and the source 5 bytes off it: at
    65 536 bytes the per-chunk 32-bit sums are at their bounds; at 32 MiB + 77 on ONE workgroup every lane passes 512 chunks and its
    sums pass 2^32.  Then the 0xFF bytes themselves as the source, under the identity key, on the input side."""
    off = (1 << 32) + 5
    src = np.full(n, 0xFF, np.uint8)
    oracle.cycle_at(src, PS3, off)
    sbuf, dbuf = gpu.DeviceBuffer(n + 3 * CHUNK), gpu.DeviceBuffer(n + 3 * CHUNK)
    d_at = (dbuf.ptr + CHUNK - 1) // CHUNK * CHUNK - dbuf.ptr + CHUNK + 16  # (a chunk in: 64 guard bytes lie in front of it)
    s_at = (sbuf.ptr + CHUNK - 1) // CHUNK * CHUNK - sbuf.ptr + CHUNK + 16 + 5
    sbuf.upload(src, offset=s_at)
    dbuf.upload(np.full(n + 128, 0x11, np.uint8), offset=d_at - 64)
    t = gpu.table(1)
    with gpu.testing_flavour():
        try:
            gpu.debug_set_cycle_digest_table_grid(grid)
            t[0] = (dbuf.ptr + d_at, sbuf.ptr + s_at, n, off, gpu.as_int32(PS3), 0)
            rec, adler = gpu.cycle_digest_table_device(t, None, gpu.DIGEST_OUTPUT)
            assert int(adler[0]) == closed_form(n) and int(rec["n"][0]) == n and int(rec["s1"][0]) % MOD == 255 * n % MOD
            got = dbuf.download(n + 128, offset=d_at - 64)
            assert (got[64:64 + n] == 0xFF).all() and (got[:64] == 0x11).all() and (got[64 + n:] == 0x11).all()
            assert np.array_equal(sbuf.download(n, offset=s_at), src)
            # the stored 0xFF bytes as the source of a copy, summed as read
            t[0] = (sbuf.ptr + s_at, dbuf.ptr + d_at, n, off, 0x7FFFFFFF, 0)
            rec, adler = gpu.cycle_digest_table_device(t, None, gpu.DIGEST_INPUT)
            assert int(adler[0]) == closed_form(n) and int(rec["n"][0]) == n and int(rec["s1"][0]) % MOD == 255 * n % MOD
            assert (sbuf.download(n, offset=s_at) == 0xFF).all()
        finally:
            gpu.debug_set_cycle_digest_table_grid(0)
    sbuf.free()
    dbuf.free()


@pytest.mark.parametrize("side", SIDES)
def test_in_place(gpu, oracle, side):
    """dst == src for a whole table; on the input side the records are of the bytes as they were before the call"""
    sizes = SIZES + [2 * CHUNK + 33, 700, 0, CHUNK]
    phases = [0, 1, 5, 15, 65535, 16, 3, 65520, 7, 0, 9, 65000, 1, 2, 0]
    a = Arena(gpu, oracle, sizes, seed=21, phases=phases, in_place=True)
    t = a.table()
    assert np.array_equal(t["dst"], t["src"])
    run(gpu, a, side, "in place")
    a.free()


def test_entry_beyond_4_gib(gpu, oracle):
    """One entry of 2^32 + 3 * 65536 + 77 bytes of 0xFF, run in place: under the identity key both sides against the closed form; under
    PS4 from ptr + 3 the output record against modgpu_digest_table_device's record of the same range taken just before, a 1 MiB window
    at either end against the oracle, and a second call that restores 0xFF with the closed form as its output record."""
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
    t = gpu.table(1)
    tb, ws = resident(gpu, t)
    res, res_d = Records(gpu, 1), Records(gpu, 1)

    def call(entry, side):
        t[0] = entry
        tb.upload(t.view(np.uint8))
        res.fill()
        gpu.cycle_digest_table_device(tb, res.ptr, side, ws, n=1)
        buf.sync()
        assert gpu.table_status(ws) is None
        return res.read("big")

    for side in (gpu.DIGEST_OUTPUT, gpu.DIGEST_INPUT):
        rec, adler = call((buf.ptr, buf.ptr, n, 9, 0x7FFFFFFF, 0), side)
        assert int(adler[0]) == closed_form(n) and int(rec["n"][0]) == n, side
    keyed = (buf.ptr + 3, buf.ptr + 3, n, off, gpu.as_int32(PS4), 0)
    t[0] = keyed
    tb.upload(t.view(np.uint8))
    gpu.digest_table_device(tb, res_d.ptr, ws, n=1)
    buf.sync()
    rec_d, adler_d = res_d.read("digest table")
    rec, adler = call(keyed, gpu.DIGEST_OUTPUT)
    assert int(adler[0]) == int(adler_d[0]) and int(rec["n"][0]) == n
    assert int(rec["s1"][0]) % MOD == int(rec_d["s1"][0]) % MOD and int(rec["s2"][0]) % MOD == int(rec_d["s2"][0]) % MOD
    W = 1 << 20
    for at in (0, n - W):
        seg = np.full(W, 0xFF, np.uint8)
        oracle.cycle_at(seg, PS4, off % PERIOD + at)  # (positions are off + j, reduced mod the period, never mod 2^64)
        assert np.array_equal(buf.download(W, offset=3 + at), seg), at
    assert (buf.download(3) == 0xFF).all() and (buf.download(61, offset=3 + n) == 0xFF).all()
    rec, adler = call(keyed, gpu.DIGEST_OUTPUT)
    assert int(adler[0]) == closed_form(n)
    assert (buf.download(W) == 0xFF).all() and (buf.download(W, offset=n + 64 - W) == 0xFF).all()
    for b in (tb, ws, res, res_d, buf):
        b.free()


@pytest.mark.parametrize("side", SIDES)
def test_against_the_existing_calls(gpu, oracle, side):
    """One resident table through cycle_table_device + digest_table_device, then through this call into a second destination: the
    destinations match byte for byte; on the output side the records match, on the input side they are those of digest_table_device
    over the same sources under the identity key."""
    a = Arena(gpu, oracle, [4097, CHUNK + 3, 0, 17, 2 * CHUNK + 9, 1000, 3 * CHUNK, 15], seed=6)
    t = a.table()
    tb, ws = resident(gpu, t)
    res_d, res = Records(gpu, len(t)), Records(gpu, len(t))
    gpu.cycle_table_device(tb, ws, n=len(t))
    if side == "input":
        plain = t.copy()
        plain["key"] = 0
        tb.upload(plain.view(np.uint8))
    gpu.digest_table_device(tb, res_d.ptr, ws, n=len(t))  # (one stream: each call takes the workspace after the one before)
    a.dst.sync()
    first = a.dst.download(a.nbytes, offset=a.d_base)
    rec_d, adler_d = res_d.read("two calls")
    a.reset()
    tb.upload(t.view(np.uint8))
    gpu.cycle_digest_table_device(tb, res.ptr, side_of(gpu, side), ws, n=len(t))
    a.dst.sync()
    assert gpu.table_status(ws) is None
    rec, adler = res.read("one call")
    assert np.array_equal(a.dst.download(a.nbytes, offset=a.d_base), first)
    assert np.array_equal(adler, adler_d) and np.array_equal(rec["s1"] % MOD, rec_d["s1"] % MOD) and np.array_equal(rec["s2"] % MOD, rec_d["s2"] % MOD)
    assert np.array_equal(rec["n"], rec_d["n"])
    a.check("one call")
    same((rec, adler), a.want[side], "one call")
    for b in (tb, ws, res, res_d, a):
        b.free()


@pytest.mark.parametrize("side", SIDES)
def test_graph_replay_follows_the_table_and_the_source(gpu, oracle, side):
    """Captured once (a linear capture on one stream), replayed twice with one entry's key and the source rewritten between the replays:
    destinations and records follow -- every replay starts clean, and there is no memset node to do it."""
    a = Arena(gpu, oracle, [int(x) for x in np.random.default_rng(8).integers(0, 3 * CHUNK, size=40)], seed=8)
    t = a.table()
    tb, ws = resident(gpu, t)
    res = Records(gpu, len(t))
    st = Stream()
    with Graph.capture(st) as g:
        gpu.cycle_digest_table_device(tb, res.ptr, side_of(gpu, side), ws, n=len(t), stream=st.handle)
    for k in range(2):
        if k:
            a.keys[17] = gpu.as_int32(KEYS[(k + 4) % len(KEYS)])
            a.fill(200 + k)
            tb.upload(a.table().view(np.uint8))
        g.launch(st)
        st.sync()
        assert gpu.table_status(ws) is None
        a.check(("replay", k))
        same(res.read(("replay", k)), a.want[side], ("replay", k))
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
    for i, ((tb, ws, res), st) in enumerate(zip(rigs, streams)):
        gpu.cycle_digest_table_device(tb, res.ptr, side_of(gpu, SIDES[i]), ws, n=60, stream=st.handle)
    for i, (a, (tb, ws, res), st) in enumerate(zip(arenas, rigs, streams)):
        st.sync()
        assert gpu.table_status(ws) is None
        a.check("two streams")
        same(res.read("two streams"), a.want[SIDES[i]], "two streams")
        for b in (tb, ws, res, a):
            b.free()
        st.destroy()


@pytest.mark.parametrize("what", ["null src", "null dst", "flags", "1 TiB"])
def test_device_tier_refusal_writes_nothing(gpu, oracle, what):
    """A bad entry in the middle of a table of 1500 (and a second one above it): no destination byte and no record is written, the
    status names the lowest bad entry, the wrapper raises; the mended table runs clean on the same workspace."""
    rng = np.random.default_rng(15)
    a = Arena(gpu, oracle, [int(x) for x in rng.integers(1, 200, size=1500)], seed=15)
    good = a.table()
    tb, ws = resident(gpu, good)
    res = Records(gpu, 1500)
    at = 1027
    t = good.copy()
    for i in (at, at + 300):
        if what == "null src":
            t["src"][i] = 0
        elif what == "null dst":
            t["dst"][i] = 0
        elif what == "flags":
            t["flags"][i] = 1 << (i % 32)
        else:
            t["n"][i] = (1 << 40) + CHUNK  # (2^24 + 1 chunks or more at any phase)
    tb.upload(t.view(np.uint8))
    before = gpu.path_stats()["gpu_launches"]
    gpu.cycle_digest_table_device(tb, res.ptr, gpu.DIGEST_OUTPUT, ws, n=1500)
    a.dst.sync()
    assert gpu.path_stats()["gpu_launches"] - before == 3
    assert gpu.table_status(ws) == at
    assert (res.raw(("refused", at)) == 0xA5).all(), "a refused call wrote records"
    a.untouched(what)
    with pytest.raises(gpu.ModGpuError, match=f"entry {at};"):
        gpu.cycle_digest_table_device(t)
    a.untouched(what)
    tb.upload(good.view(np.uint8))
    gpu.cycle_digest_table_device(tb, res.ptr, gpu.DIGEST_INPUT, ws, n=1500)
    a.dst.sync()
    assert gpu.table_status(ws) is None
    a.check("mended")
    same(res.read("mended"), a.want["input"], "mended")
    for b in (tb, ws, res, a):
        b.free()


def test_host_tier_queues_nothing(gpu, oracle):
    a = Arena(gpu, oracle, [100, 200, 300], seed=2)
    tb, ws = resident(gpu, a.table())
    res = Records(gpu, 3)
    host = np.zeros(3 * 4, np.uint64)
    L = gpu.lib()
    wb = gpu.cycle_digest_table_workspace_bytes(3)
    before = gpu.path_stats()["gpu_launches"]
    assert L.modgpu_cycle_digest_table_device(tb.ptr, 3, res.ptr, 2, ws.ptr, wb, -1, None) == 1
    assert "side is neither" in L.modgpu_last_error().decode()
    assert L.modgpu_cycle_digest_table_device(tb.ptr, 3, res.ptr + 4, 0, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_cycle_digest_table_device(tb.ptr, 3, host.ctypes.data, 0, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_cycle_digest_table_device(tb.ptr, 3, None, 1, ws.ptr, wb, -1, None) == 1
    assert "null results" in L.modgpu_last_error().decode()
    assert L.modgpu_cycle_digest_table_device(tb.ptr, 3, res.ptr, 1, ws.ptr, wb - 8, -1, None) == 1
    assert L.modgpu_cycle_digest_table_device(None, 3, res.ptr, 0, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_cycle_digest_table_device(tb.ptr, (1 << 22) + 1, res.ptr, 0, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_cycle_digest_table_device(None, 0, None, 0, None, 0, -1, None) == 0
    assert gpu.path_stats()["gpu_launches"] == before
    assert (res.raw("tier 1") == 0xA5).all()
    a.untouched("tier 1")
    rec, adler = gpu.cycle_digest_table_device(gpu.table(0))
    assert rec.size == 0 and adler.size == 0
    for b in (tb, ws, res):
        b.free()
    run(gpu, a, "output", "after the refusals")
    a.free()


def test_reporting(gpu, oracle):
    a = Arena(gpu, oracle, [3 * CHUNK + 5, 17], seed=4)
    run(gpu, a, "output", "reporting")
    info = gpu.last_launch()
    assert info["variant"] == 18 and info["bytes"] == 0 and info["kernel"] == "modgpu_cycle_table_kernel<4, 1024>", info
    assert info["grid"] >= 1 and info["block"] == 1024 and info["chunk_bytes"] == CHUNK and info["source_hash"] == gpu.table_kernel_source_hash(), info
    gpu.cycle_table_device(a.table())
    assert gpu.last_launch()["variant"] == 8
    a.reset()
    tb, ws = resident(gpu, a.table())
    res = Records(gpu, 2)
    assert gpu.time_cycle_digest_table_device(tb, 2, res.ptr, ws, gpu.DIGEST_INPUT, iters=2) > 0
    same(res.read("timed"), a.want["input"], "timed")
    a.check("timed")
    for b in (tb, ws, res, a):
        b.free()


def test_device_buffer_extract(gpu, oracle):
    n = 5 * CHUNK + 100
    img = np.random.default_rng(55).integers(0, 256, size=n, dtype=np.uint8)
    d, out = gpu.DeviceBuffer(n), gpu.DeviceBuffer(n)
    d.upload(img)
    out.upload(np.full(n, 0x33, np.uint8))
    ranges = [(0, 100), (100, CHUNK), (CHUNK + 7, 0), (CHUNK + 777, 3 * CHUNK + 1), (n - 15, 15)]
    part_off = (1 << 33) + 5
    want, plain = [], []
    for o, m in ranges:
        seg = img[o:o + m].copy()
        plain.append(zlib.adler32(seg.tobytes()) & 0xFFFFFFFF)
        if m:
            oracle.cycle_at(seg, PS3, part_off + o)
        want.append(seg)
    packed = np.concatenate(want)
    got = d.extract(ranges, PS3, out, part_off)
    assert [int(g) for g in got] == [zlib.adler32(w.tobytes()) & 0xFFFFFFFF for w in want]
    after = out.download()
    assert np.array_equal(after[:packed.size], packed) and (after[packed.size:] == 0x33).all() and np.array_equal(d.download(), img)
    assert [int(g) for g in d.extract(ranges, PS3, out, part_off, side=gpu.DIGEST_INPUT)] == plain
    # in place: each range cycled where it lies, the rest of the part as it was
    got = d.extract(ranges, PS3, d, part_off, side=gpu.DIGEST_INPUT)
    assert [int(g) for g in got] == plain
    image = img.copy()
    for (o, m), w in zip(ranges, want):
        image[o:o + m] = w
    assert np.array_equal(d.download(), image) and d.extract([], PS3, out).size == 0
    d.free()
    out.free()
