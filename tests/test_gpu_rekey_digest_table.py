"""GPU: the rekey digest table call (modgpu_rekey_digest_table_device: modgpu_rekey_table_device and one digest record per entry in the
same pass, three launches) against the oracle's keystream applied twice to each entry's source slice -- the destination arena byte for
byte, with everything around the entries untouched -- and zlib.adler32 of the stored bytes (DIGEST_OUTPUT), of the source bytes
(DIGEST_INPUT) or of the plaintext between the two keystreams (DIGEST_PLAIN), with s1, s2 and n of every record against numpy.  Every
case runs a resident table on a caller's workspace with the records between 0xA5 guard bands, and checks 3 launches, a clean status and
the source arena unchanged (unless it runs in place).  Exact compares, nothing sampled.  conftest.py sets MODGPU_REQUIRE_GPU=1 before
the library loads, so every number compared here came from a kernel."""
import ctypes
import zlib

import numpy as np
import pytest

import keystream_domain as K
from hip_rt import Graph, Stream, hip

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
CHUNK = 65536
MOD = 65521
PERIOD = (1 << 31) - 2
SIZES = [0, 1, 5, 15, 16, 17, 4095, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
# (key_from, key_to, off_from, off_to): a conversion; one key at two offsets; key_from == 0; key_to == 0; both == 0; the same key at
# offsets equal mod 2^31-2 (the keystreams cancel).  Offsets 0, 2^32, around the period and 2^64 - 1 are among them.
PAIRS = [(PS3, PS4, 0, 0), (PS4, PS4, 1 << 32, PERIOD - 3), (0, PS4, 77, PERIOD), (PS3, 0x7FFFFFFF, (1 << 64) - 1, 5),
         (0x7FFFFFFF, 0, 1, (1 << 63) + 12345), (PS3, PS3, 1000, 1000 + 3 * PERIOD), (0x80000001, 12345, PERIOD - 1, (5 << 40) + 3)]
GUARD = 64
SIDES = ["output", "input", "plain"]


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def side_of(M, name):
    return {"output": M.DIGEST_OUTPUT, "input": M.DIGEST_INPUT, "plain": M.DIGEST_PLAIN}[name]


def sums(x):
    """(Adler-32 as zlib computes it, s1 mod 65521, s2 mod 65521, n) of the bytes x"""
    j = np.arange(x.size, dtype=np.uint64) % np.uint64(MOD)
    return (zlib.adler32(x.tobytes()) & 0xFFFFFFFF, int(x.sum(dtype=np.uint64)) % MOD,
            int((j * x.astype(np.uint64)).sum(dtype=np.uint64) % np.uint64(MOD)), int(x.size))


class Arena:
    """Entries of the given sizes: destinations laid one behind the other in a buffer of random bytes, entry i at phase phases[i] (mod
    64 KiB, from a chunk-aligned base) or at a random gap, each source `diffs[i]` bytes further into the chunk of a second buffer of
    random bytes (in_place: the destination itself).  Key pairs from PAIRS in rotation, or as given.  The reference is computed once:
    the destination image afterwards, and per entry the sums of all three sides."""

    def __init__(self, M, oracle, sizes, seed, phases=None, diffs=None, pairs=None, in_place=False):
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
        self.pairs = [PAIRS[(i + seed) % len(PAIRS)] for i in range(n)] if pairs is None else list(pairs)
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
        self.want = {s: [] for s in SIDES}
        for i, n in enumerate(self.sizes):
            s, d, n = int(self.s_off[i]), int(self.d_off[i]), int(n)
            kf, kt, of, ot = self.pairs[i]
            seg = self.s_img[s:s + n].copy()
            self.want["input"].append(sums(seg))
            if n:
                self.oracle.cycle_at(seg, kf & 0xFFFFFFFF, of)
            self.want["plain"].append(sums(seg))
            if n:
                self.oracle.cycle_at(seg, kt & 0xFFFFFFFF, ot)
            self.want["output"].append(sums(seg))
            self.want_img[d:d + n] = seg

    def table(self):
        t = self.M.rekey_table(len(self.sizes))
        t["dst"] = np.uint64(self.dst.ptr + self.d_base) + self.d_off
        t["src"] = np.uint64(self.src.ptr + self.s_base) + self.s_off
        t["n"] = self.sizes
        t["key_from"] = np.array([p[0] for p in self.pairs], dtype=np.uint32).view(np.int32)
        t["key_to"] = np.array([p[1] for p in self.pairs], dtype=np.uint32).view(np.int32)
        t["off_from"] = np.array([p[2] for p in self.pairs], dtype=np.uint64)
        t["off_to"] = np.array([p[3] for p in self.pairs], dtype=np.uint64)
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
    return tb, M.DeviceBuffer(M.rekey_digest_table_workspace_bytes(len(t)))


def run(M, a, side, what, stream=None):
    """the arena's table resident, a caller's workspace and guarded records: everything every case checks"""
    what = (what, side)
    a.reset()
    t = a.table()
    tb, ws = resident(M, t)
    res = Records(M, len(t))
    before = M.path_stats()["gpu_launches"]
    assert M.rekey_digest_table_device(tb, res.ptr, side_of(M, side), ws, n=len(t), stream=stream) is None
    M.lib().modgpu_sync(-1, ctypes.c_void_p(stream or 0))
    assert M.path_stats()["gpu_launches"] - before == 3, what
    assert M.table_status(ws) is None, what
    a.check(what)
    same(res.read(what), a.want[side], what)
    for b in (tb, ws, res):
        b.free()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("phase", [0, 65520 + 15])
def test_edge_sizes_key_pairs_and_offsets_at_phases(gpu, oracle, phase, side):
    """Every edge size at one destination phase (65520 + 15: a cut first chunk with a 1-byte head), the source 0, 1 and 3 bytes off it
    (funnel shifts 0, 1, 3), the seven key pairs in rotation -- 11 sizes against 7 pairs, so every size meets several --; one entry
    whose body ends exactly on a chunk edge and one that is head and tail only."""
    sizes = SIZES * 3 + [2 * CHUNK - phase % CHUNK if phase else 2 * CHUNK, 20]
    phases = [phase] * (len(sizes) - 1) + [(phase & ~15) + 9]  # the last: 7 bytes of head, 13 of tail, no body
    diffs = [0] * 11 + [1] * 11 + [3] * 11 + [3, 1]
    a = Arena(gpu, oracle, sizes, seed=phase % 11, phases=phases, diffs=diffs)
    assert set(a.pairs) == set(PAIRS)
    t, e = a.table(), len(sizes) - 2
    assert (int(t["dst"][e]) + int(a.sizes[e])) % CHUNK == 0 and (int(t["dst"][e + 1]) + 20) % 16 == 13 and int(t["dst"][e + 1]) % 16 == 9
    assert {(int(s) - int(d)) % 4 for s, d in zip(t["src"], t["dst"])} == {0, 1, 3}
    run(gpu, a, side, ("resident", phase))
    a.reset()
    same(gpu.rekey_digest_table_device(t, None, side_of(gpu, side)), a.want[side], ("wrapper", phase))  # uploaded by the wrapper, which waits
    a.check(("wrapper", phase))
    a.free()


@pytest.mark.parametrize("pair", range(len(PAIRS)))
def test_every_key_pair_at_every_size(gpu, oracle, pair):
    a = Arena(gpu, oracle, SIZES, seed=pair, phases=[15] * 11, diffs=[3] * 11, pairs=[PAIRS[pair]] * 11)
    for side in SIDES:
        run(gpu, a, side, ("pair", pair))
    a.free()


@pytest.mark.parametrize("n_entries", [1, 15, 16, 17, 1023, 1024, 1025])
def test_table_lengths(gpu, oracle, n_entries):
    rng = np.random.default_rng(n_entries)
    a = Arena(gpu, oracle, [int(x) for x in rng.integers(0, 301, size=n_entries)], seed=n_entries)
    run(gpu, a, SIDES[n_entries % 3], ("length", n_entries))
    a.free()


def test_seventy_thousand_entries(gpu, oracle):
    """70 000 entries of 16 .. 80 bytes: the entry index passes 16 bits and the search reaches its fifth level"""
    rng = np.random.default_rng(70000)
    a = Arena(gpu, oracle, [int(x) for x in rng.integers(16, 81, size=70000)], seed=7)
    for side in SIDES:
        run(gpu, a, side, "70 000")
    a.free()


@pytest.mark.parametrize("side", SIDES)
def test_small_grids_flush_at_every_change_of_entry(gpu, oracle, side):
    """Grid forced to 1, 2 and 3 at mixed source phases: runs of one-chunk entries (a flush at every chunk), an 8-chunk entry split
    over the workgroups, empty entries and entries without a body between them -- both ping-pong buffers, both LDS parities and a
    workgroup's third trip.  Then the shipped grid."""
    sizes = [CHUNK] * 5 + [0, 7, 8 * CHUNK - 100, 0, 3] + [CHUNK - 1, CHUNK + 1, 15, 2 * CHUNK, 40000, 0, CHUNK, CHUNK]
    phases = [0] * 5 + [3, 9, 50, 1, 2] + [1, 65535, 0, 0, 30000, 5, 16, 65520]
    diffs = [0, 1, 2, 3, 5, 0, 1, 3, 0, 2, 1, 3, 0, 4, 7, 0, 2, 1]
    a = Arena(gpu, oracle, sizes, seed=3, phases=phases, diffs=diffs)
    with gpu.testing_flavour():
        try:
            for grid in (1, 2, 3):
                gpu.debug_set_rekey_digest_table_grid(grid)
                run(gpu, a, side, ("grid", grid))
                assert gpu.last_launch()["grid"] == grid
        finally:
            gpu.debug_set_rekey_digest_table_grid(0)
        run(gpu, a, side, "shipped grid, testing flavour")
    a.free()


def closed_form(n):
    """Adler-32 of n bytes 0xFF"""
    return ((n + 255 * (n * (n + 1) // 2)) % MOD) << 16 | (1 + 255 * n) % MOD


@pytest.mark.parametrize("n,grid", [(CHUNK, 0), ((32 << 20) + 77, 1)])
def test_widths_on_all_ff(gpu, oracle, n, grid):
    """The summed side is all 0xFF, the destination at phase 16 and the source 5 bytes off it: at 65 536 bytes the per-chunk 32-bit sums
    are at their bounds; at 32 MiB + 77 on ONE workgroup every lane passes 512 chunks and its 64-bit sums pass 2^32.  Input: the source
    is 0xFF fill.  Plain: the source is 0xFF fill cycled under key_from.  Output: the same source, key_to == 0."""
    off = (1 << 32) + 5
    ff = np.full(n, 0xFF, np.uint8)
    cycled = ff.copy()
    oracle.cycle_at(cycled, PS3, off)
    sbuf, dbuf = gpu.DeviceBuffer(n + 3 * CHUNK), gpu.DeviceBuffer(n + 3 * CHUNK)
    d_at = (dbuf.ptr + CHUNK - 1) // CHUNK * CHUNK - dbuf.ptr + CHUNK + 16  # (a chunk in: 64 guard bytes lie in front of it)
    s_at = (sbuf.ptr + CHUNK - 1) // CHUNK * CHUNK - sbuf.ptr + CHUNK + 16 + 5
    t = gpu.rekey_table(1)
    with gpu.testing_flavour():
        try:
            gpu.debug_set_rekey_digest_table_grid(grid)
            for side, src, key_to, off_to in ((gpu.DIGEST_INPUT, ff, PS4, 9), (gpu.DIGEST_PLAIN, cycled, PS4, 9), (gpu.DIGEST_OUTPUT, cycled, 0x7FFFFFFF, 9)):
                sbuf.upload(src, offset=s_at)
                dbuf.upload(np.full(n + 128, 0x11, np.uint8), offset=d_at - 64)
                t[0] = (dbuf.ptr + d_at, sbuf.ptr + s_at, n, off, off_to, gpu.as_int32(PS3), gpu.as_int32(key_to), 0, 0)
                rec, adler = gpu.rekey_digest_table_device(t, None, side)
                assert int(adler[0]) == closed_form(n) and int(rec["n"][0]) == n and int(rec["s1"][0]) % MOD == 255 * n % MOD, side
                want = src.copy()
                oracle.cycle_at(want, PS3, off)
                oracle.cycle_at(want, key_to, off_to)
                got = dbuf.download(n + 128, offset=d_at - 64)
                assert np.array_equal(got[64:64 + n], want) and (got[:64] == 0x11).all() and (got[64 + n:] == 0x11).all(), side
                assert np.array_equal(sbuf.download(n, offset=s_at), src)
        finally:
            gpu.debug_set_rekey_digest_table_grid(0)
    sbuf.free()
    dbuf.free()


@pytest.mark.parametrize("which", ["from", "to"])
def test_threshold_states(gpu, oracle, which):
    """States 1, 2, m - 2 and m - 1 of either keystream placed at chosen bytes of an entry -- the first byte of a word, bytes 1 and 15 of
    a word (the fold), a head byte, a tail byte, the first byte of a second chunk -- through keystream_domain.key_for; the other
    keystream is an ordinary one.  All three sides."""
    # 5 head bytes, a first chunk cut down to one word (lead 65520), a second chunk from byte 21 of the entry, 7 tail bytes
    n, phase = 5 + 16 + CHUNK + 4096 + 7, 65520 - 16 + 11
    positions = [0, 4, 5, 6, 20, 21, 22, 21 + 16 * 300, 21 + 16 * 300 + 15, n - 7, n - 1]
    pairs = []
    for state in K.THRESHOLD_STATES:
        for k, pos in enumerate(positions):
            off = [0, PERIOD - 1, (1 << 32) + 7][k % 3]
            key = K.key_for(state, off + pos, negative=k % 2 == 1)
            assert oracle.state_at(key, off + pos) == state
            key &= 0xFFFFFFFF
            pairs.append((key, PS4, off, 12345) if which == "from" else (PS3, key, 999, off))
    a = Arena(gpu, oracle, [n] * len(pairs), seed=11, phases=[phase] * len(pairs), diffs=[i % 4 for i in range(len(pairs))], pairs=pairs)
    for side in SIDES:
        run(gpu, a, side, ("threshold", which))
    a.free()


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


def test_against_the_existing_calls(gpu, oracle):
    """One resident table through rekey_table_device, then through this call: the destinations match byte for byte.  Output-side
    records are those of digest_table_device over the result under the identity key; plain-side records are those of
    digest_table_device over the sources under key_from at off_from."""
    a = Arena(gpu, oracle, [4097, CHUNK + 3, 0, 17, 2 * CHUNK + 9, 1000, 3 * CHUNK, 15], seed=6)
    t = a.table()
    n = len(t)
    tb, ws = resident(gpu, t)
    res, res_d = Records(gpu, n), Records(gpu, n)
    gpu.rekey_table_device(tb, ws, n=n)
    a.dst.sync()
    first = a.dst.download(a.nbytes, offset=a.d_base)
    d = gpu.table(n)
    d["n"] = t["n"]
    for side, src, key, off in (("output", t["dst"], 0, t["off_to"]), ("plain", t["src"], t["key_from"], t["off_from"])):
        a.reset()
        if side == "output":  # the result of the rekey table call back in place: what the digest table call reads
            a.dst.upload(first, offset=a.d_base)
        d["src"], d["key"], d["stream_off"] = src, key, off
        rec_d, adler_d = gpu.digest_table_device(d, None)
        a.reset()
        res.fill()
        gpu.rekey_digest_table_device(tb, res.ptr, side_of(gpu, side), ws, n=n)
        a.dst.sync()
        assert gpu.table_status(ws) is None
        rec, adler = res.read(side)
        assert np.array_equal(a.dst.download(a.nbytes, offset=a.d_base), first), side
        assert np.array_equal(adler, adler_d) and np.array_equal(rec["s1"] % MOD, rec_d["s1"] % MOD) and np.array_equal(rec["s2"] % MOD, rec_d["s2"] % MOD), side
        assert np.array_equal(rec["n"], rec_d["n"])
        same((rec, adler), a.want[side], side)
    a.check("one call")
    for b in (tb, ws, res, res_d, a):
        b.free()


def node_types(graph):
    """the hipGraphNodeType of every node of a captured graph (0 = kernel, 1 = memcpy, 2 = memset)"""
    n = ctypes.c_size_t(0)
    assert hip().hipGraphGetNodes(graph.graph, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip().hipGraphGetNodes(graph.graph, nodes, ctypes.byref(n)) == 0
    out = []
    for node in nodes:
        kind = ctypes.c_int(-1)
        assert hip().hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) == 0
        out.append(kind.value)
    return out


def test_graph_replay_with_the_check_behind_it(gpu, oracle):
    """One linear capture of the call followed by modgpu_digest_check_device with the table workspace: replayed twice with one entry's
    keys and the source rewritten in between, and once with an entry made bad.  Bytes, records and the check's summary follow, refused
    = 1 included; the graph is five kernel nodes -- no memset node."""
    a = Arena(gpu, oracle, [int(x) for x in np.random.default_rng(8).integers(0, 3 * CHUNK, size=40)], seed=8)
    t = a.table()
    n = len(t)
    tb, ws = resident(gpu, t)
    res = Records(gpu, n)
    expect, summary, bits = gpu.DeviceBuffer(4 * n), gpu.DeviceBuffer(32), gpu.DeviceBuffer(gpu.digest_check_bits_bytes(n))
    st = Stream()
    with Graph.capture(st) as g:
        gpu.rekey_digest_table_device(tb, res.ptr, gpu.DIGEST_PLAIN, ws, n=n, stream=st.handle)
        gpu.digest_check_device(res.ptr, expect, n, ws, summary, bits, stream=st.handle)
    assert node_types(g) == [0] * 5
    for k in range(2):
        if k:
            a.pairs[17] = (PS4, 0x7FFFFFFF, 5, 6)
            a.fill(200 + k)
            tb.upload(a.table().view(np.uint8))
        manifest = np.array([w[0] for w in a.want["plain"]], dtype=np.uint32)
        manifest[23] ^= k << 16  # the second replay: one wrong value in the manifest
        expect.upload(manifest.view(np.uint8))
        g.launch(st)
        st.sync()
        assert gpu.table_status(ws) is None
        a.check(("replay", k))
        same(res.read(("replay", k)), a.want["plain"], ("replay", k))
        bad, first, which = gpu.digest_check_result(summary, n, bits)
        assert (bad, first, [int(x) for x in which]) == ((1, 23, [23]) if k else (0, None, []))
    # an entry made bad: nothing is written, neither bytes nor records, and the check says so on the device
    a.reset()
    res.fill()
    bad_t = a.table()
    bad_t["reserved"][9] = 1
    tb.upload(bad_t.view(np.uint8))
    g.launch(st)
    st.sync()
    assert gpu.table_status(ws) == 9
    a.untouched("refused replay")
    assert (res.raw("refused replay") == 0xA5).all()
    out = np.zeros(1, dtype=gpu.DIGEST_CHECK_SUMMARY_DTYPE)
    assert gpu.lib().modgpu_digest_check_summary(ctypes.c_void_p(summary.ptr), -1, ctypes.c_void_p(out.ctypes.data)) == 1
    assert (int(out["bad_entries"][0]), int(out["entries"][0]), int(out["refused"][0])) == (0, n, 1)
    g.destroy()
    st.destroy()
    for b in (tb, ws, res, expect, summary, bits, a):
        b.free()


def test_two_streams_two_workspaces(gpu, oracle):
    arenas = [Arena(gpu, oracle, [int(x) for x in np.random.default_rng(90 + i).integers(0, 2 * CHUNK, size=60)], seed=90 + i) for i in range(2)]
    streams = [Stream() for _ in arenas]
    rigs = []
    for a in arenas:
        tb, ws = resident(gpu, a.table())
        rigs.append((tb, ws, Records(gpu, 60)))
    for i, ((tb, ws, res), st) in enumerate(zip(rigs, streams)):
        gpu.rekey_digest_table_device(tb, res.ptr, side_of(gpu, SIDES[2 - i]), ws, n=60, stream=st.handle)
    for i, (a, (tb, ws, res), st) in enumerate(zip(arenas, rigs, streams)):
        st.sync()
        assert gpu.table_status(ws) is None
        a.check("two streams")
        same(res.read("two streams"), a.want[SIDES[2 - i]], "two streams")
        for b in (tb, ws, res, a):
            b.free()
        st.destroy()


@pytest.mark.parametrize("what", ["null src", "null dst", "flags", "reserved", "1 TiB"])
def test_device_tier_refusal_writes_nothing(gpu, oracle, what):
    """A bad entry at 700 of 1500 (and a second one above it): no destination byte and no record is written, the status names 700, the
    wrapper raises; the mended table runs clean on the same workspace."""
    rng = np.random.default_rng(15)
    a = Arena(gpu, oracle, [int(x) for x in rng.integers(1, 200, size=1500)], seed=15)
    good = a.table()
    tb, ws = resident(gpu, good)
    res = Records(gpu, 1500)
    at = 700
    t = good.copy()
    for i in (at, at + 300):
        if what == "null src":
            t["src"][i] = 0
        elif what == "null dst":
            t["dst"][i] = 0
        elif what == "flags":
            t["flags"][i] = 1 << (i % 32)
        elif what == "reserved":
            t["reserved"][i] = 7
        else:
            t["n"][i] = (1 << 40) + CHUNK  # (2^24 + 1 chunks or more at any phase)
    tb.upload(t.view(np.uint8))
    before = gpu.path_stats()["gpu_launches"]
    gpu.rekey_digest_table_device(tb, res.ptr, gpu.DIGEST_PLAIN, ws, n=1500)
    a.dst.sync()
    assert gpu.path_stats()["gpu_launches"] - before == 3
    assert gpu.table_status(ws) == at
    assert (res.raw(("refused", at)) == 0xA5).all(), "a refused call wrote records"
    a.untouched(what)
    with pytest.raises(gpu.ModGpuError, match=f"entry {at};"):
        gpu.rekey_digest_table_device(t)
    a.untouched(what)
    tb.upload(good.view(np.uint8))
    gpu.rekey_digest_table_device(tb, res.ptr, gpu.DIGEST_PLAIN, ws, n=1500)
    a.dst.sync()
    assert gpu.table_status(ws) is None
    a.check("mended")
    same(res.read("mended"), a.want["plain"], "mended")
    for b in (tb, ws, res, a):
        b.free()


def test_host_tier_queues_nothing(gpu, oracle):
    a = Arena(gpu, oracle, [100, 200, 300], seed=2)
    tb, ws = resident(gpu, a.table())
    res = Records(gpu, 3)
    host = np.zeros(3 * 4, np.uint64)
    L = gpu.lib()
    wb = gpu.rekey_digest_table_workspace_bytes(3)
    before = gpu.path_stats()["gpu_launches"]
    assert L.modgpu_rekey_digest_table_device(tb.ptr, 3, res.ptr, 3, ws.ptr, wb, -1, None) == 1
    assert "side is neither" in L.modgpu_last_error().decode()
    assert L.modgpu_rekey_digest_table_device(None, 0, None, 3, None, 0, -1, None) == 1
    assert L.modgpu_rekey_digest_table_device(tb.ptr, 3, res.ptr + 4, 0, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_rekey_digest_table_device(tb.ptr, 3, host.ctypes.data, 0, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_rekey_digest_table_device(tb.ptr, 3, None, 2, ws.ptr, wb, -1, None) == 1
    assert "null results" in L.modgpu_last_error().decode()
    assert L.modgpu_rekey_digest_table_device(tb.ptr, 3, res.ptr, 2, ws.ptr, wb - 8, -1, None) == 1
    assert L.modgpu_rekey_digest_table_device(None, 3, res.ptr, 0, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_rekey_digest_table_device(tb.ptr, (1 << 22) + 1, res.ptr, 0, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_rekey_digest_table_device(None, 0, None, 0, None, 0, -1, None) == 0
    assert gpu.path_stats()["gpu_launches"] == before
    assert (res.raw("tier 1") == 0xA5).all()
    a.untouched("tier 1")
    rec, adler = gpu.rekey_digest_table_device(gpu.rekey_table(0))
    assert rec.size == 0 and adler.size == 0
    for b in (tb, ws, res):
        b.free()
    run(gpu, a, "plain", "after the refusals")
    a.free()


def test_reporting(gpu, oracle):
    a = Arena(gpu, oracle, [3 * CHUNK + 5, 17], seed=4)
    run(gpu, a, "plain", "reporting")
    info = gpu.last_launch()
    assert info["variant"] == 20 and info["bytes"] == 0 and info["kernel"] == "modgpu_cycle_rekey_table_kernel<4, 1024>", info
    assert info["grid"] >= 1 and info["block"] == 1024 and info["chunk_bytes"] == CHUNK and info["source_hash"] == gpu.rekey_table_kernel_source_hash(), info
    a.reset()
    gpu.rekey_table_device(a.table())
    assert gpu.last_launch()["variant"] == 9
    a.check("the plain call")
    a.reset()
    tb, ws = resident(gpu, a.table())
    res = Records(gpu, 2)
    assert gpu.time_rekey_digest_table_device(tb, 2, res.ptr, ws, gpu.DIGEST_INPUT, iters=1) > 0
    same(res.read("timed"), a.want["input"], "timed")
    a.check("timed")
    for b in (tb, ws, res, a):
        b.free()


def test_device_buffer_convert(gpu, oracle):
    n = 5 * CHUNK + 100
    img = np.random.default_rng(55).integers(0, 256, size=n, dtype=np.uint8)
    d, out = gpu.DeviceBuffer(n), gpu.DeviceBuffer(n)
    d.upload(img)
    out.upload(np.full(n, 0x33, np.uint8))
    ranges = [(0, 100), (100, CHUNK), (CHUNK + 107, 0), (CHUNK + 777, 3 * CHUNK + 1), (n - 15, 15)]
    part_off = (1 << 33) + 5
    image, plain, stored = np.full(n, 0x33, np.uint8), [], []
    for o, m in ranges:
        seg = img[o:o + m].copy()
        if m:
            oracle.cycle_at(seg, PS3, part_off + o)
        plain.append(zlib.adler32(seg.tobytes()) & 0xFFFFFFFF)
        if m:
            oracle.cycle_at(seg, PS4, part_off + o)
        stored.append(zlib.adler32(seg.tobytes()) & 0xFFFFFFFF)
        image[o:o + m] = seg
    assert [int(g) for g in d.convert(ranges, PS3, PS4, out, part_off)] == plain
    assert np.array_equal(out.download(), image) and np.array_equal(d.download(), img)
    assert [int(g) for g in d.convert(ranges, PS3, PS4, out, part_off, side=gpu.DIGEST_OUTPUT)] == stored
    got, (bad, first, which) = d.convert_checked(ranges, PS3, PS4, out, np.array(plain, dtype=np.uint32), part_off)
    assert [int(g) for g in got] == plain and (bad, first, list(which)) == (0, None, [])
    wrong = np.array(plain, dtype=np.uint32)
    wrong[3] ^= 1
    got, (bad, first, which) = d.convert_checked(ranges, PS3, PS4, out, wrong, part_off)
    assert [int(g) for g in got] == plain and (bad, first, [int(x) for x in which]) == (1, 3, [3])
    # in place: each range converted where it lies, the rest of the part as it was
    assert [int(g) for g in d.convert(ranges, PS3, PS4, d, part_off)] == plain
    inplace = img.copy()
    for o, m in ranges:
        inplace[o:o + m] = image[o:o + m]
    assert np.array_equal(d.download(), inplace) and d.convert([], PS3, PS4, out).size == 0
    d.free()
    out.free()
