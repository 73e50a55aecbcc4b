"""GPU: modgpu_rekey_move_table_device -- a table of rekey entries moved with memmove rules, a destination on top of any entry's source,
in one pass -- against the CPU oracle.

The model is the oracle applied to a host copy: want = img.copy(), then for each entry want[dst:dst+n] = img[src:src+n] ^ ks_from ^
ks_to, the keystreams computed ONCE per key from one 64-bit base offset and sliced.  Every case runs in one arena on a 64 KiB-aligned
base whose payload is surrounded by 0xA5 guard bands, and the WHOLE window is compared, guards and untouched source bytes included.
After every case the status is OK.  The tests run in the testing flavour with the move launch's grid forced to 4, so that workgroups
draw many tickets and wait across entries.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte compared
here came from a kernel."""
import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
CHUNK = 65536
G = 256                                   # guard bytes on either side of the payload
BIG = 40 * CHUNK + 77
SIZES = [1, 15, 17, 65535, 65537, 131073, BIG]
GAPS = [1, 3, 16, 17, 4096, 65535, 65536, 65537, 3 * CHUNK + 5]
BASE = (1 << 32) + 12345                  # where the precomputed keystreams start: 64-bit offsets, a phase of its own
CAP = 7 << 20                             # bytes of arena a case may span, counted from its base
SPAN = CAP + (1 << 20)                    # bytes of keystream kept per key
# (name, key_from, key_to, off_from - BASE - src, off_to - BASE - src or None = the compaction pair: off_to follows the destination)
KEY_PAIRS = [("ps3->ps4", PS3, PS4, 3, 22), ("compaction", PS4, PS4, 1000, None), ("plain", PS3, PS3, 77, 77),
             ("from-identity", 0, PS4, 5, 9), ("to-identity", PS3, 0x7FFFFFFF, 5, 9), ("both-identity", 0, 0x80000001, 1, 2)]
MAX_ENTRIES = 512


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


@pytest.fixture(scope="module")
def streams(oracle):
    """the keystream bytes of both keys from BASE on, once for every test of the module (read-only); a zero key's are zero"""
    ks = {}
    for key in (PS3, PS4):
        z = np.zeros(SPAN, np.uint8)
        oracle.cycle_at(z, key, BASE)
        z.setflags(write=False)
        ks[key] = z
    zero = np.zeros(SPAN, np.uint8)
    zero.setflags(write=False)
    return lambda key: ks.get(key, zero)


@pytest.fixture(scope="module")
def payload(oracle):
    p = oracle.splitmix_bytes(CAP, 35)
    p.setflags(write=False)
    return p


def layout(sizes, gaps, down, start, pairs):
    """[(dst, src, n, pair)] counted from the arena's base: `down` packs the segments from `start` with their sources the gaps further
    up each (closing the gaps), else the sources are packed and the gaps opened"""
    segs, packed, spread = [], start, start
    for i, (n, g) in enumerate(zip(sizes, gaps)):
        spread += g
        segs.append((packed, spread, n, pairs[i % len(pairs)]) if down else (spread, packed, n, pairs[i % len(pairs)]))
        packed += n
        spread += n
    return segs


class Arena:
    """Device memory whose offset 0 (self.base) lies on a 64 KiB boundary with room below for the guard; a table and a workspace."""

    def __init__(self, M, cap=CAP, entries=MAX_ENTRIES):
        self.M = M
        self.buf = M.DeviceBuffer(cap + 3 * CHUNK)
        self.at = (-self.buf.ptr) % CHUNK + CHUNK  # offset of `base` inside the buffer
        self.base = self.buf.ptr + self.at
        self.table = M.DeviceBuffer(entries * 56)
        self.ws = M.DeviceBuffer(M.rekey_move_table_workspace_bytes(entries, cap))

    def entries(self, segs):
        t = self.M.rekey_table(len(segs))
        for i, (dst, src, n, (_, kf, kt, of, ot)) in enumerate(segs):
            t[i]["dst"], t[i]["src"], t[i]["n"] = self.base + dst, self.base + src, n
            t[i]["off_from"], t[i]["off_to"] = BASE + of + src, BASE + (of + dst if ot is None else ot + src)
            t[i]["key_from"], t[i]["key_to"] = self.M.as_int32(kf), self.M.as_int32(kt)
        return t

    def window(self, segs, payload):
        """(lo, img): the bytes [lo - G, hi + G) of the arena, the payload inside 0xA5 guards"""
        lo = min(min(d, s) for d, s, n, _ in segs if n)
        hi = max(max(d, s) + n for d, s, n, _ in segs if n)
        img = np.full(2 * G + hi - lo, 0xA5, np.uint8)
        img[G:G + hi - lo] = payload[:hi - lo]
        return lo, img

    @staticmethod
    def model(segs, lo, img, streams):
        want = img.copy()
        for dst, src, n, (_, kf, kt, of, ot) in segs:
            o_to = of + dst if ot is None else ot + src
            want[G + dst - lo:G + dst - lo + n] = img[G + src - lo:G + src - lo + n] ^ streams(kf)[of + src:of + src + n] ^ streams(kt)[o_to:o_to + n]
        return want

    def run(self, t, total=None, stream=None):
        self.table.upload(t.view(np.uint8))
        total = int(t["n"].sum()) if total is None else total
        self.M.rekey_move_table_device(self.table, total, self.ws, n=t.size, stream=stream)

    def case(self, segs, payload, streams, what):
        lo, img = self.window(segs, payload)
        self.buf.upload(img, offset=self.at + lo - G)
        want = self.model(segs, lo, img, streams)
        self.run(self.entries(segs))
        self.buf.sync()
        assert self.M.rekey_move_table_status(self.ws) == (None, None), what
        assert self.M.table_status(self.ws) is None, what
        got = self.buf.download(img.size, offset=self.at + lo - G)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError((what, [(d, s, n, p[0]) for d, s, n, p in segs],
                                  "first/last/count of differing bytes (window offsets; the payload starts at G)", int(bad[0]), int(bad[-1]), bad.size))

    def free(self):
        for b in (self.buf, self.table, self.ws):
            b.free()


@pytest.fixture()
def arena(gpu):
    with gpu.testing_flavour():
        gpu.debug_set_move_table_grid(4)
        a = Arena(gpu)
        try:
            yield a
        finally:
            gpu.debug_set_move_table_grid(0)
            a.free()


@pytest.mark.parametrize("ph", (0, 1, 7))
@pytest.mark.parametrize("down", (True, False), ids=("down", "up"))
def test_matrix_at_a_grid_of_4(arena, streams, payload, down, ph):
    """tables of 5 segments, sizes and gaps taken in rotation from the lists (every size and every gap is met in each direction and
    phase; the 40-chunk segment at most once per table), every key pair and one table that mixes all six, one per entry"""
    for k, pairs in enumerate([[p] for p in KEY_PAIRS] + [KEY_PAIRS]):
        for draw in range(3):
            sizes = [SIZES[(5 * draw + i + k) % len(SIZES)] for i in range(5)]
            gaps = [GAPS[(5 * draw + i + 2 * k) % len(GAPS)] for i in range(5)]
            arena.case(layout(sizes, gaps, down, 12345 * draw + ph, pairs), payload, streams, (k, draw))


@pytest.mark.parametrize("down", (True, False), ids=("down", "up"))
def test_waits_across_entries(gpu, arena, streams, payload, down):
    rng = np.random.default_rng(15)
    # gaps below a chunk: the first destination chunk of entry i+1 covers the last source chunk of entry i
    arena.case(layout([3 * CHUNK + 5, 2 * CHUNK + 100, 3 * CHUNK, 65537, 2 * CHUNK + 1], [100, 17, 4096, 1, 65535], down, 1, KEY_PAIRS[1:2]), payload, streams,
               "gaps below a chunk")
    # 300 entries of 1 to 100 bytes with 1-byte gaps and one entry of 5 chunks + 9 whose chunks meet the sources of many of them (it
    # comes last in the downward table, first in the upward one: its destinations lie over the small entries' sources either way)
    sizes = [int(x) for x in rng.integers(1, 101, 300)] + [5 * CHUNK + 9]
    for pairs in (KEY_PAIRS[:1], KEY_PAIRS):
        arena.case(layout(sizes if down else sizes[::-1], [1] * 301, down, 3, pairs), payload, streams, "300 small entries")
    # dst == src in the middle of a table, and empty entries with pointers of any kind anywhere
    C = CHUNK
    mid = [(C, C + 500, 70000), (C + 70000, C + 80000, 65537), (4 * C + 9, 4 * C + 9, 2 * C + 3), (6 * C + 12, 6 * C + 4096, 131073), (9 * C, 9 * C + 100, 17)]
    if not down:
        mid = [(C + 500, C, 70000), (3 * C, 2 * C + 60000, 65537), (4 * C + 9, 4 * C + 9, 2 * C + 3), (6 * C + 4096, 6 * C + 12, 131073), (9 * C + 100, 9 * C, 17)]
    segs = [(d, s, n, KEY_PAIRS[i]) for i, (d, s, n) in enumerate(mid)]
    arena.case(segs, payload, streams, "an entry in the middle stays")
    arena.case([(CAP, 0, 0, KEY_PAIRS[0])] + segs[:2] + [(0, CAP, 0, KEY_PAIRS[0])] + segs[2:] + [(5, 5, 0, KEY_PAIRS[0])], payload, streams, "empty entries")
    # the shipped grid (one workgroup per CU): the same table, every workgroup on its first tickets
    gpu.debug_set_move_table_grid(0)
    arena.case(layout([BIG, 131073, 17, 65537, 15], [65537, 3, 4096, 17, 65536], down, 7, KEY_PAIRS), payload, streams, "shipped grid")
    info = gpu.last_launch()
    assert info["variant"] == 15 and info["bytes"] == 0 and 4 < info["grid"] <= 256 and info["block"] == 1024, info
    assert info["source_hash"] == gpu.rekey_move_table_kernel_source_hash() and "modgpu_cycle_rekey_move_table_kernel" in info["kernel"], info


@pytest.mark.parametrize("n", SIZES)
def test_one_entry_is_the_single_move_call(gpu, arena, payload, n):
    """one entry of each size gives byte for byte what modgpu_rekey_move_device gives on the same arena, every key pair, both
    directions; the from-identity pair takes ONE pass here (five launches, whatever the keys)"""
    single_ws = gpu.DeviceBuffer(gpu.move_workspace_bytes(n))
    try:
        for d in (1, 17, 65537):
            for down in (True, False):
                for pair in KEY_PAIRS:
                    segs = layout([n], [d], down, 12345 + 7, [pair])
                    lo, img = arena.window(segs, payload)
                    t = arena.entries(segs)
                    arena.buf.upload(img, offset=arena.at + lo - G)
                    gpu.rekey_move_device(int(t[0]["dst"]), int(t[0]["src"]), n, pair[1], pair[2], int(t[0]["off_from"]), int(t[0]["off_to"]), single_ws)
                    arena.buf.sync()
                    assert gpu.move_status(single_ws) is None
                    want = arena.buf.download(img.size, offset=arena.at + lo - G)
                    arena.buf.upload(img, offset=arena.at + lo - G)
                    before = gpu.path_stats()["gpu_launches"]
                    arena.run(t)
                    arena.buf.sync()
                    assert gpu.path_stats()["gpu_launches"] - before == 5, pair[0]
                    assert gpu.last_launch()["variant"] == 15 and gpu.last_launch()["grid"] == 4
                    assert gpu.rekey_move_table_status(arena.ws) == (None, None)
                    assert np.array_equal(arena.buf.download(img.size, offset=arena.at + lo - G), want), (n, d, down, pair[0])
    finally:
        single_ws.free()


def test_captured_call_replayed_with_the_table_rewritten(gpu, arena, streams, payload):
    """one captured call, replayed twice: the table's gaps and keys rewritten and the payload uploaded again in between -- the table is
    read when the call runs, and the first launch resets the workspace"""
    st = Stream()
    try:
        sizes = [2 * CHUNK + 33, 65537, 17, 3 * CHUNK + 1, 70000]
        arena.table.upload(arena.entries(layout(sizes, [1] * 5, True, 0, KEY_PAIRS[:1])).view(np.uint8))
        with Graph.capture(st) as g:
            gpu.rekey_move_table_device(arena.table, sum(sizes), arena.ws, n=5, stream=st.handle)
        for k, (gaps, pairs, down) in enumerate((([65537, 3, 4096, 17, 100], KEY_PAIRS[:1], True), ([5, 65536, 1, 3 * CHUNK + 5, 16], KEY_PAIRS[1:], False))):
            segs = layout(sizes, gaps, down, 12345 + k, pairs)
            lo, img = arena.window(segs, payload)
            arena.buf.upload(img, offset=arena.at + lo - G)
            arena.table.upload(arena.entries(segs).view(np.uint8))
            g.launch(st)
            st.sync()
            assert gpu.rekey_move_table_status(arena.ws) == (None, None)
            assert np.array_equal(arena.buf.download(img.size, offset=arena.at + lo - G), arena.model(segs, lo, img, streams)), ("replay", k)
        g.destroy()
    finally:
        st.destroy()


def test_refusals_on_the_device_leave_the_arena_untouched(gpu, arena, payload):
    """each fault makes the whole call write nothing, and the status names the lowest bad entry (modgpu_table_status too)"""
    good = layout([65537, 131073, 17, 2 * CHUNK + 5, 70000], [4096, 17, 1, 65537, 3], True, 7, KEY_PAIRS[:1])
    lo, img = arena.window(good, payload)
    t0 = arena.entries(good)
    total = int(t0["n"].sum())

    def upward(t):
        t[3]["dst"], t[3]["src"] = t[3]["src"], t[3]["dst"]

    def falling(t):
        t[[1, 2]] = t[[2, 1]]

    def dst_overlap(t):
        t[2]["dst"] = int(t[1]["dst"]) + int(t[1]["n"]) - 1

    def src_overlap(t):
        t[4]["src"] = int(t[3]["src"]) + int(t[3]["n"]) - 1

    def flags(t):
        t[1]["flags"] = 1
        t[4]["reserved"] = 9

    for what, change, bad, tb in (("an upward entry in a downward table", upward, 3, total), ("two entries listed in falling order", falling, 2, total),
                                  ("overlapping destinations", dst_overlap, 2, total), ("overlapping sources", src_overlap, 4, total),
                                  ("nonzero flags", flags, 1, total)):
        t = t0.copy()
        change(t)
        with pytest.raises(gpu.ModGpuError, match=f"entry {bad}:"):
            gpu.rekey_move_table_validate(t)
        arena.buf.upload(img, offset=arena.at + lo - G)
        arena.run(t, total=tb)
        arena.buf.sync()
        assert gpu.rekey_move_table_status(arena.ws) == (bad, None), what
        assert gpu.table_status(arena.ws) == bad, what
        assert np.array_equal(arena.buf.download(img.size, offset=arena.at + lo - G), img), what
    # total_bytes too small for the table: 0 sizes the workspace for 2 chunks per entry, 10 in all, and the third entry alone has 41.
    # The status names the first entry whose chunks pass that.
    small = layout([17, 65537, BIG, 17, 15], [4096, 17, 1, 65537, 3], True, 7, KEY_PAIRS[:1])
    slo, simg = arena.window(small, payload)
    t = arena.entries(small)
    gpu.rekey_move_table_validate(t)
    sums = np.cumsum([planned_chunks(int(d), int(n)) for d, n in zip(t["dst"], t["n"])])
    assert sums[-1] > 10 and int(np.argmax(sums > 10)) == 2
    arena.buf.upload(simg, offset=arena.at + slo - G)
    arena.run(t, total=0)
    arena.buf.sync()
    assert gpu.rekey_move_table_status(arena.ws) == (2, None) and gpu.table_status(arena.ws) == 2
    assert np.array_equal(arena.buf.download(simg.size, offset=arena.at + slo - G), simg)
    # ... and the call after a refused one on the same workspace runs clean
    arena.buf.upload(img, offset=arena.at + lo - G)
    arena.run(t0)
    arena.buf.sync()
    assert gpu.rekey_move_table_status(arena.ws) == (None, None)


def planned_chunks(dst, n):
    """the 64 KiB chunks of the destination an entry's body (its 16-byte words) lies on"""
    head = min(n, -dst % 16)
    words = (n - head) // 16
    return -(-((dst + head) % CHUNK + 16 * words) // CHUNK) if words else 0


def test_compaction_of_a_resident_part(gpu, oracle):
    """a 3 MiB + 77 part under the PS4 key from offset 0, 7 ranges kept: DeviceBuffer.compact packs them, and the result decrypts to
    the concatenation of the kept plaintext"""
    n = (3 << 20) + 77
    plain = oracle.splitmix_bytes(n, 36)
    enc = plain.copy()
    oracle.cycle_at(enc, PS4, 0)
    keep = [(0, 100001), (100001 + 5, 65536), (200000, 1), (200017, 15), (300000, 17 * CHUNK + 3), (n - 700000, 65537), (n - 77, 77)]
    t = gpu.compaction_table(1 << 20, keep, PS4, part_off=9)
    assert [int(x) for x in t["src"]] == [(1 << 20) + o for o, _ in keep] and int(t[1]["dst"]) == (1 << 20) + 100001
    assert int(t[1]["off_from"]) == 9 + 100006 and int(t[1]["off_to"]) == 9 + 100001 and int(t[6]["key_from"]) == int(t[6]["key_to"]) == gpu.as_int32(PS4)
    gpu.rekey_move_table_validate(t)
    part = gpu.DeviceBuffer(n)
    try:
        part.upload(enc)
        new_n = part.compact(keep, PS4)
        assert new_n == sum(k for _, k in keep)
        got = part.download()
        assert np.array_equal(got[new_n:], enc[new_n:]), "bytes behind the packed ranges were written"
        packed = got[:new_n].copy()
        oracle.cycle_at(packed, PS4, 0)
        assert np.array_equal(packed, np.concatenate([plain[o:o + k] for o, k in keep]))
    finally:
        part.free()
