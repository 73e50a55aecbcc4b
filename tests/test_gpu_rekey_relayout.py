"""GPU: modgpu_rekey_relayout_table_device -- a table of rekey entries whose segments slide BOTH ways, moved with memmove rules in one
pass of ten launches -- against the CPU oracle.

The arena, the guards, the key pairs and the model are tests/test_gpu_rekey_move_table.py's: want = img.copy(), then for each entry
want[dst:dst+n] = img[src:src+n] ^ ks_from ^ ks_to, and the WHOLE window is compared, guards and untouched source bytes included.
After every accepted case the status is (None, None) and the call has made ten launches.  The tests run in the testing flavour with
the move launches' grid forced to 4, so that workgroups draw many tickets and wait across entries.  Every case stays inside the 7 MiB
arena.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte compared here came from a kernel."""
import numpy as np
import pytest

from hip_rt import Graph, Stream
from test_gpu_rekey_move_table import BASE, BIG, CAP, CHUNK, G, KEY_PAIRS, PS3, PS4, SPAN, Arena, planned_chunks

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 17, 4101, 65535, 65537, 131073]
SHIFTS = [1, 17, 4099, 65541, 7, 65536]
GAPS = [0, 1, 3, 16]
PATTERNS = ["DU", "UD", "DSU", "UDUD", "DDUUDD"]  # D slides down, U up, S stays: one letter per entry


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
    p = oracle.splitmix_bytes(CAP, 41)
    p.setflags(write=False)
    return p


def pattern(runs, start, turn, sizes=None):
    """[(dst, src, n, pair)] counted from the arena's base: the sources laid from `start` upward with small gaps, each entry's shift
    taken from SHIFTS with the sign of its letter; where the destination would fall into the one before it the source moves up, so
    sources and destinations both stay rising and disjoint.  Sizes, shifts, gaps and key pairs rotate from `turn`."""
    segs, src, dst_end = [], start, 0
    for i, way in enumerate(runs):
        n = sizes[i] if sizes else SIZES[(i + turn) % len(SIZES)]
        shift = 0 if way == "S" else (1 if way == "U" else -1) * SHIFTS[(i + 2 * turn) % len(SHIFTS)]
        src += GAPS[(i + turn) % len(GAPS)]
        if i and src + shift < dst_end:
            src = dst_end - shift
        segs.append((src + shift, src, n, KEY_PAIRS[(i + turn) % len(KEY_PAIRS)]))
        dst_end = src + shift + n
        src += n
    return segs


def alternating(count, each, start):
    """`count` entries of `each` bytes, sliding alternately by +7 and -7"""
    return [(start + i * (each + 16) + (-7 if i % 2 else 7), start + i * (each + 16), each, KEY_PAIRS[i % len(KEY_PAIRS)]) for i in range(count)]


class RelayoutArena(Arena):
    """the move table tests' arena, its table run through the relayout call; an accepted case makes ten launches"""

    def run(self, t, total=None, stream=None):
        self.table.upload(t.view(np.uint8))
        total = int(t["n"].sum()) if total is None else total
        self.M.rekey_relayout_table_device(self.table, total, self.ws, n=t.size, stream=stream)

    def case(self, segs, payload, streams, what):
        before = self.M.path_stats()["gpu_launches"]
        super().case(segs, payload, streams, what)
        assert self.M.path_stats()["gpu_launches"] - before == 10, what
        info = self.M.last_launch()
        assert info["variant"] == 15 and info["source_hash"] == self.M.rekey_move_table_kernel_source_hash(), info


@pytest.fixture()
def arena(gpu):
    with gpu.testing_flavour():
        gpu.debug_set_move_table_grid(4)
        a = RelayoutArena(gpu)
        try:
            yield a
        finally:
            gpu.debug_set_move_table_grid(0)
            a.free()


@pytest.mark.parametrize("ph", (0, 1, 7))
def test_run_patterns_at_a_grid_of_4(arena, streams, payload, ph):
    """every run pattern, sizes, shifts (from 1 byte to above a chunk) and the six key pairs in rotation, three destination phases"""
    for runs in PATTERNS:
        for turn in range(len(SIZES)):
            arena.case(pattern(runs, 2 * CHUNK + 12345 * turn + ph, turn), payload, streams, (runs, turn))


def test_a_40_chunk_entry_in_each_direction(gpu, arena, streams, payload):
    arena.case(pattern("DUDU", 2 * CHUNK + 7, 0, [BIG, 65537, 17, BIG]), payload, streams, "big")
    # the shipped grid (one workgroup per CU): the same table, every workgroup on its first tickets
    gpu.debug_set_move_table_grid(0)
    arena.case(pattern("DUDU", 2 * CHUNK + 7, 0, [BIG, 65537, 17, BIG]), payload, streams, "big, shipped grid")
    info = gpu.last_launch()
    assert info["bytes"] == 0 and 4 < info["grid"] <= 256 and info["block"] == 1024 and "modgpu_cycle_rekey_move_table_kernel" in info["kernel"], info


def test_small_entries_alternating(arena, streams, payload):
    for ph in (0, 1, 7):
        arena.case(alternating(64, 9, CHUNK + ph), payload, streams, ("64 x 9", ph))
        arena.case(alternating(64, 1000, CHUNK + ph), payload, streams, ("64 x 1000", ph))
    arena.case(alternating(300, 100, CHUNK - 3000), payload, streams, "300 x 100 across a chunk boundary")


def test_empty_entries_between_the_runs(arena, streams, payload):
    for runs in PATTERNS:
        segs, holes = pattern(runs, 2 * CHUNK + 9, 2), [(CAP, 0, 0, KEY_PAIRS[0])]
        for i, seg in enumerate(segs):
            if i and runs[i] != runs[i - 1]:
                holes.append((0, CAP, 0, KEY_PAIRS[0]) if i % 2 else (5, 5, 0, KEY_PAIRS[0]))
            holes.append(seg)
        arena.case(holes + [(5, 7, 0, KEY_PAIRS[0])], payload, streams, runs)


@pytest.mark.parametrize("runs", ("DDDSD", "UUSUU"), ids=("down", "up"))
def test_one_way_tables_give_what_the_move_table_call_gives(gpu, arena, streams, payload, runs):
    segs = pattern(runs, 2 * CHUNK + 7, 3, [65537, 3 * CHUNK + 5, 17, 131073, 4101])
    lo, img = arena.window(segs, payload)
    t = arena.entries(segs)
    arena.buf.upload(img, offset=arena.at + lo - G)
    Arena.run(arena, t)
    arena.buf.sync()
    assert gpu.rekey_move_table_status(arena.ws) == (None, None)
    want = arena.buf.download(img.size, offset=arena.at + lo - G)
    assert np.array_equal(want, arena.model(segs, lo, img, streams))
    arena.buf.upload(img, offset=arena.at + lo - G)
    before = gpu.path_stats()["gpu_launches"]
    arena.run(t)
    arena.buf.sync()
    assert gpu.path_stats()["gpu_launches"] - before == 10 and gpu.rekey_move_table_status(arena.ws) == (None, None)
    assert np.array_equal(arena.buf.download(img.size, offset=arena.at + lo - G), want)


@pytest.mark.parametrize("key,key_to", ((PS4, PS4), (PS3, PS4)), ids=("same-key", "ps3->ps4"))
def test_splice_of_a_resident_part(gpu, oracle, key, key_to):
    """a 1 MiB + 77 part under `key` at part offset 9: edits that grow, shrink, delete, insert and replace -- the surviving segments
    stay, slide up and slide down --, DeviceBuffer.splice, the holes uploaded with the cipher in flight: the whole part then is the
    oracle's encryption of the spliced plaintext under key_to"""
    n, part_off = (1 << 20) + 77, 9
    plain = oracle.splitmix_bytes(n, 42)
    fresh = oracle.splitmix_bytes(1 << 19, 43)
    edits = [(1000, 500, 70000), (200000, 65537 + 70000, 17), (400000, 4101, 0), (450000, 0, 131073), (700001, 3 * CHUNK, 3 * CHUNK), (n - 15, 15, 1)]
    pieces, holes_want, at, used, new_at, ways = [], [], 0, 0, 0, set()
    for off, old, new in edits:
        ways.add(np.sign(new_at - at) if off > at else None)
        pieces += [plain[at:off], fresh[used:used + new]]
        new_at += off - at
        if new:
            holes_want.append((new_at, new))
        at, used, new_at = off + old, used + new, new_at + new
    assert {-1, 0, 1} <= ways, "the case has segments that stay, slide down and slide up"
    spliced = np.concatenate(pieces + [plain[at:]])
    want = spliced.copy()
    oracle.cycle_at(want, key_to, part_off)
    enc = plain.copy()
    oracle.cycle_at(enc, key, part_off)
    with gpu.testing_flavour():
        gpu.debug_set_move_table_grid(4)
        part = gpu.DeviceBuffer(n + (1 << 18))
        try:
            part.upload(np.full(part.nbytes, 0xA5, np.uint8))
            part.upload(enc)
            with pytest.raises(ValueError):
                part.splice([(0, 0, 1 << 19)], key, n, part_off)
            new_used, holes = part.splice(edits, key, n, part_off, key_to=None if key_to == key else key_to)
            assert new_used == spliced.size and holes == holes_want
            part.sync()
            used = 0
            for off, new in holes:
                gpu.cycle_host_to_device(part.ptr + off, fresh[used:used + new], key_to, part_off + off)
                used += new
            got = part.download()
            assert np.array_equal(got[:new_used], want)
            assert (got[max(n, new_used):] == 0xA5).all(), "bytes behind the part were written"
        finally:
            gpu.debug_set_move_table_grid(0)
            part.free()


def test_refusals_on_the_device_leave_the_arena_untouched(gpu, arena, payload):
    """each fault makes the whole call write nothing, in either sweep, and the status names the lowest bad entry"""
    good = pattern("DUDUD", 2 * CHUNK + 7, 0, [65537, 131073, 17, 2 * CHUNK + 5, 70000])
    lo, img = arena.window(good, payload)
    t0 = arena.entries(good)
    total = int(t0["n"].sum())
    gpu.rekey_relayout_table_validate(t0)

    def runs_into(t):  # entry 1 slides up, entry 2 down
        t[1]["dst"] = int(t[2]["dst"]) - int(t[1]["n"]) + 1

    def falling(t):
        t[[1, 2]] = t[[2, 1]]

    def flags_filtered_by_sweep_0(t):
        t[1]["flags"] = 1
        t[4]["reserved"] = 9

    def flags_filtered_by_sweep_1(t):
        t[2]["flags"] = 1

    def null_source(t):
        t[3]["src"] = 0

    def huge(t):
        t[4]["n"] = 1 << 41

    for what, change, bad in (("an upward entry's destination runs into the next, downward, entry's", runs_into, 2),
                              ("falling order across a direction change", falling, 2),
                              ("nonzero flags on an entry sweep 0 filters", flags_filtered_by_sweep_0, 1),
                              ("nonzero flags on an entry sweep 1 filters", flags_filtered_by_sweep_1, 2),
                              ("a null source", null_source, 3), ("an entry of 1 TiB or more", huge, 4)):
        t = t0.copy()
        change(t)
        with pytest.raises(gpu.ModGpuError, match=f"entry {bad}:"):
            gpu.rekey_relayout_table_validate(t)
        arena.buf.upload(img, offset=arena.at + lo - G)
        arena.run(t, total=total)
        arena.buf.sync()
        assert gpu.rekey_move_table_status(arena.ws) == (bad, None), what
        assert gpu.table_status(arena.ws) == bad, what
        assert np.array_equal(arena.buf.download(img.size, offset=arena.at + lo - G), img), what
    # total_bytes large enough for each sweep alone, too small for the table: 45 chunks' worth sizes the workspace for 45 + 2 per entry,
    # each 40-chunk entry lies on 41 or 42, and the status names the first entry whose chunks, counted over ALL entries, pass that
    for runs in ("DU", "UD"):
        small = pattern(runs, 2 * CHUNK + 7, 0, [BIG, BIG])
        slo, simg = arena.window(small, payload)
        t = arena.entries(small)
        gpu.rekey_relayout_table_validate(t)
        chunks = [planned_chunks(int(d), int(n)) for d, n in zip(t["dst"], t["n"])]
        room = 45 + 2 * t.size
        assert max(chunks) <= room < sum(chunks)
        arena.buf.upload(simg, offset=arena.at + slo - G)
        arena.run(t, total=45 * CHUNK)
        arena.buf.sync()
        assert gpu.rekey_move_table_status(arena.ws) == (1, None) and gpu.table_status(arena.ws) == 1, runs
        assert np.array_equal(arena.buf.download(simg.size, offset=arena.at + slo - G), simg), runs
    # ... and the call after a refused one on the same workspace runs clean
    arena.buf.upload(img, offset=arena.at + lo - G)
    arena.run(t0)
    arena.buf.sync()
    assert gpu.rekey_move_table_status(arena.ws) == (None, None)


def test_captured_call_replayed_with_the_table_rewritten(gpu, arena, streams, payload):
    """one captured call -- a single chain of ten kernel nodes --, replayed three times: mixed, another mixed, pure down, the table
    rewritten and the payload uploaded again in between.  The table is read when the call runs, by both sweeps."""
    st = Stream()
    try:
        sizes = [2 * CHUNK + 33, 65537, 17, 3 * CHUNK + 1, 70000]
        arena.table.upload(arena.entries(pattern("DDDDD", 2 * CHUNK, 0, sizes)).view(np.uint8))
        with Graph.capture(st) as g:
            gpu.rekey_relayout_table_device(arena.table, sum(sizes), arena.ws, n=5, stream=st.handle)
        for k, runs in enumerate(("DUDUD", "UUSDD", "DDDDD")):
            segs = pattern(runs, 2 * CHUNK + 12345 + k, k + 1, sizes)
            lo, img = arena.window(segs, payload)
            arena.buf.upload(img, offset=arena.at + lo - G)
            arena.table.upload(arena.entries(segs).view(np.uint8))
            g.launch(st)
            st.sync()
            assert gpu.rekey_move_table_status(arena.ws) == (None, None)
            assert np.array_equal(arena.buf.download(img.size, offset=arena.at + lo - G), arena.model(segs, lo, img, streams)), ("replay", k, runs)
        g.destroy()
    finally:
        st.destroy()
