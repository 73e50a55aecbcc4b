"""GPU: the list transfers (modgpu_cycle_host_to_device_list, modgpu_cycle_device_to_host_list) against the CPU oracle.

Every case lays its entries out in one device buffer and two host arrays with guard bytes around EVERY entry and checks all
destination bytes and all guard bytes (the whole arena is compared), that every source is unchanged, how many launches the call was
(ONE, unless the case lowers the one-launch limit), and that last_launch() reports the list variant, a funnel kernel and the transfer
TU's source hash.  The reference is oracle.cycle_at or a call pinned elsewhere (modgpu_cycle_device), never a list call.

The first seven cases stay below ~2 MiB of packed stream: at the chunk the library reports for such calls (read from its host trace,
not assumed) that is at least 12 chunks on several pipelines, and every slot holds ONE chunk.  The cases behind them are there for
what that size cannot reach, and each ASSERTS on its inputs that it reaches it:
  * every staging slot filled at least three times (chunks forced to 32 and 64 KiB in the testing flavour; 256 KiB chunks of the
    shipped library under the 32 MiB list);
  * entries above 8 MiB and one above 2 GiB: the second and the third jump table of the list branch read at an index other than 0;
  * the cut into windows on the device (the one-launch limit lowered in the testing flavour): one plan allocation rewritten between
    real launches, first and last record clipped, a window that begins and ends inside one entry;
  * a plan of more than 65 535 records;
  * two list calls at once on one device's staging sets.
Cases that need a tunable take the testing flavour (the gpu_t fixture below) and put the tunable back in a `finally`.
conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte compared here came from a kernel.  No case injects a
failure or holds the kernel up: tests/xfer_list_main.cpp does that on the CPU stand-in, where it also runs the lists of the cases
below but the 2 GiB one."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = [0x90CFC0AB, 0xC64EED30, 1, 0xFFFFFFFF, 0x80000000, 12345, 0x7FFFFFFF, 0]  # (the last two: the identity keystream)
PERIOD = 0x7FFFFFFE
OFFSETS = [0, 5, (1 << 32) + 5, PERIOD - 100, (1 << 63) + 11, (1 << 64) - 3, 3 * PERIOD - 7]  # past 2^32; crossing the period inside an entry
PIECE = 32768
GUARD = 24
DEV_FILL, HOST_FILL = 0xD5, 0x3C


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


@pytest.fixture()
def gpu_t(gpu):
    """The same bindings routed to libmodgpu_testing.so for one test (the flavour that carries modgpu_debug_set_host_tunable); every
    test that does not ask for this fixture runs on the shipped library.  The two tunables the cases here touch go back to what the
    library ships with, whatever happened."""
    with gpu.testing_flavour():
        assert gpu.testing_hooks() and gpu.gpu_required() and gpu.device_count() >= 1
        try:
            yield gpu
        finally:
            gpu.debug_set_host_tunable("feed_chunk_bytes", 256 << 10)
            gpu.debug_set_host_tunable("xfer_list_most_bytes", 0)
    assert gpu.active_flavour() == "shipped"


def phases_and_sizes():
    """(n, key, stream_off, device phase, host phase) per entry: ten sizes five times over, the device phase walking 0..15, the host
    phase against it by a different amount each time, the packed phase following from the odd sizes"""
    sizes = [1, 15, 16, 17, 4095, 32767, 32768, 32769, 65536 + 17, 3 * 65536 + 77]
    specs, k = [], 0
    for rep in range(5):
        for n in sizes:
            specs.append((n, KEYS[k % 8], OFFSETS[k % 7], k % 16, (k * 7 + rep * 3) % 16))
            k += 1
    return specs


def boundaries(chunk):
    specs, state = [], {"packed": 0, "k": 0}

    def add(n):
        k = state["k"]
        specs.append((n, KEYS[k % 6], OFFSETS[k % 7], (k * 5) % 16, (k * 3 + 1) % 16))
        state["packed"] += n
        state["k"] += 1

    def end_at(p):  # an entry that ends exactly at packed position p
        add(p - state["packed"])

    for p in (PIECE - 1, PIECE, 2 * PIECE, 3 * PIECE + 1):  # boundaries one before, on, on and one behind a piece boundary
        end_at(p)
    c1 = (state["packed"] // chunk + 1) * chunk
    for p in (c1 - 1, c1, c1 + chunk, c1 + 2 * chunk + 1):  # the same around chunk boundaries
        end_at(p)
    add(3 * chunk + 4097)  # one entry that spans more than three chunks
    p0 = (state["packed"] // PIECE + 1) * PIECE
    end_at(p0 - 15000)  # then 10 000 entries of 1..7 bytes (40 000 bytes): the run crosses the piece boundary p0 and the next one
    for i in range(10000):
        specs.append((1 + i % 7, KEYS[i % 6], (OFFSETS[i % 7] + i) % (1 << 64), i % 16, (i * 11) % 16))  # (a 64-bit offset)
    state["packed"] += sum(1 + i % 7 for i in range(10000))
    assert (p0 - 15000) // PIECE < (p0 + 25000) // PIECE
    add(777)
    return specs


NUL = (0, 0x90CFC0AB, 0, 0, 0, True)  # an empty entry with NULL pointers
EMPTY = (0, 0xC64EED30, 9, 3, 5)  # an empty entry with pointers


def with_empties():
    return [NUL, EMPTY, NUL, (70000, 0x90CFC0AB, 17, 1, 2), NUL, NUL, EMPTY, (5, 0xC64EED30, (1 << 40) + 3, 15, 0), NUL,
            (PIECE + 3, 1, 0, 7, 9), EMPTY, NUL]


# ---- the lists of the cases behind the first seven (tests/xfer_list_main.cpp builds the same ones for the CPU stand-in) ---------------
PIPES_MOST = 8  # the pipelines a call can have (MODGPU_HOST_PIPES' default), two slots each
SLOT_ROUNDS = 3


def refilled(specs, chunk):
    """`specs` behind as many copies of phases_and_sizes() as it takes for ceil(total / chunk) >= 3 x 2 x 8, so that every slot of every
    pipeline is filled at least three times.  The copies are padded to a whole number of chunks: every packed position of `specs` keeps
    its place in its piece and its chunk, and lies in a slot that has been used before."""
    need = SLOT_ROUNDS * 2 * PIPES_MOST * chunk
    own = sum(s[0] for s in specs)
    head = []
    while own + sum(s[0] for s in head) < need:
        head += phases_and_sizes()
    pad = -sum(s[0] for s in head) % chunk
    if pad:
        head.append((pad, KEYS[1], OFFSETS[2], 9, 4))
    return head + specs


LONG_2, LONG_4 = (8 << 20) + 3 * PIECE + 77, (16 << 20) + PIECE + 1


def long_entries():
    """~32 MiB, entries above 8 and above 16 MiB: the list branch's second jump table at the indices 1 and 2"""
    return [(13, KEYS[1], 5, 3, 7), (LONG_2, KEYS[0], (1 << 64) - 3, 5, 11), (4097, KEYS[2], (1 << 32) + 5, 0, 9),
            (LONG_4, KEYS[1], PERIOD - 100, 12, 1), ((8 << 20) + 5, 0x7FFFFFFF, 3, 7, 14)]


def seventy_thousand():
    """70 000 entries of 1..7 bytes, one of 40 000 bytes in the middle, empty and NULL entries scattered in"""
    specs = []
    for i in range(70000):
        if i == 35000:
            specs.append((40000, KEYS[1], OFFSETS[2], 5, 11))
        if i % 9973 == 17:
            specs.append(NUL if (i // 9973) % 2 else EMPTY)
        specs.append((1 + i % 7, KEYS[i % 6], (OFFSETS[i % 7] + i) % (1 << 64), i % 16, (i * 11) % 16))
    return specs


def most_steps(specs, most=0):
    """per non-empty entry, the largest `steps` -- whole 32 KiB steps from a record's first byte to a segment's -- that the kernel computes
    for it: pieces are cut from each window's first byte, a window's first record begins where the window does, and a segment begins at
    a record's first byte or on a piece boundary; `steps` takes every value from 0 up to the one returned"""
    out, es = [], 0
    total = sum(s[0] for s in specs)
    for s in specs:
        n = s[0]
        if not n:
            continue
        top, at = 0, es - es % most if most else 0
        while at < es + n:
            first, end = max(es, at), min(es + n, at + most if most else total)
            last_piece = at + (end - 1 - at) // PIECE * PIECE  # the last piece boundary of the window that lies in front of the record's end
            if last_piece > first:
                top = max(top, (last_piece - first) // PIECE)
            if not most:
                break
            at += most
        out.append(top)
        es += n
    return out

class Layout:
    """A case laid out: entry e's device side at dev + d_at[e], its plaintext at src[h_at[e]:], its download at back[h_at[e]:]"""

    def __init__(self, M, oracle, specs, seed=1):
        self.M, self.specs = M, [s if len(s) == 6 else s + (False,) for s in specs]
        d = h = 64
        self.d_at, self.h_at = [], []
        for n, _, _, dp, hp, _ in self.specs:
            d = (d + GUARD + 15) // 16 * 16 + dp
            h = (h + GUARD + 15) // 16 * 16 + hp
            self.d_at.append(d)
            self.h_at.append(h)
            d, h = d + n, h + n
        self.d_size, self.h_size = d + 64, h + 64
        self.total = sum(s[0] for s in self.specs)
        self.dev = M.DeviceBuffer(self.d_size)
        self.dev.upload(np.full(self.d_size, DEV_FILL, np.uint8))
        self.src = oracle.splitmix_bytes(self.h_size, seed)
        self.back = np.full(self.h_size, HOST_FILL, np.uint8)
        self.want_dev = np.full(self.d_size, DEV_FILL, np.uint8)
        self.want_back = np.full(self.h_size, HOST_FILL, np.uint8)
        for (n, key, so, _, _, _), da, ha in zip(self.specs, self.d_at, self.h_at):
            if n:
                w = self.src[ha:ha + n].copy()
                self.want_dev[da:da + n] = w if key % 0x7FFFFFFF == 0 else oracle.cycle_at(w, key, so % PERIOD)
                self.want_back[ha:ha + n] = self.src[ha:ha + n]

    def table(self, upload):
        t = self.M.table(len(self.specs))
        host = self.src if upload else self.back
        for i, ((n, key, so, _, _, nul), da, ha) in enumerate(zip(self.specs, self.d_at, self.h_at)):
            d, h = (0, 0) if nul else (self.dev.ptr + da, host.ctypes.data + ha)
            t[i]["dst"], t[i]["src"] = (d, h) if upload else (h, d)
            t[i]["n"], t[i]["stream_off"], t[i]["key"] = n, so, self.M.as_int32(key)
        return t

    def reset(self):
        """both destinations back to their fill, so that a second round trip over the same layout proves itself"""
        self.dev.upload(np.full(self.d_size, DEV_FILL, np.uint8))
        self.back[:] = HOST_FILL

    def free(self):
        self.dev.free()


def windows(total, most):
    """the launches of a list call of `total` packed bytes under a one-launch limit of `most` (0: the library's own, far above any case
    here): how many, and the bytes of the last"""
    k = -(-total // most) if most else 1
    return k, total - (k - 1) * most if most else total


def one_list_launch(M, before, upload, total, most=0):
    """the call was ONE launch (ceil(total / most) under a lowered limit) and the last launch is the list variant over the last window"""
    st = M.path_stats()
    k, last = windows(total, most)
    assert st["gpu_launches"] - before == (k if total else 0), (st["gpu_launches"] - before, k)
    if total:
        ll = M.last_launch()
        name = "modgpu_cycle_xfer_kernel<%s, true>" % ("true" if upload else "false")
        assert ll["variant"] == 21 and ll["kernel"] == name and ll["source_hash"] == M.xfer_kernel_source_hash() and ll["bytes"] == last, ll


def round_trip(M, L, most=0, counted=True, gate=None):
    """up, then down: the round trip to plaintext, every byte of the three arenas.  `most`: the one-launch limit the caller has set.
    counted=False leaves the launch counters alone (they are the process's: another thread is at work).  `gate`, if given, is called
    in front of each of the two list calls with the list built, and returns what is called behind it."""
    src_keep = L.src.copy()
    t = L.table(True)
    before = M.path_stats()["gpu_launches"]
    after = gate() if gate else None
    M.cycle_host_to_device_list(t)
    if after:
        after()
    if counted:
        one_list_launch(M, before, True, L.total, most)
    got = L.dev.download()
    bad = np.flatnonzero(got != L.want_dev)
    assert bad.size == 0, ("upload", bad.size, bad[:8].tolist())
    assert np.array_equal(L.src, src_keep), "the upload changed a source"
    t = L.table(False)
    before = M.path_stats()["gpu_launches"]
    after = gate() if gate else None
    M.cycle_device_to_host_list(t)
    if after:
        after()
    if counted:
        one_list_launch(M, before, False, L.total, most)
    bad = np.flatnonzero(L.back != L.want_back)
    assert bad.size == 0, ("download", bad.size, bad[:8].tolist())
    assert np.array_equal(L.dev.download(), L.want_dev), "the download changed a source"


@pytest.fixture(scope="module")
def chunk(gpu, oracle):
    """the chunk of a list call of the cases' size, as the library's host trace reports it"""
    M = gpu
    L = Layout(M, oracle, phases_and_sizes())
    M.host_trace(True)
    M.cycle_host_to_device_list(L.table(True))
    M.host_trace(False)
    slots = [e for e in M.host_trace_read() if e["kind"] == "slots"]
    L.free()
    assert len(slots) == 1 and slots[0]["bytes"] % PIECE == 0, slots
    assert L.total <= 2 << 20 and L.total // slots[0]["bytes"] >= 12 and slots[0]["chunk"] > 1, (L.total, slots)  # >= 12 chunks, several pipelines
    return slots[0]["bytes"]


def test_phases_and_sizes(gpu, oracle, chunk):
    L = Layout(gpu, oracle, phases_and_sizes())
    met = {}
    for (_, _, _, dp, hp, _), ha in zip(L.specs, L.h_at):
        met.setdefault(dp, set()).add(hp)
    assert sorted(met) == list(range(16)) and all(len(v) >= 3 for v in met.values()), met
    round_trip(gpu, L)
    L.free()


def test_boundaries(gpu, oracle, chunk):
    L = Layout(gpu, oracle, boundaries(chunk))
    assert L.total <= 2 << 20
    starts = np.cumsum([0] + [s[0] for s in L.specs])
    for unit in (PIECE, chunk):  # packed entry boundaries on a multiple of the unit and one byte to either side of one
        r = set(int(s) % unit for s in starts[1:-1])
        assert {0, 1, unit - 1} <= r, (unit, sorted(r)[:5])
    assert max(s[0] for s in L.specs) > 3 * chunk
    round_trip(gpu, L)
    L.free()


def test_empty_entries(gpu, oracle):
    M = gpu
    L = Layout(M, oracle, with_empties())
    round_trip(M, L)
    L.free()
    L = Layout(M, oracle, [NUL, EMPTY, NUL])  # only such entries: nothing is launched
    round_trip(M, L)
    before = M.path_stats()["gpu_launches"]
    M.cycle_host_to_device_list(M.table(0))
    M.cycle_device_to_host_list([])
    assert M.path_stats()["gpu_launches"] == before
    L.free()


def test_same_bytes_as_the_loop(gpu, oracle):
    M = gpu
    A, B = Layout(M, oracle, phases_and_sizes(), seed=7), Layout(M, oracle, phases_and_sizes(), seed=7)
    M.cycle_host_to_device_list(A.table(True))
    for e in B.table(True):
        if e["n"]:
            ha = int(e["src"]) - B.src.ctypes.data
            M.cycle_host_to_device(int(e["dst"]), B.src[ha:ha + int(e["n"])], int(e["key"]), int(e["stream_off"]))
    a = A.dev.download()
    assert np.array_equal(a, B.dev.download()) and np.array_equal(a, A.want_dev)
    M.cycle_device_to_host_list(A.table(False))
    for e in B.table(False):
        if e["n"]:
            ha = int(e["dst"]) - B.back.ctypes.data
            M.cycle_device_to_host(B.back[ha:ha + int(e["n"])], int(e["src"]), int(e["key"]), int(e["stream_off"]))
    assert np.array_equal(A.back, B.back) and np.array_equal(A.back, A.want_back)
    A.free()
    B.free()


def test_shared_sources(gpu, oracle):
    M = gpu
    n = 2 * PIECE + 301
    L = Layout(M, oracle, [(n, 0x90CFC0AB, 3, 1, 5), (n, 0xC64EED30, 1 << 33, 9, 5), (n, 0, 0, 14, 5)])
    src_keep = L.src.copy()
    up = L.table(True)
    up["src"][1:] = up["src"][0]  # one host range to three destinations under three keys
    for (_, key, so, _, _, _), da in zip(L.specs, L.d_at):
        w = L.src[L.h_at[0]:L.h_at[0] + n].copy()
        L.want_dev[da:da + n] = w if key % 0x7FFFFFFF == 0 else oracle.cycle_at(w, key, so)
    before = M.path_stats()["gpu_launches"]
    M.cycle_host_to_device_list(up)
    one_list_launch(M, before, True, 3 * n)
    assert np.array_equal(L.dev.download(), L.want_dev) and np.array_equal(L.src, src_keep)
    dn = L.table(False)[:2].copy()  # one device range to two host destinations
    dn["src"][1], dn["key"][1], dn["stream_off"][1] = dn["src"][0], dn["key"][0], dn["stream_off"][0]
    want = np.full(L.h_size, HOST_FILL, np.uint8)
    for ha in L.h_at[:2]:
        want[ha:ha + n] = L.src[L.h_at[0]:L.h_at[0] + n]
    before = M.path_stats()["gpu_launches"]
    M.cycle_device_to_host_list(dn)
    one_list_launch(M, before, False, 2 * n)
    assert np.array_equal(L.back, want) and np.array_equal(L.dev.download(), L.want_dev)
    L.free()


def test_refusals_on_a_live_device(gpu, oracle):
    M = gpu
    L = Layout(M, oracle, [(1000, 0x90CFC0AB, 0, 1, 2), (2000, 0xC64EED30, 5, 3, 4), NUL, (3000, 1, 7, 5, 6), (4000, 0x90CFC0AB, 9, 7, 8)])
    src_keep, before = L.src.copy(), M.path_stats()["gpu_launches"]
    for upload in (True, False):
        call = M.cycle_host_to_device_list if upload else M.cycle_device_to_host_list
        side = "dst" if upload else "src"
        t = L.table(upload)
        t[side][3] = L.back.ctypes.data + 64  # a host pointer as the device side of a middle entry
        with pytest.raises(M.ModGpuError) as e:
            call(t)
        assert e.value.code == 1 and str(e.value).find("entry 3:") >= 0 and "not device memory" in str(e.value), str(e.value)
        t = L.table(upload)
        t["n"][4] = L.d_size  # a device range that runs off the end of its allocation
        if not upload:
            big = np.empty(L.d_size, np.uint8)
            t["dst"][4] = big.ctypes.data
        with pytest.raises(M.ModGpuError) as e:
            call(t)
        assert e.value.code == 1 and str(e.value).find("entry 4:") >= 0 and "not device memory" in str(e.value), str(e.value)
    assert M.path_stats()["gpu_launches"] == before
    assert np.all(L.dev.download() == DEV_FILL) and np.all(L.back == HOST_FILL) and np.array_equal(L.src, src_keep)
    round_trip(M, L)  # ... and the same buffers take a good list afterwards
    L.free()


def test_splice_and_fill(gpu, oracle):
    M = gpu
    key, part_off = 0xC64EED30, (1 << 32) - 1000
    used, cap = 300000, 400000
    old = oracle.splitmix_bytes(used, 21)
    edits = [(100, 50, 0), (5000, 0, 33), (70001, 4096, 65536 + 5), (150000, 17, 17), (299000, 1000, 3000)]
    buf = M.DeviceBuffer(cap)
    buf.upload(np.zeros(cap, np.uint8))
    buf.upload_ranges([(0, old)], key, part_off)
    new_used, holes = buf.splice(edits, key, used, part_off)
    buf.sync()
    fills = [oracle.splitmix_bytes(n, 30 + i) for i, (_, n) in enumerate(holes)]
    before = M.path_stats()["gpu_launches"]
    buf.fill(holes, fills, key, part_off)
    one_list_launch(M, before, True, sum(n for _, n in holes))
    # the part as the host would have built it: the survivors and the fills end to end, then the cipher from part_off
    parts, at, it = [], 0, iter(fills)
    for off, old_len, new_len in edits:
        parts.append(old[at:off])
        if new_len:
            parts.append(next(it))
        at = off + old_len
    parts.append(old[at:])
    plain = np.concatenate(parts)
    assert plain.size == new_used
    assert np.array_equal(buf.download(new_used), oracle.cycle_at(plain.copy(), key, part_off))
    # ... and ranges of it come back as plaintext, in one call
    ranges = [(0, 100), (5000, 33), (70001 - 50 + 33, 65536 + 5), (new_used - 3000, 3000), (17, 0)]
    outs = buf.download_ranges(ranges, key, [np.full(n, HOST_FILL, np.uint8) for _, n in ranges], part_off)
    for (o, n), got in zip(ranges, outs):
        assert np.array_equal(got, plain[o:o + n]), (o, n)
    buf.free()


# ---- past one round of the slots, 8 MiB, 65 535 records, one launch, one caller and 2 GiB -------------------------------------------
def traced_round_trip(M, L, most=0):
    """round_trip with the host trace on: the (pipelines, chunk bytes) of every window's `slots` event and the bytes of every launch"""
    M.host_trace(True)
    try:
        round_trip(M, L, most)
    finally:
        M.host_trace(False)
    ev = M.host_trace_read()
    return [(e["chunk"], e["bytes"]) for e in ev if e["kind"] == "slots"], [e["bytes"] for e in ev if e["kind"] == "launched"]


@pytest.mark.parametrize("knob, want_chunk", [(32 << 10, 32 << 10), (64 << 10, 32 << 10), (128 << 10, 64 << 10)])
def test_every_slot_is_refilled(gpu_t, oracle, knob, want_chunk):
    """Chunks of one piece and of two (a call of 8 MiB or less takes chunks of HALF feed_chunk_bytes, at least a piece: 32 and 64 KiB
    both give one piece, 128 KiB gives two), the lists long enough for three rounds of every slot: fill_slot gathers into, drain_slot
    scatters out of and the funnel kernels read and write slots that have held another chunk of the same call."""
    M = gpu_t
    M.debug_set_host_tunable("feed_chunk_bytes", knob)
    for specs in (refilled(phases_and_sizes(), want_chunk), refilled(boundaries(want_chunk), want_chunk)):
        L = Layout(M, oracle, specs)
        slots, launched = traced_round_trip(M, L)
        assert len(slots) == 2 and launched == [L.total] * 2, (slots, launched)
        for pipes, got_chunk in slots:
            assert got_chunk == want_chunk and L.total <= 8 << 20, (got_chunk, L.total)
            assert -(-L.total // got_chunk) >= SLOT_ROUNDS * 2 * pipes and pipes > 1, (L.total, got_chunk, pipes)
        L.free()


def test_entries_longer_than_8_mib(gpu, oracle):
    """The shipped library, nothing forced: the segments of an entry above 8 MiB take c_chunk_pow1 at index 1 while c_chunk_pow0's index
    wraps, those of an entry above 16 MiB index 2; ~32 MiB in 256 KiB chunks is eight rounds of every slot."""
    M = gpu
    L = Layout(M, oracle, long_entries())
    steps = most_steps(L.specs)
    assert steps[1] >> 8 == 1 and steps[1] & 255 < 255 and steps[3] >> 8 == 2, steps
    starts = np.cumsum([0] + [s[0] for s in L.specs])
    assert all(int(s) % PIECE for s in starts[1:-1])  # no long entry begins on a piece boundary
    slots, launched = traced_round_trip(M, L)
    assert launched == [L.total] * 2 and len(slots) == 2, (slots, launched)
    for pipes, got_chunk in slots:
        assert -(-L.total // got_chunk) >= SLOT_ROUNDS * 2 * pipes and pipes > 1, (L.total, got_chunk, pipes)
    L.free()


def windowed(M, L, most):
    """the limit at `most`: ceil(total / most) launches each way, every window but the last of `most` bytes; then the limit back and one
    launch again"""
    k, last = windows(L.total, most)
    assert k > 1
    M.debug_set_host_tunable("xfer_list_most_bytes", most)
    slots, launched = traced_round_trip(M, L, most)
    assert launched == ([most] * (k - 1) + [last]) * 2 and len(slots) == 2 * k, (k, launched)
    M.debug_set_host_tunable("xfer_list_most_bytes", 0)
    L.reset()
    slots, launched = traced_round_trip(M, L)
    assert launched == [L.total] * 2 and len(slots) == 2, launched


@pytest.mark.parametrize("most", [300000, 3 * PIECE])
def test_windows(gpu_t, oracle, chunk, most):
    """The one-launch limit lowered: a launch per window, the one plan allocation rewritten between them, first and last record clipped
    (a clipped record's base is the host's state at off + into).  300 000 is no multiple of a piece; at 3 pieces every window edge is a
    piece edge."""
    M = gpu_t
    for specs in (phases_and_sizes(), boundaries(chunk)):
        L = Layout(M, oracle, specs)
        windowed(M, L, most)
        L.free()


def test_windows_inside_long_entries(gpu_t, oracle):
    """The 32 MiB list in windows of 5 MiB + 12345: windows that begin AND end inside one entry, then the whole list in one launch.  Such a
    window is too short for the second jump table (the one launch behind it has it), so the list goes once more in windows of
    12 MiB + 4099: the 16 MiB entry's second record is clipped and its segments go on to index 1 of that table from the HOST's base."""
    M = gpu_t
    most = (5 << 20) + 12345
    L = Layout(M, oracle, long_entries())
    starts = np.cumsum([0] + [s[0] for s in L.specs])
    inside = [w for w in range(0, L.total - most, most) if any(a < w and w + most < b for a, b in zip(starts[:-1], starts[1:]))]
    assert inside, "no window lies inside one entry"
    assert max(most_steps(L.specs, most)) < 256 <= max(most_steps(L.specs))
    windowed(M, L, most)
    most = (12 << 20) + 4099
    assert starts[3] < most < 2 * most < starts[4] and most_steps(L.specs, most)[3] >> 8 == 1  # (the window from `most` on lies inside entry 3)
    L.reset()
    windowed(M, L, most)
    L.free()


def test_seventy_thousand_entries(gpu, oracle):
    M = gpu
    L = Layout(M, oracle, seventy_thousand())
    records = sum(1 for s in L.specs if s[0])
    assert records > 65535 and len(L.specs) > records and max(s[0] for s in L.specs) == 40000, (records, len(L.specs))
    assert sum(1 for s in L.specs if s[5]) >= 3 and sum(1 for s in L.specs if not s[0] and not s[5]) >= 3
    round_trip(M, L)
    L.free()


def test_two_calls_at_once(gpu, oracle):
    """Two threads, three round trips each on layouts of their own: the device's staging sets, slot leases and flag words are shared.
    The threads meet at a barrier in front of every list call, so that the calls do run side by side (their times say whether they did)."""
    M = gpu
    before = M.path_stats()["gpu_launches"]
    errors, spans = [], {100: [], 200: []}
    barrier = threading.Barrier(2)

    def work(seed):
        def gate():
            barrier.wait(60)
            t0 = time.perf_counter()
            return lambda: spans[seed].append((t0, time.perf_counter()))

        try:
            for k in range(3):
                L = Layout(M, oracle, with_empties() if k == 1 else phases_and_sizes(), seed=seed + k)
                round_trip(M, L, counted=False, gate=gate)
                L.free()
        except BaseException as e:  # (an assertion in a thread is the test's)
            errors.append((seed, repr(e)))
            barrier.abort()  # (the other thread does not wait for this one)

    threads = [threading.Thread(target=work, args=(seed,)) for seed in spans]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)  # (the library's own limits are far below this: a call that does not return fails the test, it does not hang it)
    assert not any(t.is_alive() for t in threads), "a list call did not return"
    assert not errors, errors
    assert M.path_stats()["gpu_launches"] - before == 2 * 3 * 2
    side_by_side = sum(1 for (a0, a1), (b0, b1) in zip(spans[100], spans[200]) if a0 < b1 and b0 < a1)
    assert len(spans[100]) == len(spans[200]) == 6 and side_by_side >= 1, (side_by_side, spans)


def test_one_entry_beyond_2_gib(gpu, oracle):
    """One entry of 2 GiB + 3 pieces + 77 between two small ones: the smallest shape at which the list branch reads c_chunk_pow2 at an
    index other than 0.  Judged like test_gpu_xfer.py::test_4gib_pageable_upload_equals_the_device_cipher: windows of the upload against
    the oracle, the whole entry undone in place by modgpu_cycle_device against the source, then up again and down through the list."""
    M = gpu
    key, so = 0x90CFC0AB, (1 << 32) - 1000
    big = (1 << 31) + 3 * PIECE + 77
    specs = [(13, KEYS[1], 5, 3, 7), (big, key, so, 5, 11), (4097, KEYS[2], PERIOD - 100, 9, 2)]
    assert most_steps(specs)[1] >> 16 >= 1
    d = h = 64
    d_at, h_at = [], []
    for n, _, _, dp, hp in specs:  # (Layout's rule)
        d, h = (d + GUARD + 15) // 16 * 16 + dp, (h + GUARD + 15) // 16 * 16 + hp
        d_at.append(d)
        h_at.append(h)
        d, h = d + n, h + n
    d_size, h_size, total = d + 64, h + 64, sum(s[0] for s in specs)
    block = oracle.splitmix_bytes(64 << 20, 4)
    src = np.tile(block, -(-h_size // block.size))[:h_size]
    flip = h_at[1] + 12345
    src[flip] ^= 0xFF  # (not periodic at the block size)

    def src_intact():
        for o in range(0, h_size, block.size):
            m = min(block.size, h_size - o)
            if o <= flip < o + m:
                f = flip - o
                assert src[flip] == block[f] ^ 0xFF and np.array_equal(src[o:flip], block[:f]) and np.array_equal(src[flip + 1:o + m], block[f + 1:m])
            else:
                assert np.array_equal(src[o:o + m], block[:m]), o

    dev = M.DeviceBuffer(d_size)
    head_n, tail_at = d_at[1], d_at[1] + big  # the device arena around the long entry: both small entries and every guard byte
    want_head, want_tail = np.full(head_n, DEV_FILL, np.uint8), np.full(d_size - tail_at, DEV_FILL, np.uint8)
    dev.upload(want_head)
    dev.upload(want_tail, offset=tail_at)
    for e, want, base in ((0, want_head, 0), (2, want_tail, tail_at)):
        n, k, o = specs[e][:3]
        want[d_at[e] - base:d_at[e] - base + n] = oracle.cycle_at(src[h_at[e]:h_at[e] + n].copy(), k, o % PERIOD)

    def around_intact():
        assert np.array_equal(dev.download(head_n), want_head) and np.array_equal(dev.download(d_size - tail_at, offset=tail_at), want_tail)

    def table(upload, host):
        t = M.table(3)
        for i, ((n, k, o, _, _), da, ha) in enumerate(zip(specs, d_at, h_at)):
            t[i]["dst"], t[i]["src"] = (dev.ptr + da, host.ctypes.data + ha) if upload else (host.ctypes.data + ha, dev.ptr + da)
            t[i]["n"], t[i]["stream_off"], t[i]["key"] = n, o, M.as_int32(k)
        return t

    before = M.path_stats()["gpu_launches"]
    M.cycle_host_to_device_list(table(True, src))
    one_list_launch(M, before, True, total)
    around_intact()
    mib = 1 << 20
    for o, m in ((0, mib), ((1 << 31) - mib // 2, big - (1 << 31) + mib // 2), (big - mib, mib)):  # the head, across entry index 2^31, the tail
        want = oracle.cycle_at(src[h_at[1] + o:h_at[1] + o + m].copy(), key, (so + o) % PERIOD)
        bad = np.flatnonzero(dev.download(m, offset=d_at[1] + o) != want)
        assert bad.size == 0, ("upload", o, bad.size, bad[:8].tolist())
    M.cycle_device(dev.ptr + d_at[1], big, key, so)
    dev.sync()
    step = 256 << 20
    for o in range(0, big, step):
        m = min(step, big - o)
        assert np.array_equal(dev.download(m, offset=d_at[1] + o), src[h_at[1] + o:h_at[1] + o + m]), o
    around_intact()
    src_intact()
    # up again, and back through the list: the whole host array, guards included
    before = M.path_stats()["gpu_launches"]
    M.cycle_host_to_device_list(table(True, src))
    one_list_launch(M, before, True, total)
    back = np.full(h_size, HOST_FILL, np.uint8)
    before = M.path_stats()["gpu_launches"]
    M.cycle_device_to_host_list(table(False, back))
    one_list_launch(M, before, False, total)
    at = 0
    for (n, _, _, _, _), ha in zip(specs, h_at):
        assert np.all(back[at:ha] == HOST_FILL), ("a guard in front of the entry at", ha)
        for o in range(0, n, step):
            m = min(step, n - o)
            assert np.array_equal(back[ha + o:ha + o + m], src[ha + o:ha + o + m]), ("download", ha, o)
        at = ha + n
    assert np.all(back[at:] == HOST_FILL)
    around_intact()
    src_intact()
    dev.free()
