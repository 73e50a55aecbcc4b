"""GPU: the list transfers (modgpu_cycle_host_to_device_list, modgpu_cycle_device_to_host_list) against the CPU oracle.

Every case lays its entries out in one device buffer and two host arrays with guard bytes around EVERY entry and checks all
destination bytes and all guard bytes (the whole arena is compared), that every source is unchanged, that the call was ONE launch,
and that last_launch() reports the list variant, a funnel kernel and the transfer TU's source hash.  Totals stay below ~2 MiB: at the
chunk the library reports for such calls (read from its host trace, not assumed) that is at least 12 chunks on several pipelines.
conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte compared here came from a kernel.  No case injects a
failure or holds the kernel up: tests/xfer_list_main.cpp does that on the CPU stand-in."""
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

    def free(self):
        self.dev.free()


def one_list_launch(M, before, upload, total):
    st = M.path_stats()
    assert st["gpu_launches"] - before == (1 if total else 0), st["gpu_launches"] - before
    if total:
        ll = M.last_launch()
        name = "modgpu_cycle_xfer_kernel<%s, true>" % ("true" if upload else "false")
        assert ll["variant"] == 21 and ll["kernel"] == name and ll["source_hash"] == M.xfer_kernel_source_hash() and ll["bytes"] == total, ll


def round_trip(M, L):
    """up, then down: the round trip to plaintext, every byte of the three arenas"""
    src_keep = L.src.copy()
    t = L.table(True)
    before = M.path_stats()["gpu_launches"]
    M.cycle_host_to_device_list(t)
    one_list_launch(M, before, True, L.total)
    got = L.dev.download()
    bad = np.flatnonzero(got != L.want_dev)
    assert bad.size == 0, ("upload", bad.size, bad[:8].tolist())
    assert np.array_equal(L.src, src_keep), "the upload changed a source"
    t = L.table(False)
    before = M.path_stats()["gpu_launches"]
    M.cycle_device_to_host_list(t)
    one_list_launch(M, before, False, L.total)
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
    empty = (0, 0xC64EED30, 9, 3, 5)
    L = Layout(M, oracle, [NUL, empty, NUL, (70000, 0x90CFC0AB, 17, 1, 2), NUL, NUL, empty, (5, 0xC64EED30, (1 << 40) + 3, 15, 0), NUL,
                           (PIECE + 3, 1, 0, 7, 9), empty, NUL])
    round_trip(M, L)
    L.free()
    L = Layout(M, oracle, [NUL, empty, NUL])  # only such entries: nothing is launched
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
