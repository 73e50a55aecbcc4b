"""GPU: the table call (modgpu_cycle_table_device: a device-resident table of out-of-place entries, three launches) against the CPU
oracle.  Every case lays its entries' destinations disjointly in one arena pre-filled with a guard pattern and checks the WHOLE arena --
each entry's bytes equal cycle_at(src, key, stream_off), every byte outside the entries unchanged -- and that the sources did not
change.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte compared here came from a kernel."""
import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
KEYS = [PS4, PS3, 1, 0xFFFFFFFF, 0x80000000, 12345, 0x7FFFFFFF, 0, 0x80000001, 0xDEADBEEF]  # incl. INT_MIN, -1, identity keys
CHUNK = 65536
SIZES = [0, 1, 5, 15, 16, 17, 4095, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


class Arena:
    """n_entries entries: destinations disjoint (with gaps) at random phases in one arena, sources anywhere in a source buffer of
    random bytes (they may overlap each other), keys from KEYS, offsets up to 2^64-1."""

    def __init__(self, M, oracle, n_entries, seed, sizes=SIZES, small=False, phases=None):
        rng = np.random.default_rng(seed)
        if small:  # many entries: mostly small, some around a chunk
            sz = rng.integers(0, 4096, size=n_entries)
            pick = rng.random(n_entries) < 0.02
            sz[pick] = rng.integers(CHUNK - 16, 2 * CHUNK + 16, size=int(pick.sum()))
        else:
            sz = np.array([sizes[i % len(sizes)] for i in range(n_entries)], dtype=np.int64)
        self.sizes = sz.astype(np.uint64)
        self.src_n = int(max(4 * CHUNK, sz.max() + 64, int(sz.sum()) // 2 + 64))
        gaps = rng.integers(1, 48, size=n_entries)
        cur, dst_off = 64, []
        for i, s in enumerate(sz):
            if phases is not None:  # (destination phase, source phase) of entry i
                cur = ((cur + 15) & ~15) + phases[i][0]
            dst_off.append(cur)
            cur += int(s) + int(gaps[i])
        self.dst_off = np.array(dst_off, dtype=np.uint64)
        self.dst_n = cur + 64
        if phases is not None:
            self.src_off = np.array([16 * (i % 64) + phases[i][1] for i in range(n_entries)], dtype=np.uint64)
        else:
            self.src_off = np.array([int(rng.integers(0, self.src_n - s + 1)) for s in sz], dtype=np.uint64)
        self.keys = np.array([KEYS[int(k)] for k in rng.integers(0, len(KEYS), size=n_entries)], dtype=np.uint32).view(np.int32)
        offs = rng.integers(0, 1 << 63, size=n_entries, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n_entries, dtype=np.uint64)
        offs[::7] = (1 << 64) - 1 - np.arange(len(offs[::7]), dtype=np.uint64)
        offs[1::7] = np.arange(len(offs[1::7]), dtype=np.uint64)
        self.offs = offs
        self.src_img = rng.integers(0, 256, size=self.src_n, dtype=np.uint8)
        self.src = M.DeviceBuffer(self.src_n)
        self.dst = M.DeviceBuffer(self.dst_n)
        self.src.upload(self.src_img)
        self.oracle = oracle

    def table(self, M, in_place=()):
        t = M.table(len(self.sizes))
        t["dst"] = self.dst.ptr + self.dst_off
        t["src"] = self.src.ptr + self.src_off
        t["n"] = self.sizes
        t["stream_off"] = self.offs
        t["key"] = self.keys
        for i in in_place:
            t["src"][i] = t["dst"][i]
        return t

    def reset(self, fill=0x5A):
        self.dst.upload(np.full(self.dst_n, fill, np.uint8))

    def expected(self, t, before=None):
        want = np.full(self.dst_n, 0x5A, np.uint8) if before is None else before.copy()
        base_d, base_s = self.dst.ptr, self.src.ptr
        for e in t:
            n = int(e["n"])
            if not n:
                continue
            d = int(e["dst"]) - base_d
            if int(e["src"]) == int(e["dst"]):
                seg = want[d:d + n].copy()
            else:
                s = int(e["src"]) - base_s
                seg = self.src_img[s:s + n].copy()
            self.oracle.cycle_at(seg, int(e["key"]) & 0xFFFFFFFF, int(e["stream_off"]))
            want[d:d + n] = seg
        return want

    def check(self, want, what):
        got = self.dst.download()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what}: {bad.size} bytes differ, first at arena offset {bad[0]}")
        assert np.array_equal(self.src.download(), self.src_img), (what, "source changed")

    def free(self):
        self.src.free()
        self.dst.free()


@pytest.mark.parametrize("n_entries", [1, 16, 17, 1000, 100000])
def test_table_parity(gpu, oracle, n_entries):
    """Random tables against the oracle, uploaded from numpy (validated) and, the second time, resident with a caller workspace."""
    a = Arena(gpu, oracle, n_entries, seed=n_entries, small=n_entries >= 1000)
    t = a.table(gpu)
    want = a.expected(t)
    a.reset()
    gpu.cycle_table_device(t)
    a.check(want, "uploaded table")
    # resident table and workspace; a phase sweep of both sides for the first 256 entries of the small tables
    if n_entries <= 17:
        t2 = t.copy()
        for i in range(len(t2)):
            t2["src"][i] = a.src.ptr + 16 * (i % 16) + (i * 7) % 16
    else:
        t2 = t
    tb = gpu.DeviceBuffer(t2.nbytes)
    tb.upload(t2.view(np.uint8))
    ws = gpu.DeviceBuffer(gpu.table_workspace_bytes(n_entries))
    a.reset()
    before = gpu.path_stats()["gpu_launches"]
    gpu.cycle_table_device(tb, ws, n=n_entries)
    a.dst.sync()
    assert gpu.path_stats()["gpu_launches"] - before == 3
    assert gpu.table_status(ws) is None
    info = gpu.last_launch()
    assert info["variant"] == 8 and info["source_hash"] == gpu.table_kernel_source_hash(), info
    a.check(a.expected(t2), "resident table")
    tb.free()
    ws.free()
    a.free()


def test_all_phases_and_edge_sizes(gpu, oracle):
    """All 16 x 16 destination / source phases at sizes 0..17, chunk +- 1 and several chunks, in one table."""
    sizes = [0, 1, 7, 15, 16, 17, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3]
    n = 256 * len(sizes)
    a = Arena(gpu, oracle, n, seed=5, sizes=sizes, phases=[((i // len(sizes)) % 16, (i // len(sizes)) // 16) for i in range(n)])
    t = a.table(gpu)
    gpu.table_validate(t)
    want = a.expected(t)
    a.reset()
    gpu.cycle_table_device(t)
    a.check(want, "phases")
    a.free()


def test_same_bytes_as_the_batch_call_and_in_place(gpu, oracle):
    """40 entries under one key: the table call's bytes equal modgpu_cycle_batch_device_to's; then in-place entries mixed in."""
    a = Arena(gpu, oracle, 40, seed=40)
    t = a.table(gpu)
    t["key"] = np.int32(gpu.as_int32(PS4))
    a.reset()
    gpu.cycle_batch_device_to([int(x) for x in t["dst"]], [int(x) for x in t["src"]], [int(x) for x in t["n"]], PS4,
                              stream_offs=[int(x) for x in t["stream_off"]])
    a.dst.sync()
    batch = a.dst.download()
    a.reset()
    gpu.cycle_table_device(t)
    assert np.array_equal(a.dst.download(), batch)
    # in place: every third entry cycles its own destination
    t2 = a.table(gpu, in_place=range(0, 40, 3))
    before = np.full(a.dst_n, 0x5A, np.uint8)
    before[::3] = (np.arange(before[::3].size) % 251).astype(np.uint8)
    a.dst.upload(before)
    gpu.cycle_table_device(t2)
    a.check(a.expected(t2, before), "in place")
    a.free()


def test_graph_replay_reads_the_table_each_time(gpu, oracle):
    """Captured once; the device table is rewritten (new keys and offsets) between replays and each replay follows it."""
    a = Arena(gpu, oracle, 300, seed=77, small=True)
    t = a.table(gpu)
    tb = gpu.DeviceBuffer(t.nbytes)
    ws = gpu.DeviceBuffer(gpu.table_workspace_bytes(len(t)))
    tb.upload(t.view(np.uint8))
    st = Stream()
    with Graph.capture(st) as g:
        gpu.cycle_table_device(tb, ws, n=len(t), stream=st.handle)
    rng = np.random.default_rng(3)
    for k in range(3):
        t["key"] = np.array([KEYS[int(x)] for x in rng.integers(0, len(KEYS), size=len(t))], dtype=np.uint32).view(np.int32)
        t["stream_off"] = rng.integers(0, 1 << 62, size=len(t), dtype=np.uint64)
        tb.upload(t.view(np.uint8))
        a.reset()
        g.launch(st)
        st.sync()
        assert gpu.table_status(ws) is None
        a.check(a.expected(t), ("replay", k))
    g.destroy()
    st.destroy()
    tb.free()
    ws.free()
    a.free()


def test_two_streams_two_workspaces(gpu, oracle):
    arenas = [Arena(gpu, oracle, 2000, seed=90 + i, small=True) for i in range(2)]
    streams = [Stream() for _ in arenas]
    res = []
    for a, st in zip(arenas, streams):
        t = a.table(gpu)
        tb = gpu.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        ws = gpu.DeviceBuffer(gpu.table_workspace_bytes(len(t)))
        a.reset()
        res.append((t, tb, ws))
    gpu.path_stats(reset=False)
    for (t, tb, ws), st in zip(res, streams):
        gpu.cycle_table_device(tb, ws, n=len(t), stream=st.handle)
    for a, (t, tb, ws), st in zip(arenas, res, streams):
        st.sync()
        assert gpu.table_status(ws) is None
        a.check(a.expected(t), "two streams")
        tb.free()
        ws.free()
        st.destroy()
        a.free()


def test_device_tier_refusal_writes_nothing(gpu, oracle):
    """Nonzero flags on entries 700 and 123 of 1000: the whole call writes nothing and the status names 123; the wrapper raises."""
    a = Arena(gpu, oracle, 1000, seed=11, small=True)
    t = a.table(gpu)
    t["flags"][700] = 1
    t["flags"][123] = 2
    tb = gpu.DeviceBuffer(t.nbytes)
    tb.upload(t.view(np.uint8))
    ws = gpu.DeviceBuffer(gpu.table_workspace_bytes(len(t)))
    a.reset()
    gpu.cycle_table_device(tb, ws, n=len(t))
    a.dst.sync()
    assert gpu.table_status(ws) == 123
    a.check(np.full(a.dst_n, 0x5A, np.uint8), "refused call")
    with pytest.raises(gpu.ModGpuError):
        gpu.cycle_table_device(t, check=False)
    a.check(np.full(a.dst_n, 0x5A, np.uint8), "refused call, uploaded")
    # the same workspace runs clean again once the table is fixed
    t["flags"] = 0
    tb.upload(t.view(np.uint8))
    gpu.cycle_table_device(tb, ws, n=len(t))
    a.dst.sync()
    assert gpu.table_status(ws) is None
    a.check(a.expected(t), "fixed table")
    tb.free()
    ws.free()
    a.free()


def test_launch_count_is_flat(gpu, oracle):
    """17 entries and 100 000 entries: three launches each."""
    deltas = []
    for n in (17, 100000):
        a = Arena(gpu, oracle, n, seed=n + 1, small=True)
        t = a.table(gpu)
        tb = gpu.DeviceBuffer(t.nbytes)
        tb.upload(t.view(np.uint8))
        ws = gpu.DeviceBuffer(gpu.table_workspace_bytes(n))
        before = gpu.path_stats()["gpu_launches"]
        gpu.cycle_table_device(tb, ws, n=n)
        deltas.append(gpu.path_stats()["gpu_launches"] - before)
        a.dst.sync()
        tb.free()
        ws.free()
        a.free()
    assert deltas == [3, 3], deltas


def test_entry_beyond_4_gib(gpu, oracle):
    """One entry of 4 GiB + 77 bytes at odd phases and an offset near 2^64: windows at the start, across 2^32 and at the end, read back
    through the out-of-place kernel under another key (one host copy of a window that crosses 4 GiB inside an allocation is refused
    by the runtime) and compared with the oracle over the source's known pattern."""
    n = (1 << 32) + 77
    src, dst = gpu.DeviceBuffer(n + 64), gpu.DeviceBuffer(n + 64)
    tile = np.random.default_rng(4).integers(0, 256, size=(1 << 24) + 13, dtype=np.uint8)
    for at in range(0, n + 64, tile.size):
        src.upload(tile[:min(tile.size, n + 64 - at)], offset=at)
    dst.upload(np.full(61, 0x5A, np.uint8), offset=n + 3)
    off = (1 << 64) - 12345
    t = gpu.table(1)
    t[0] = (dst.ptr + 3, src.ptr + 9, n, off, gpu.as_int32(PS3), 0)
    gpu.cycle_table_device(t)
    win = 1 << 20
    tmp = gpu.DeviceBuffer(win)
    for m in (0, (1 << 32) - win + 50, n - win):  # (the second window ends 50 bytes past 2^32)
        gpu.cycle_device_to(tmp.ptr, dst.ptr + 3 + m, win, PS4, 0)
        tmp.sync()
        got = oracle.cycle_at(tmp.download(), PS4, 0)
        want = np.take(tile, np.arange(9 + m, 9 + m + win) % tile.size)
        oracle.cycle_at(want, PS3, off % 0x7FFFFFFE + m)  # (positions are off + j, reduced mod the period, never mod 2^64)
        assert np.array_equal(got, want), m
    assert (dst.download(61, offset=n + 3) == 0x5A).all(), "bytes behind the entry"
    tmp.free()
    src.free()
    dst.free()
