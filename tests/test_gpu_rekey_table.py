"""GPU: the rekey table call (modgpu_rekey_table_device: a device-resident table of rekey entries, three launches) against the CPU
oracle and against the rekey calls.  Every case lays its entries' destinations disjointly in one arena pre-filled with a guard pattern
and checks the WHOLE arena -- each entry's bytes equal src ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j], every byte outside the
entries unchanged -- and that the sources did not change.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every
byte compared here came from a kernel."""
import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
M31 = 0x7FFFFFFF
KEYS = [PS4, PS3, 1, 0xFFFFFFFF, 0x80000000, 12345, M31, 0, 0x80000001, 0xDEADBEEF]  # incl. INT_MIN, -1, identity keys
CHUNK = 65536
SIZES = [0, 1, 5, 15, 16, 17, 4095, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
PERIOD = M31 - 1


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def rekey(oracle, seg, key_from, off_from, key_to, off_to):
    """the oracle's rekey of a host segment: both keystreams XORed in (keystream(key_from, n, off_from) ^ keystream(key_to, n, off_to))"""
    oracle.cycle_at(seg, int(key_from) & 0xFFFFFFFF, int(off_from))
    oracle.cycle_at(seg, int(key_to) & 0xFFFFFFFF, int(off_to))
    return seg


def offsets(rng, n):
    offs = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    offs[::7] = (1 << 64) - 1 - np.arange(len(offs[::7]), dtype=np.uint64)
    offs[1::7] = np.arange(len(offs[1::7]), dtype=np.uint64)
    return offs


class Arena:
    """n_entries entries: destinations disjoint (with gaps) at random phases in one arena, sources anywhere in a source buffer of
    random bytes (they may overlap each other), both keys from KEYS, both offsets independent and up to 2^64-1."""

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
        pick = lambda: np.array([KEYS[int(k)] for k in rng.integers(0, len(KEYS), size=n_entries)], dtype=np.uint32).view(np.int32)  # noqa: E731
        self.key_from, self.key_to = pick(), pick()
        self.off_from, self.off_to = offsets(rng, n_entries), offsets(rng, n_entries)
        self.src_img = rng.integers(0, 256, size=self.src_n, dtype=np.uint8)
        self.src = M.DeviceBuffer(self.src_n)
        self.dst = M.DeviceBuffer(self.dst_n)
        self.src.upload(self.src_img)
        self.oracle = oracle

    def table(self, M, in_place=()):
        t = M.rekey_table(len(self.sizes))
        t["dst"] = self.dst.ptr + self.dst_off
        t["src"] = self.src.ptr + self.src_off
        t["n"] = self.sizes
        t["off_from"] = self.off_from
        t["off_to"] = self.off_to
        t["key_from"] = self.key_from
        t["key_to"] = self.key_to
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
            want[d:d + n] = rekey(self.oracle, seg, e["key_from"], e["off_from"], e["key_to"], e["off_to"])
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


def resident(M, t):
    tb = M.DeviceBuffer(t.nbytes)
    tb.upload(t.view(np.uint8))
    ws = M.DeviceBuffer(M.rekey_table_workspace_bytes(len(t)))
    return tb, ws


@pytest.mark.parametrize("n_entries", [1, 16, 17, 1000, 100000])
def test_rekey_table_parity(gpu, oracle, n_entries):
    """Random tables against the oracle, uploaded from numpy (validated) and, the second time, resident with a caller workspace."""
    a = Arena(gpu, oracle, n_entries, seed=n_entries, small=n_entries >= 1000)
    t = a.table(gpu)
    want = a.expected(t)
    a.reset()
    gpu.rekey_table_device(t)
    a.check(want, "uploaded table")
    if n_entries <= 17:  # a phase sweep of the sources for the small tables
        t2 = t.copy()
        for i in range(len(t2)):
            t2["src"][i] = a.src.ptr + 16 * (i % 16) + (i * 7) % 16
    else:
        t2 = t
    tb, ws = resident(gpu, t2)
    a.reset()
    before = gpu.path_stats()["gpu_launches"]
    gpu.rekey_table_device(tb, ws, n=n_entries)
    a.dst.sync()
    assert gpu.path_stats()["gpu_launches"] - before == 3
    assert gpu.table_status(ws) is None
    info = gpu.last_launch()
    assert info["variant"] == 9 and info["source_hash"] == gpu.rekey_table_kernel_source_hash(), info
    a.check(a.expected(t2), "resident table")
    tb.free()
    ws.free()
    a.free()


def test_all_phases_and_edge_sizes(gpu, oracle):
    """All 16 x 16 destination / source phases at sizes 0..17, chunk +- 1 and several chunks, offsets of independent phases."""
    sizes = list(range(18)) + [CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3]
    n = 256 * len(sizes)
    a = Arena(gpu, oracle, n, seed=5, sizes=sizes, phases=[((i // len(sizes)) % 16, (i // len(sizes)) // 16) for i in range(n)])
    t = a.table(gpu)
    gpu.rekey_table_validate(t)
    want = a.expected(t)
    a.reset()
    gpu.rekey_table_device(t)
    a.check(want, "phases")
    a.free()


def test_degenerate_keys_match_the_rekey_call(gpu, oracle):
    """Per entry, mixed in one table: key_from == 0 mod 2^31-1, key_to == 0, both, the same reduced key at offsets equal mod 2^31-2
    (a copy), the same key at other offsets, and plain pairs.  Each entry's bytes equal modgpu_rekey_device_to's for it."""
    sizes = [1, 15, 16, 33, 4097, CHUNK + 3, 3 * CHUNK + 7]
    combos = [(0, PS4, 0), (M31, PS3, 0), (PS3, 0, 0), (PS4, M31, 0), (0, 0, 0), (M31, 0, 0), (PS3, PS3, PERIOD), (PS4, PS4, 3 * PERIOD),
              (0xFFFFFFFF, 0xFFFFFFFF, 0), (PS3, PS3, 1), (PS3, PS4, 0), (1, 0x80000000, 5)]
    n = len(sizes) * len(combos)
    a = Arena(gpu, oracle, n, seed=21, sizes=sizes)
    t = a.table(gpu)
    for i in range(n):
        kf, kt, shift = combos[i // len(sizes)]
        t["key_from"][i], t["key_to"][i] = gpu.as_int32(kf), gpu.as_int32(kt)
        if combos[i // len(sizes)][:2] in ((PS3, PS3), (PS4, PS4), (0xFFFFFFFF, 0xFFFFFFFF)) or shift == 5:
            t["off_to"][i] = (int(t["off_from"][i]) % (1 << 62)) + shift
            t["off_from"][i] = int(t["off_from"][i]) % (1 << 62)
    gpu.rekey_table_validate(t)
    want = a.expected(t)
    a.reset()
    gpu.rekey_table_device(t)
    a.check(want, "degenerate keys vs oracle")
    table_bytes = a.dst.download()
    a.reset()
    for e in t:
        if int(e["n"]):
            gpu.rekey_device_to(int(e["dst"]), int(e["src"]), int(e["key_from"]), int(e["key_to"]), int(e["off_from"]), int(e["off_to"]), n=int(e["n"]))
    a.dst.sync()
    assert np.array_equal(a.dst.download(), table_bytes)
    a.free()


def test_same_bytes_as_the_batch_call_and_in_place(gpu, oracle):
    """40 entries under one key pair: the table call's bytes equal modgpu_rekey_batch_device_to's, with every third entry in place."""
    a = Arena(gpu, oracle, 40, seed=40)
    t = a.table(gpu, in_place=range(0, 40, 3))
    t["key_from"] = np.int32(gpu.as_int32(PS3))
    t["key_to"] = np.int32(gpu.as_int32(PS4))
    before = np.full(a.dst_n, 0x5A, np.uint8)
    before[::3] = (np.arange(before[::3].size) % 251).astype(np.uint8)
    a.dst.upload(before)
    gpu.rekey_batch_device_to([int(x) for x in t["dst"]], [int(x) for x in t["src"]], [int(x) for x in t["n"]], PS3, PS4,
                              offs_from=[int(x) for x in t["off_from"]], offs_to=[int(x) for x in t["off_to"]])
    a.dst.sync()
    batch = a.dst.download()
    a.dst.upload(before)
    gpu.rekey_table_device(t)
    assert np.array_equal(a.dst.download(), batch)
    a.check(a.expected(t, before), "in place")
    a.free()


def test_relocation_of_an_encrypted_part_ps3_to_ps4(gpu, oracle):
    """A PS3-encrypted part of 3000 files; a new file is inserted near the front and two files change size, so every file after them
    moves.  One table call moves each kept file to its new offset under PS4.  The result equals decrypting, moving and encrypting on
    the host; the bytes between files (where the new and resized data go) keep the guard."""
    rng = np.random.default_rng(33)
    sizes = rng.integers(0, 9000, size=3000)
    sizes[::97] = rng.integers(CHUNK - 8, 3 * CHUNK, size=sizes[::97].size)
    old_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    old_n = int(sizes.sum())
    plain = oracle.splitmix_bytes(old_n, 7)
    part = plain.copy()
    oracle.cycle_at(part, PS3, 0)
    new_sizes = sizes.copy()
    new_sizes[10] += 333
    new_sizes[2000] += 1
    insert_at, inserted = 5, 12345
    new_off = np.zeros_like(old_off)
    cur = 0
    for i in range(len(sizes)):
        if i == insert_at:
            cur += inserted
        new_off[i] = cur
        cur += int(new_sizes[i])
    new_n = cur
    src, dst = gpu.DeviceBuffer(old_n), gpu.DeviceBuffer(new_n)
    src.upload(part)
    dst.upload(np.full(new_n, 0x5A, np.uint8))
    keep = [i for i in range(len(sizes)) if new_sizes[i] == sizes[i]]  # resized files are rewritten by the caller, not moved
    t = gpu.rekey_table(len(keep))
    t["dst"] = dst.ptr + new_off[keep]
    t["src"] = src.ptr + old_off[keep]
    t["n"] = sizes[keep]
    t["off_from"] = old_off[keep]
    t["off_to"] = new_off[keep]
    t["key_from"] = gpu.as_int32(PS3)
    t["key_to"] = gpu.as_int32(PS4)
    gpu.rekey_table_device(t)
    want = np.full(new_n, 0x5A, np.uint8)
    for i in keep:
        want[int(new_off[i]):int(new_off[i]) + int(sizes[i])] = plain[int(old_off[i]):int(old_off[i]) + int(sizes[i])]
    whole = want.copy()
    oracle.cycle_at(whole, PS4, 0)
    for i in keep:  # the moved files are the new part's PS4 ciphertext at their new offsets; the rest keeps the guard
        want[int(new_off[i]):int(new_off[i]) + int(sizes[i])] = whole[int(new_off[i]):int(new_off[i]) + int(sizes[i])]
    got = dst.download()
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    assert np.array_equal(src.download(), part)
    src.free()
    dst.free()


def test_graph_replay_reads_the_table_each_time(gpu, oracle):
    """Captured once; the device table is rewritten (new key pairs and offsets) between replays and each replay follows it."""
    a = Arena(gpu, oracle, 300, seed=77, small=True)
    t = a.table(gpu)
    tb, ws = resident(gpu, t)
    st = Stream()
    with Graph.capture(st) as g:
        gpu.rekey_table_device(tb, ws, n=len(t), stream=st.handle)
    rng = np.random.default_rng(3)
    for k in range(3):
        for f in ("key_from", "key_to"):
            t[f] = np.array([KEYS[int(x)] for x in rng.integers(0, len(KEYS), size=len(t))], dtype=np.uint32).view(np.int32)
        t["off_from"] = rng.integers(0, 1 << 62, size=len(t), dtype=np.uint64)
        t["off_to"] = rng.integers(0, 1 << 62, size=len(t), dtype=np.uint64)
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
    for a in arenas:
        t = a.table(gpu)
        tb, ws = resident(gpu, t)
        a.reset()
        res.append((t, tb, ws))
    for (t, tb, ws), st in zip(res, streams):
        gpu.rekey_table_device(tb, ws, n=len(t), stream=st.handle)
    for a, (t, tb, ws), st in zip(arenas, res, streams):
        st.sync()
        assert gpu.table_status(ws) is None
        a.check(a.expected(t), "two streams")
        tb.free()
        ws.free()
        st.destroy()
        a.free()


def test_device_tier_refusal_writes_nothing(gpu, oracle):
    """Nonzero reserved on entry 700 and nonzero flags on entry 123 of 1000: the whole call writes nothing and modgpu_table_status
    names 123; the wrapper raises; the same workspace runs clean once the table is fixed."""
    a = Arena(gpu, oracle, 1000, seed=11, small=True)
    t = a.table(gpu)
    t["reserved"][700] = 1
    t["flags"][123] = 2
    tb, ws = resident(gpu, t)
    a.reset()
    gpu.rekey_table_device(tb, ws, n=len(t))
    a.dst.sync()
    assert gpu.table_status(ws) == 123
    a.check(np.full(a.dst_n, 0x5A, np.uint8), "refused call")
    with pytest.raises(gpu.ModGpuError):
        gpu.rekey_table_device(t, check=False)
    a.check(np.full(a.dst_n, 0x5A, np.uint8), "refused call, uploaded")
    t["flags"][123] = 0
    tb.upload(t.view(np.uint8))
    gpu.rekey_table_device(tb, ws, n=len(t))
    a.dst.sync()
    assert gpu.table_status(ws) == 700
    t["reserved"][700] = 0
    tb.upload(t.view(np.uint8))
    gpu.rekey_table_device(tb, ws, n=len(t))
    a.dst.sync()
    assert gpu.table_status(ws) is None
    a.check(a.expected(t), "fixed table")
    tb.free()
    ws.free()
    a.free()


def test_both_grids_give_the_same_bytes(gpu, oracle):
    """The table call's grid (25 workgroups per 32 CUs) and one workgroup per CU (testing flavour) give identical bytes."""
    with gpu.testing_flavour():
        a = Arena(gpu, oracle, 3000, seed=55, small=True)
        t = a.table(gpu)
        tb, ws = resident(gpu, t)
        want = a.expected(t)
        got, grids = {}, {}
        try:
            for grid in (200, 256, 0):
                gpu.debug_set_rekey_table_grid(grid)
                a.reset()
                gpu.rekey_table_device(tb, ws, n=len(t))
                a.dst.sync()
                grids[grid] = gpu.last_launch()["grid"]
                got[grid] = a.dst.download()
                a.check(want, ("grid", grid))
        finally:
            gpu.debug_set_rekey_table_grid(0)
        assert grids[200] == 200 and grids[256] == 256, grids
        assert np.array_equal(got[200], got[256])
        tb.free()
        ws.free()
        a.free()


def test_entry_beyond_4_gib(gpu, oracle):
    """One entry of 4 GiB + 77 bytes at odd phases, offsets near 2^64 and at another phase: windows at the start, across 2^32 and at
    the end, read back through the out-of-place kernel under another key and compared with the oracle over the source's pattern."""
    n = (1 << 32) + 77
    src, dst = gpu.DeviceBuffer(n + 64), gpu.DeviceBuffer(n + 64)
    tile = np.random.default_rng(4).integers(0, 256, size=(1 << 24) + 13, dtype=np.uint8)
    for at in range(0, n + 64, tile.size):
        src.upload(tile[:min(tile.size, n + 64 - at)], offset=at)
    dst.upload(np.full(61, 0x5A, np.uint8), offset=n + 3)
    off_from, off_to = (1 << 64) - 12345, 987654321011
    t = gpu.rekey_table(1)
    t[0] = (dst.ptr + 3, src.ptr + 9, n, off_from, off_to, gpu.as_int32(PS3), gpu.as_int32(PS4), 0, 0)
    gpu.rekey_table_device(t)
    win = 1 << 20
    tmp = gpu.DeviceBuffer(win)
    for m in (0, (1 << 32) - win + 50, n - win):  # (the second window ends 50 bytes past 2^32)
        gpu.cycle_device_to(tmp.ptr, dst.ptr + 3 + m, win, 12345, 0)
        tmp.sync()
        got = oracle.cycle_at(tmp.download(), 12345, 0)
        want = np.take(tile, np.arange(9 + m, 9 + m + win) % tile.size)
        rekey(oracle, want, PS3, off_from % PERIOD + m, PS4, off_to + m)  # (positions reduced mod the period, never mod 2^64)
        assert np.array_equal(got, want), m
    assert (dst.download(61, offset=n + 3) == 0x5A).all(), "bytes behind the entry"
    tmp.free()
    src.free()
    dst.free()
