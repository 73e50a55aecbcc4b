"""GPU: the rekey verify table call (modgpu_verify_rekey_table_device: a device-resident table of rekey entries, `dst` read as the
comparand, three launches) against numpy over host images.  Every case lays its comparands disjointly in one arena made with the
oracle's cycle_at of each entry's source under key_from / off_from and then under key_to / off_to, plants mismatches by XORing chosen
bytes, and checks every entry's {mismatches, first_mismatch, n, 0}, the call's summary (through modgpu_verify_table_summary), that BOTH
arenas are byte-identical afterwards and that the guard bytes in front of and behind the results array did not change.  All
comparisons are exact.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every number compared here came from a
kernel."""
import ctypes

import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
KEYS = [PS4, PS3, 1, 0xFFFFFFFF, 0x80000000, 12345, 0x7FFFFFFF, 0, 0x80000001, 0xDEADBEEF]  # incl. INT_MIN, -1, identity keys
M31 = (1 << 31) - 1
PERIOD = M31 - 1
CHUNK = 65536
SIZES = [0, 1, 5, 15, 16, 17, 4095, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
NONE = (1 << 64) - 1
GUARD = 64


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def i32(key):
    key &= 0xFFFFFFFF
    return key - (1 << 32) if key & 0x80000000 else key


def residue(key):
    """the key as the cipher reduces it: the signed 32-bit value mod 2^31-1; 0 is the identity keystream"""
    return i32(key) % M31


def stream_class(kf, of, kt, ot):
    """'two' for two genuinely different keystreams, else the degenerate class the pair falls in"""
    rf, rt = residue(int(kf)), residue(int(kt))
    if rf == 0 and rt == 0:
        return "both_identity"
    if rf == 0:
        return "from_identity"
    if rt == 0:
        return "to_identity"
    if rf == rt and int(of) % PERIOD == int(ot) % PERIOD:
        return "cancel"
    return "two"


def plant_positions(addr, n):
    """entry indices where the kernels change path: the ends, either side of the head / body / tail seams, either side of every chunk
    edge of the comparand's chunk grid (the first few and the last)"""
    if n == 0:
        return []
    head = min(n, (16 - (addr & 15)) & 15)
    body = (n - head) // 16 * 16
    lead = (addr + head) % CHUNK
    pos = [0, n - 1, head - 1, head, head + body - 1, head + body]
    edges = list(range(CHUNK - lead, body, CHUNK))
    for e in edges[:3] + edges[-1:]:
        pos += [head + e - 1, head + e, head + e + 1]
    return sorted({p for p in pos if 0 <= p < n})


def random_offsets(rng, n):
    offs = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    return offs


class Arena:
    """n_entries entries: comparands disjoint (with gaps) at random phases in one arena, sources anywhere in a source buffer of random
    bytes (they may overlap each other), key pairs drawn independently from KEYS, both offsets up to 2^64-1.  The comparand arena is
    cycle_at under key_from / off_from and then under key_to / off_to of each entry's source; plant() then makes entries dirty."""

    def __init__(self, M, oracle, n_entries, seed, sizes=SIZES, small=False, phases=None, keys=None, off_phases=None):
        rng = np.random.default_rng(seed)
        self.rng = rng
        if small:  # many entries: mostly small, some around a chunk
            sz = rng.integers(0, 4096, size=n_entries)
            pick = rng.random(n_entries) < 0.02
            sz[pick] = rng.integers(CHUNK - 16, 2 * CHUNK + 16, size=int(pick.sum()))
            sz[5:7] = (777, CHUNK + 5)  # (the entries draw_keys gives cancelling streams are not empty)
        else:
            sz = np.array([sizes[(i - 1) % len(sizes)] for i in range(n_entries)], dtype=np.int64)  # (entry 0: the last size)
        self.sizes = sz.astype(np.uint64)
        self.src_n = int(max(4 * CHUNK, sz.max() + 64, int(sz.sum()) // 2 + 64))
        gaps = rng.integers(1, 48, size=n_entries)
        cur, exp_off = 64, []
        for i, s in enumerate(sz):
            if phases is not None:  # (comparand phase, source phase) of entry i
                cur = ((cur + 15) & ~15) + phases[i][0]
            exp_off.append(cur)
            cur += int(s) + int(gaps[i])
        self.exp_off = np.array(exp_off, dtype=np.uint64)
        self.exp_n = cur + 64
        if phases is not None:
            self.src_off = np.array([16 * (i % 64) + phases[i][1] for i in range(n_entries)], dtype=np.uint64)
        else:
            self.src_off = np.array([int(rng.integers(0, self.src_n - s + 1)) for s in sz], dtype=np.uint64)
        self.draw_keys(rng, keys, off_phases)
        self.src_img = rng.integers(0, 256, size=self.src_n, dtype=np.uint8)
        self.src = M.DeviceBuffer(self.src_n)
        self.exp = M.DeviceBuffer(self.exp_n)
        self.src.upload(self.src_img)
        self.oracle, self.M = oracle, M
        self.remake()

    def draw_keys(self, rng, keys=None, off_phases=None):
        n = len(self.sizes)
        if keys is None:
            self.keys_from = np.array([KEYS[int(k)] for k in rng.integers(0, len(KEYS), size=n)], dtype=np.uint32).view(np.int32)
            self.keys_to = np.array([KEYS[int(k)] for k in rng.integers(0, len(KEYS), size=n)], dtype=np.uint32).view(np.int32)
        else:
            self.keys_from = np.full(n, keys[0], dtype=np.uint32).view(np.int32)
            self.keys_to = np.full(n, keys[1], dtype=np.uint32).view(np.int32)
        of, ot = random_offsets(rng, n), random_offsets(rng, n)
        of[::7] = (1 << 64) - 1 - np.arange(len(of[::7]), dtype=np.uint64)
        ot[3::7] = (1 << 64) - 1 - np.arange(len(ot[3::7]), dtype=np.uint64)
        of[1::7] = np.arange(len(of[1::7]), dtype=np.uint64)
        ot[2::7] = np.arange(len(ot[2::7]), dtype=np.uint64)
        if off_phases is not None:  # (off_from, off_to) mod 16 of entry i
            for i in range(n):
                of[i] = (int(of[i]) & ~15 & NONE) | off_phases[i][0]
                ot[i] = (int(ot[i]) & ~15 & NONE) | off_phases[i][1]
        self.offs_from, self.offs_to = of, ot
        if keys is None and n <= 17:  # the two-stream path must not hang on the draw: entry 0 is PS3 -> PS4
            self.keys_from[0], self.keys_to[0] = i32(PS3), i32(PS4)
        if keys is None and off_phases is None and n >= 300:  # the class random offsets never hit: the same key at offsets equal mod 2^31-2
            for i in (5, 6):
                self.keys_from[i] = self.keys_to[i] = i32(PS3 if i == 5 else 12345)
                self.offs_from[i] = int(self.offs_from[i]) >> 2
                self.offs_to[i] = int(self.offs_from[i]) + (i - 2) * PERIOD

    def classes(self):
        return [stream_class(self.keys_from[i], self.offs_from[i], self.keys_to[i], self.offs_to[i]) for i in range(len(self.sizes))]

    def check_mix(self):
        """the cap on the draw: at 1000 entries or more, at least 40 % of the non-empty entries have two genuinely different streams
        (independent pairs from KEYS give 49 %), and each degenerate class occurs"""
        cl = [c for c, s in zip(self.classes(), self.sizes) if s]
        assert cl.count("two") >= 0.4 * len(cl), (cl.count("two"), len(cl))
        for c in ("from_identity", "to_identity", "both_identity", "cancel"):
            assert c in cl, c

    def remake(self):
        """the clean comparand image of the current keys and offsets (the reference, computed once per set of keys)"""
        clean = np.full(self.exp_n, 0x5A, np.uint8)
        for i in range(len(self.sizes)):
            n = int(self.sizes[i])
            if n:
                s, d = int(self.src_off[i]), int(self.exp_off[i])
                seg = self.src_img[s:s + n].copy()
                self.oracle.cycle_at(seg, int(self.keys_from[i]) & 0xFFFFFFFF, int(self.offs_from[i]))
                self.oracle.cycle_at(seg, int(self.keys_to[i]) & 0xFFFFFFFF, int(self.offs_to[i]))
                clean[d:d + n] = seg
        self.clean = clean
        self.exp_img = clean.copy()

    def plant(self, dirty, several=3):
        """XORs bytes of the entries in `dirty`: `several` positions each, drawn from plant_positions in turn and one random"""
        self.exp_img = self.clean.copy()
        for k, i in enumerate(dirty):
            n, d = int(self.sizes[i]), int(self.exp_off[i])
            pos = plant_positions(self.exp.ptr + d, n)
            if not pos:
                continue
            take = [pos[(k + m * 5) % len(pos)] for m in range(several)] + [int(self.rng.integers(0, n))]
            for p in set(take):
                self.exp_img[d + p] ^= np.uint8(1 + (k + p) % 255)
        self.exp.upload(self.exp_img)

    def table(self):
        t = self.M.rekey_table(len(self.sizes))
        t["dst"] = self.exp.ptr + self.exp_off
        t["src"] = self.src.ptr + self.src_off
        t["n"] = self.sizes
        t["off_from"] = self.offs_from
        t["off_to"] = self.offs_to
        t["key_from"] = self.keys_from
        t["key_to"] = self.keys_to
        return t

    def expected(self, want_img=None):
        """numpy over the host images: per entry (mismatches, first_mismatch, n)"""
        ref = self.clean if want_img is None else want_img
        diff = self.exp_img != ref
        out = np.zeros(len(self.sizes), dtype=self.M.VERIFY_RESULT_DTYPE)
        out["n"] = self.sizes
        out["first_mismatch"] = NONE
        for i in range(len(self.sizes)):
            d, n = int(self.exp_off[i]), int(self.sizes[i])
            seg = diff[d:d + n]
            if seg.any():
                out["mismatches"][i] = int(seg.sum())
                out["first_mismatch"][i] = int(np.argmax(seg))
        return out

    def check_unchanged(self, what):
        assert np.array_equal(self.exp.download(), self.exp_img), (what, "comparand arena changed")
        assert np.array_equal(self.src.download(), self.src_img), (what, "source arena changed")

    def free(self):
        self.src.free()
        self.exp.free()


def summary_of(want):
    dirty = np.flatnonzero(want["mismatches"])
    return {"mismatches": int(want["mismatches"].sum()), "first_bad_entry": int(dirty[0]) if dirty.size else None, "entries": len(want)}


class Results:
    """a results array for n entries between two guard bands, pre-filled with 0xA5"""

    def __init__(self, M, n):
        self.M, self.n = M, n
        self.buf = M.DeviceBuffer(2 * GUARD + 32 * n)
        self.fill()

    @property
    def ptr(self):
        return self.buf.ptr + GUARD

    def fill(self):
        self.buf.upload(np.full(2 * GUARD + 32 * self.n, 0xA5, np.uint8))

    def read(self, what=""):
        got = self.buf.download()
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + 32 * self.n:] == 0xA5).all(), (what, "guard bytes around the results were written")
        return got[GUARD:GUARD + 32 * self.n].view(self.M.VERIFY_RESULT_DTYPE)

    def free(self):
        self.buf.free()


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got["mismatches"] != want["mismatches"]) | (got["first_mismatch"] != want["first_mismatch"]) | (got["n"] != want["n"]) |
                             (got["reserved"] != want["reserved"]))
        raise AssertionError(f"{what}: {bad.size} results differ, first entry {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")


def resident(M, t):
    tb = M.DeviceBuffer(t.nbytes)
    tb.upload(t.view(np.uint8))
    return tb, M.DeviceBuffer(M.verify_rekey_table_workspace_bytes(len(t)))


def run_resident(M, a, tb, ws, res, n, want, what, stream=None):
    res.fill()
    M.verify_rekey_table_device(tb, res.ptr, ws, n=n, stream=stream)
    M.lib().modgpu_sync(-1, ctypes.c_void_p(stream or 0))
    assert M.table_status(ws) is None, what
    same(res.read(what), want, what)
    assert M.verify_table_summary(ws) == summary_of(want), what
    a.check_unchanged(what)


@pytest.mark.parametrize("n_entries", [1, 16, 17, 1000, 100000])
def test_verify_rekey_table_parity(gpu, oracle, n_entries):
    """About a third of the entries dirty at the seams; once with the table uploaded by the wrapper, once resident with a caller
    workspace: three launches, a clean status, variant 13, the summary where the verify table call has it."""
    a = Arena(gpu, oracle, n_entries, seed=n_entries, small=n_entries >= 1000)
    if n_entries >= 1000:
        a.check_mix()
    else:
        assert a.classes()[0] == "two"
    a.plant([i for i in range(n_entries) if i % 3 == 0])
    t = a.table()
    want = a.expected()
    assert (want["mismatches"] > 0).sum() >= max(1, n_entries // 8)
    got = gpu.verify_rekey_table_device(t)
    same(got, want, "uploaded table")
    a.check_unchanged("uploaded table")
    tb, ws = resident(gpu, t)
    res = Results(gpu, n_entries)
    before = gpu.path_stats()["gpu_launches"]
    gpu.verify_rekey_table_device(tb, res.ptr, ws, n=n_entries)
    a.exp.sync()
    assert gpu.path_stats()["gpu_launches"] - before == 3
    assert gpu.table_status(ws) is None
    info = gpu.last_launch()
    assert info["variant"] == 13 and info["bytes"] == 0 and info["source_hash"] == gpu.rekey_verify_table_kernel_source_hash(), info
    assert info["kernel"] == "modgpu_cycle_rekey_verify_table_kernel<4, 1024>", info
    same(res.read("resident"), want, "resident table")
    assert gpu.verify_table_summary(ws) == summary_of(want)
    a.check_unchanged("resident table")
    # ... and clean: no finding anywhere
    a.plant([])
    run_resident(gpu, a, tb, ws, res, n_entries, a.expected(), "clean")
    for b in (tb, ws, res, a):
        b.free()


def test_all_phases_and_edge_sizes(gpu, oracle):
    """All 16 x 16 comparand / source phases at sizes 0..17, chunk +- 1 and several chunks, in one table, the two offsets' phases
    mod 16 varying independently of them; every second entry dirty in one byte whose position cycles through the seams."""
    sizes = [0, 1, 7, 15, 16, 17, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3]
    n = 256 * len(sizes)
    a = Arena(gpu, oracle, n, seed=5, sizes=sizes, phases=[((i // len(sizes)) % 16, (i // len(sizes)) // 16) for i in range(n)],
              off_phases=[((7 * i) % 16, (11 * i + 3) % 16) for i in range(n)])
    assert all(int(a.offs_from[i]) % 16 == (7 * i) % 16 and int(a.offs_to[i]) % 16 == (11 * i + 3) % 16 for i in range(n))
    a.exp_img = a.clean.copy()
    for k, i in enumerate(range(0, n, 2)):
        pos = plant_positions(a.exp.ptr + int(a.exp_off[i]), int(a.sizes[i]))
        if pos:
            a.exp_img[int(a.exp_off[i]) + pos[k % len(pos)]] ^= np.uint8(0x80 >> (k % 8))
    a.exp.upload(a.exp_img)
    want = a.expected()
    assert set(want["mismatches"]) == {0, 1}
    same(gpu.verify_rekey_table_device(a.table()), want, "phases")
    a.check_unchanged("phases")
    a.free()


def test_degenerate_keystreams_on_the_one_kernel(gpu, oracle):
    """key_from == 0 mod 2^31-1, key_to == 0, both, the same key at equal offsets, at offsets 2^31-2 apart and at offsets 1 apart,
    each clean and dirty at 17 and CHUNK + 77 bytes: byte-identical to modgpu_verify_rekey_device per entry, and to
    modgpu_verify_table_device for the entries that reduce to one keystream."""
    o1, o2 = (1 << 40) + 12345, (1 << 63) + 7
    shapes = [(k, o1, PS4, o2) for k in (0, 0x7FFFFFFF, 0x80000001)] + [(PS3, o1, k, o2) for k in (0, 0x7FFFFFFF, 0x80000001)]
    shapes += [(0, o1, 0x80000001, o2), (PS3, o1, PS3, o1), (PS4, o1, PS4, o1 + PERIOD), (PS3, o1, PS3, o1 + 1)]
    want_class = 3 * ["from_identity"] + 3 * ["to_identity"] + ["both_identity", "cancel", "cancel", "two"]
    cases = [(sh, size, dirty) for sh in shapes for size in (17, CHUNK + 77) for dirty in (False, True)]
    n = len(cases)
    a = Arena.__new__(Arena)  # (laid out here: the sizes and keys are the cases', not a draw)
    rng = np.random.default_rng(33)
    a.rng, a.M, a.oracle = rng, gpu, oracle
    a.sizes = np.array([c[1] for c in cases], dtype=np.uint64)
    cur, exp_off = 64, []
    for i, s in enumerate(a.sizes):
        cur = ((cur + 15) & ~15) + (3 * i) % 16
        exp_off.append(cur)
        cur += int(s) + 7
    a.exp_off, a.exp_n = np.array(exp_off, dtype=np.uint64), cur + 64
    a.src_n = 4 * CHUNK
    a.src_off = np.array([16 * i + (5 * i + 1) % 16 for i in range(n)], dtype=np.uint64)
    a.keys_from = np.array([c[0][0] for c in cases], dtype=np.uint32).view(np.int32)
    a.keys_to = np.array([c[0][2] for c in cases], dtype=np.uint32).view(np.int32)
    a.offs_from = np.array([c[0][1] for c in cases], dtype=np.uint64)
    a.offs_to = np.array([c[0][3] for c in cases], dtype=np.uint64)
    assert a.classes() == [want_class[i // 4] for i in range(n)]
    a.src_img = rng.integers(0, 256, size=a.src_n, dtype=np.uint8)
    a.src, a.exp = gpu.DeviceBuffer(a.src_n), gpu.DeviceBuffer(a.exp_n)
    a.src.upload(a.src_img)
    a.remake()
    a.plant([i for i, c in enumerate(cases) if c[2]], several=2)
    t = a.table()
    want = a.expected()
    assert all((want["mismatches"][i] > 0) == cases[i][2] for i in range(n))
    got = gpu.verify_rekey_table_device(t)
    same(got, want, "degenerate")
    one = gpu.table(n)  # the single-keystream reading of the entries that have one
    single = []
    for i, c in enumerate(a.classes()):
        r = gpu.verify_rekey_device(int(t["dst"][i]), int(t["src"][i]), int(t["key_from"][i]), int(t["key_to"][i]), int(t["off_from"][i]),
                                    int(t["off_to"][i]), n=int(t["n"][i]))
        assert r.tobytes() == got[i].tobytes(), (i, c, r, got[i])
        if c != "two":
            key, off = {"from_identity": (t["key_to"][i], t["off_to"][i]), "to_identity": (t["key_from"][i], t["off_from"][i])}.get(c, (0, 0))
            one[i] = (t["dst"][i], t["src"][i], t["n"][i], off, key, 0)
            single.append(i)
    assert len(single) == n - 4
    got_one = gpu.verify_table_device(one)
    assert got_one[single].tobytes() == got[single].tobytes()
    a.check_unchanged("degenerate")
    a.free()


def test_same_answers_as_the_batch_and_the_one_buffer_call(gpu, oracle):
    """40 entries under one key pair: dev_results byte-identical to modgpu_verify_rekey_batch_device's; one entry also against
    modgpu_verify_rekey_device."""
    a = Arena(gpu, oracle, 40, seed=40, keys=(PS3, PS4))
    a.plant(range(0, 40, 2))
    t = a.table()
    res_b, res_t = Results(gpu, 40), Results(gpu, 40)
    gpu.verify_rekey_batch_device([int(x) for x in t["dst"]], [int(x) for x in t["src"]], [int(x) for x in t["n"]], PS3, PS4, res_b.ptr,
                                  offs_from=[int(x) for x in t["off_from"]], offs_to=[int(x) for x in t["off_to"]])
    tb, ws = resident(gpu, t)
    gpu.verify_rekey_table_device(tb, res_t.ptr, ws, n=40)
    a.exp.sync()
    batch, table = res_b.read("batch"), res_t.read("table")
    assert batch.tobytes() == table.tobytes()
    same(table, a.expected(), "table")
    i = 22  # 3 * CHUNK + 5 bytes, dirty
    assert int(t["n"][i]) == 3 * CHUNK + 5
    one = gpu.verify_rekey_device(int(t["dst"][i]), int(t["src"][i]), PS3, PS4, int(t["off_from"][i]), int(t["off_to"][i]), n=int(t["n"][i]))
    assert one.tobytes() == table[i].tobytes() and int(one["mismatches"]) > 0
    for b in (tb, ws, res_b, res_t, a):
        b.free()


def test_the_table_that_rekeyed_verifies_its_own_result(gpu, oracle):
    """The user story: a 300-entry rekey table with mixed key pairs writes into a scratch arena; the SAME table, verified, reports 0
    mismatches and a clean summary; three bytes flipped in the scratch arena by one-byte uploads are reported in exactly those entries
    at exactly those indices."""
    a = Arena(gpu, oracle, 300, seed=300, small=True)
    t = a.table()
    a.exp.upload(np.full(a.exp_n, 0x5A, np.uint8))  # the scratch arena: nothing of the oracle's image in it
    tb, ws = resident(gpu, t)
    wr = gpu.DeviceBuffer(gpu.rekey_table_workspace_bytes(300))
    gpu.rekey_table_device(tb, wr, n=300)
    a.exp.sync()
    assert gpu.table_status(wr) is None
    a.exp_img = a.clean.copy()
    res = Results(gpu, 300)
    run_resident(gpu, a, tb, ws, res, 300, a.expected(), "the rekey table's own result")
    flips = {}
    for i in [int(x) for x in np.flatnonzero(a.sizes > 40)[[3, 50, -1]]]:
        flips[i] = int(a.sizes[i]) // 2 + i % 5
        at = int(a.exp_off[i]) + flips[i]
        a.exp_img[at] ^= np.uint8(0x10)
        a.exp.upload(a.exp_img[at:at + 1], offset=at)
    want = a.expected()
    assert {int(i): int(want["first_mismatch"][i]) for i in np.flatnonzero(want["mismatches"])} == flips and want["mismatches"].sum() == 3
    run_resident(gpu, a, tb, ws, res, 300, want, "three flipped bytes")
    for b in (tb, ws, wr, res, a):
        b.free()


def test_every_byte_wrong(gpu, oracle):
    """An entry of 3 * CHUNK + 5 bytes compared under the WRONG key_to, a clean entry on either side: the count is numpy's (two
    keystreams agree in a byte now and then, so it is not n)."""
    a = Arena(gpu, oracle, 3, seed=8, sizes=[3 * CHUNK + 5, 4097, CHUNK + 9], keys=(PS3, PS4))
    t = a.table()
    t["key_to"][1] = gpu.as_int32(12345)
    d, n, s = int(a.exp_off[1]), int(a.sizes[1]), int(a.src_off[1])
    assert n == 3 * CHUNK + 5
    ref = a.clean.copy()
    seg = a.src_img[s:s + n].copy()
    oracle.cycle_at(seg, PS3, int(a.offs_from[1]))
    oracle.cycle_at(seg, 12345, int(a.offs_to[1]))
    ref[d:d + n] = seg
    a.exp.upload(a.exp_img)
    want = a.expected(ref)
    assert n * 0.99 < int(want["mismatches"][1]) <= n and want["mismatches"][0] == 0 and want["mismatches"][2] == 0
    same(gpu.verify_rekey_table_device(t), want, "wrong key")
    a.check_unchanged("wrong key")
    a.free()


def test_small_grids_flush_between_entries(gpu, oracle):
    """12 entries of 5 chunks + 9 bytes, each dirty in its first, a middle and its last chunk, on 1, 3 and the shipped number of
    workgroups (testing flavour): one workgroup passes several entries and must hand each its own findings."""
    with gpu.testing_flavour():
        n = 5 * CHUNK + 9
        a = Arena(gpu, oracle, 12, seed=12, sizes=[n], phases=[(i % 16, (5 * i + 3) % 16) for i in range(12)])
        a.exp_img = a.clean.copy()
        for i in range(12):
            d = int(a.exp_off[i])
            for p in (100 + i, 2 * CHUNK + 4097 * (i + 1) % CHUNK, 3 * CHUNK - 1 - i, n - 20 - i, n - 1 - (i % 3)):
                a.exp_img[d + p] ^= np.uint8(i + 1)
        a.exp.upload(a.exp_img)
        want = a.expected()
        assert (want["mismatches"] == 5).all()
        t = a.table()
        tb, ws = resident(gpu, t)
        res = Results(gpu, 12)
        try:
            for grid in (1, 3, 0):
                gpu.debug_set_rekey_verify_table_grid(grid)
                run_resident(gpu, a, tb, ws, res, 12, want, ("grid", grid))
                if grid:
                    assert gpu.last_launch()["grid"] == grid
        finally:
            gpu.debug_set_rekey_verify_table_grid(0)
        for b in (tb, ws, res, a):
            b.free()


def test_no_overlap_rule(gpu, oracle):
    """dst == src under two identity keys: 0 mismatches; two entries reading the same ranges: equal results; a comparand that overlaps
    another entry's source: still numpy's answer."""
    a = Arena(gpu, oracle, 6, seed=21, sizes=[CHUNK + 77], keys=(PS3, PS4))
    a.plant([2])
    t = a.table()
    t[0] = (a.src.ptr + 5, a.src.ptr + 5, CHUNK + 77, 9, 11, 0, 0x7FFFFFFF, 0, 0)                 # itself, two identity keys
    t[1] = (a.src.ptr + 1000, a.src.ptr + 1000, 3 * CHUNK, 1 << 63, 5, gpu.as_int32(0x80000001), 0, 0, 0)  # itself, two identity keys
    t[3] = t[2]
    t[4] = (a.src.ptr + 16, a.src.ptr + 17, CHUNK, 77, 77 + PERIOD, gpu.as_int32(PS4), gpu.as_int32(PS4), 0, 0)  # shifted by one, streams cancel
    got = gpu.verify_rekey_table_device(t)
    assert tuple(got[0]) == (0, NONE, CHUNK + 77, 0) and tuple(got[1]) == (0, NONE, 3 * CHUNK, 0)
    want = a.expected()
    assert tuple(got[2]) == tuple(want[2]) == tuple(got[3]) and int(got[2]["mismatches"]) > 0
    shifted = a.src_img[16:16 + CHUNK] != a.src_img[17:17 + CHUNK]
    assert tuple(got[4]) == (int(shifted.sum()), int(np.argmax(shifted)), CHUNK, 0)
    assert tuple(got[5]) == tuple(want[5])
    a.check_unchanged("overlaps")
    a.free()


def test_graph_replay_starts_clean_every_time(gpu, oracle):
    """Captured once with 300 entries; between three replays the table's keys and offsets are rewritten and other mismatches planted
    -- the second replay has none: every replay's results and summary are that replay's alone."""
    a = Arena(gpu, oracle, 300, seed=77, small=True)
    t = a.table()
    tb, ws = resident(gpu, t)
    res = Results(gpu, 300)
    st = Stream()
    with Graph.capture(st) as g:
        gpu.verify_rekey_table_device(tb, res.ptr, ws, n=300, stream=st.handle)
    rng = np.random.default_rng(3)
    for k in range(3):
        a.draw_keys(rng)
        cl = [c for c, s in zip(a.classes(), a.sizes) if s]
        assert cl.count("two") >= 0.4 * len(cl) and "cancel" in cl
        a.remake()
        a.plant([] if k == 1 else [i for i in range(300) if i % 3 == k])
        tb.upload(a.table().view(np.uint8))
        g.launch(st)
        st.sync()
        assert gpu.table_status(ws) is None
        want = a.expected()
        same(res.read(("replay", k)), want, ("replay", k))
        assert gpu.verify_table_summary(ws) == summary_of(want), k
        assert (summary_of(want)["mismatches"] == 0) == (k == 1)
        a.check_unchanged(("replay", k))
    g.destroy()
    st.destroy()
    for b in (tb, ws, res, a):
        b.free()


def test_two_streams_two_workspaces(gpu, oracle):
    arenas = [Arena(gpu, oracle, 2000, seed=90 + i, small=True) for i in range(2)]
    streams = [Stream() for _ in arenas]
    rigs = []
    for k, a in enumerate(arenas):
        a.plant([i for i in range(2000) if i % 4 == k])
        tb, ws = resident(gpu, a.table())
        rigs.append((tb, ws, Results(gpu, 2000)))
    for (tb, ws, res), st in zip(rigs, streams):
        gpu.verify_rekey_table_device(tb, res.ptr, ws, n=2000, stream=st.handle)
    for a, (tb, ws, res), st in zip(arenas, rigs, streams):
        st.sync()
        assert gpu.table_status(ws) is None
        want = a.expected()
        same(res.read("two streams"), want, "two streams")
        assert gpu.verify_table_summary(ws) == summary_of(want)
        a.check_unchanged("two streams")
        for b in (tb, ws, res, a):
            b.free()
        st.destroy()


def test_device_tier_refusal_writes_no_result(gpu, oracle):
    """Nonzero flags on entry 700 and nonzero reserved on entry 123 of 1000: the results array keeps its 0xA5, the status names 123,
    the summary and the wrapper raise; after both fields are 0 the same workspace runs clean."""
    a = Arena(gpu, oracle, 1000, seed=11, small=True)
    a.plant(range(0, 1000, 5))
    t = a.table()
    t["flags"][700] = 1
    t["reserved"][123] = 2
    tb, ws = resident(gpu, t)
    res = Results(gpu, 1000)
    gpu.verify_rekey_table_device(tb, res.ptr, ws, n=1000)
    a.exp.sync()
    assert gpu.table_status(ws) == 123
    assert (res.read("refused").view(np.uint8) == 0xA5).all(), "a refused call wrote results"
    with pytest.raises(gpu.ModGpuError):
        gpu.verify_table_summary(ws)
    with pytest.raises(gpu.ModGpuError, match="entry 123"):
        gpu.verify_rekey_table_device(t)
    t["flags"] = 0
    t["reserved"] = 0
    tb.upload(t.view(np.uint8))
    run_resident(gpu, a, tb, ws, res, 1000, a.expected(), "fixed table")
    for b in (tb, ws, res, a):
        b.free()


def test_host_tier_queues_nothing(gpu, oracle):
    """A misaligned dev_results, a host pointer or NULL for dev_results, a workspace 8 bytes short or the rekey table call's (one line
    short): MODGPU_ERR_INVALID with gpu_launches unchanged; n_entries == 0 queues nothing."""
    a = Arena(gpu, oracle, 3, seed=2, sizes=[100, 200, 300])
    a.plant([1])
    tb, ws = resident(gpu, a.table())
    res = Results(gpu, 3)
    host = np.zeros(3 * 4, np.uint64)
    L = gpu.lib()
    wb = gpu.verify_rekey_table_workspace_bytes(3)
    before = gpu.path_stats()["gpu_launches"]
    assert L.modgpu_verify_rekey_table_device(tb.ptr, 3, res.ptr + 4, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(tb.ptr, 3, host.ctypes.data, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(tb.ptr, 3, None, ws.ptr, wb, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(tb.ptr, 3, res.ptr, ws.ptr, wb - 8, -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(tb.ptr, 3, res.ptr, ws.ptr, gpu.rekey_table_workspace_bytes(3), -1, None) == 1
    assert L.modgpu_verify_rekey_table_device(None, 0, None, None, 0, -1, None) == 0
    assert gpu.path_stats()["gpu_launches"] == before
    assert (res.read("tier 1").view(np.uint8) == 0xA5).all()
    assert len(gpu.verify_rekey_table_device(gpu.rekey_table(0))) == 0
    run_resident(gpu, a, tb, ws, res, 3, a.expected(), "after the refusals")
    for b in (tb, ws, res, a):
        b.free()


def test_entry_beyond_4_gib(gpu, oracle):
    """One entry of 2^32 + 77 bytes at odd phases, off_from near 2^64, the comparand made on the device by rekey_device_to from a
    tiled source: clean; then single bytes flipped by one-byte uploads at 2^32 - 1, 2^32 and n - 1 (3 mismatches, the first at
    2^32 - 1); the first restored: first_mismatch 2^32 (an index cut to 32 bits would read 0)."""
    n = (1 << 32) + 77
    src, exp = gpu.DeviceBuffer(n + 64), gpu.DeviceBuffer(n + 64)
    tile = np.random.default_rng(4).integers(0, 256, size=(1 << 24) + 13, dtype=np.uint8)
    for at in range(0, n + 64, tile.size):
        src.upload(tile[:min(tile.size, n + 64 - at)], offset=at)
    off_from, off_to = (1 << 64) - 12345, (1 << 33) + 5
    gpu.rekey_device_to(exp.ptr + 3, src.ptr + 9, PS3, PS4, off_from, off_to, n=n)
    exp.sync()
    t = gpu.rekey_table(1)
    t[0] = (exp.ptr + 3, src.ptr + 9, n, off_from, off_to, gpu.as_int32(PS3), gpu.as_int32(PS4), 0, 0)
    tb, ws = resident(gpu, t)
    res = Results(gpu, 1)

    def call():
        res.fill()
        gpu.verify_rekey_table_device(tb, res.ptr, ws, n=1)
        exp.sync()
        assert gpu.table_status(ws) is None
        r = res.read("big")[0]
        s = gpu.verify_table_summary(ws)
        assert s["mismatches"] == int(r["mismatches"]) and s["first_bad_entry"] == (0 if r["mismatches"] else None) and s["entries"] == 1
        return int(r["mismatches"]), int(r["first_mismatch"]), int(r["n"]), int(r["reserved"])

    def flip(j):
        b = exp.download(1, offset=3 + j)
        exp.upload(b ^ np.uint8(0x40), offset=3 + j)

    assert call() == (0, NONE, n, 0)
    for j in ((1 << 32) - 1, 1 << 32, n - 1):
        flip(j)
    assert call() == (3, (1 << 32) - 1, n, 0)
    flip((1 << 32) - 1)
    assert call() == (2, 1 << 32, n, 0)
    for b in (tb, ws, res, src, exp):
        b.free()
