"""GPU: the out-of-place, rekey and verify calls on ONE entry beyond 4 GiB -- n = 2^32 + 3 chunks + 77 bytes: whole chunks on both sides
of chunk index 65536 (the first non-zero index into the third chunk-jump table), a ragged last chunk, a tail of fewer than 16 bytes and,
at the phases used, a cut first chunk.  Entry indices, chunk offsets and a batch's chunk starts all pass 32 bits here.

The calls under test never judge themselves at this size.  Two independent instruments do:
  1. oracle windows: up to 1 MiB at entry index 0, across byte 2^32, across the chunk boundary behind it and at the end, read back through
     a SMALL out-of-place call under another key (one host copy of a window that crosses 4 GiB inside an allocation is refused by the
     runtime) and compared with oracle.cycle_at over the plaintext rebuilt from the host's tile;
  2. the whole buffer: undone in place by modgpu_cycle_device (oracle-checked up to 48 GiB in test_gpu_parity.py) and compared with the
     plaintext by modgpu_verify_batch_device under key 0 in slices of at most 1 GiB (the sizes test_gpu_verify.py covers).
The plaintext is a seeded tile of 16 MiB + 13 bytes repeated: periodic in no whole number of chunks, so an addressing error of any whole
number of chunks shows.  All expectations are exact.

Buffers: the plaintext P is n + 64 bytes and each arena n + 128 bytes, plus ROOM (six chunks) behind both -- the small entries of the
two batch tests lie BEHIND the big entry, and 64 / 128 bytes do not hold them.  The window at 2^32 + CHUNK - 4096 is cut at the entry's
end (n lies 2 chunks + 4173 bytes behind it).  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte and every
number compared here came from a kernel."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
READ_KEY = 12345  # the key windows are read back under
CHUNK = 65536
PERIOD = 0x7FFFFFFE
NONE = 0xFFFFFFFFFFFFFFFF
BAND = 4096
N = (1 << 32) + 3 * CHUNK + 77
ROOM = 6 * CHUNK
P_LEN = N + 64 + ROOM
ARENA_LEN = N + 128 + ROOM
TILE = (16 << 20) + 13
WIN = 1 << 20
WINDOWS = (0, (1 << 32) - WIN + 50, (1 << 32) + CHUNK - 4096, N - WIN)  # the second straddles byte 2^32, the third the chunk edge behind it
SLICE = 1 << 30
OFF = (1 << 64) - 12345


def triple(r):
    assert int(r["reserved"]) == 0
    return int(r["mismatches"]), int(r["first_mismatch"]), int(r["n"])


class Shared:
    """The plaintext P (device; its tile on the host), two arenas, a window's scratch and a result buffer, made once for the module."""

    def __init__(self, M, oracle):
        self.M, self.oracle = M, oracle
        self.tile = np.random.default_rng(4).integers(0, 256, size=TILE, dtype=np.uint8)
        self.P = M.DeviceBuffer(P_LEN)
        for at in range(0, P_LEN, TILE):
            self.P.upload(self.tile[:min(TILE, P_LEN - at)], offset=at)
        self.arena, self.arena2 = M.DeviceBuffer(ARENA_LEN), M.DeviceBuffer(ARENA_LEN)
        self.tmp = M.DeviceBuffer(WIN)
        self.res = M.DeviceBuffer(2 * BAND + 32 * 8)
        self.seed = np.full(16 << 20, 0x5A, np.uint8)

    def plain(self, at, size):
        """P[at : at + size], rebuilt on the host"""
        return np.take(self.tile, np.arange(at, at + size) % TILE)

    def fill(self, buf):
        """0x5A everywhere: one 16 MiB upload, then doubled by key-0 out-of-place calls (copies) of at most 2 GiB"""
        buf.upload(self.seed)
        done = self.seed.size
        while done < buf.nbytes:
            c = min(done, buf.nbytes - done, 2 << 30)
            self.M.cycle_device_to(buf.ptr + done, buf.ptr, c, 0, 0)
            done += c
        buf.sync()

    def copy(self, dst, src, size):
        """a plain copy in slices of at most 1 GiB (key 0: the identity keystream)"""
        for at in range(0, size, SLICE):
            self.M.cycle_device_to(dst + at, src + at, min(SLICE, size - at), 0, 0)

    def window(self, ptr, size):
        """`size` (<= 1 MiB) device bytes at any address, through a small out-of-place call under another key and the oracle"""
        self.M.cycle_device_to(self.tmp.ptr, ptr, size, READ_KEY, 0)
        self.tmp.sync()
        return self.oracle.cycle_at(self.tmp.download(size), READ_KEY, 0)

    def check_windows(self, ptr, src_at, key, off, what):
        """instrument 1: the entry at `ptr` must be P[src_at : src_at + N] under (key, off)"""
        for m in WINDOWS:
            size = min(WIN, N - m)
            got = self.window(ptr + m, size)
            want = self.plain(src_at + m, size)
            self.oracle.cycle_at(want, key, off % PERIOD + m)  # (positions are off + j, reduced mod the period, never mod 2^64)
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError(f"{what}: window at entry index {m}: {bad.size} bytes differ, first at entry index {m + int(bad[0])}")

    def compare(self, expect, src, size=N):
        """the triples of a key-0 verify (a plain compare) of [expect, expect + size) with [src, src + size), per slice of <= 1 GiB"""
        ats = list(range(0, size, SLICE))
        sizes = [min(SLICE, size - at) for at in ats]
        self.M.verify_batch_device([expect + at for at in ats], [src + at for at in ats], sizes, 0, self.res.ptr + BAND)
        self.res.sync()
        return [triple(r) for r in self.M.verify_results(self.res.ptr + BAND, len(ats))], [(0, NONE, s) for s in sizes]

    def check_whole(self, ptr, src_at, key, off, what, reapply=False):
        """instrument 2: undo the entry at `ptr` in place and compare all of it with P[src_at : src_at + N]"""
        self.M.cycle_device(ptr, N, key, off)
        got, clean = self.compare(ptr, self.P.ptr + src_at)
        assert got == clean, (what, got)
        if reapply:
            self.M.cycle_device(ptr, N, key, off)

    def check_guards(self, buf, at, what, size=N):
        """every byte of `buf` in front of and behind [at, at + size) is still 0x5A"""
        assert (buf.download(at, offset=0) == 0x5A).all(), (what, "bytes in front of the entry")
        assert (buf.download(buf.nbytes - at - size, offset=at + size) == 0x5A).all(), (what, "bytes behind the entry")

    def cipher_of_p(self, buf, at, src_at, key, off):
        """buf[at : at + N] := P[src_at : src_at + N] under (key, off), by calls checked elsewhere at their sizes: copies, then in place"""
        self.copy(buf.ptr + at, self.P.ptr + src_at, N)
        self.M.cycle_device(buf.ptr + at, N, key, off)
        buf.sync()

    def free(self):
        for b in (self.P, self.arena, self.arena2, self.tmp, self.res):
            b.free()


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


@pytest.fixture(scope="module")
def shared(gpu, oracle):
    s = Shared(gpu, oracle)
    yield s
    s.free()


def flip(buf, at):
    buf.upload(buf.download(1, offset=at) ^ 0x01, offset=at)


def test_cycle_to_beyond_4gib(gpu, oracle, shared):
    """modgpu_cycle_device_to over the whole entry at an offset near 2^64: the funnel read ((src - dst) mod 4 = 2) and the plain read, both
    with a cut first chunk.  Windows against the oracle, the whole buffer undone and compared, the guard bytes, the launch's byte count."""
    s = shared
    for k, (pd, ps) in enumerate(((3, 9), (3, 7))):
        what = ("cycle_to", pd, ps)
        s.fill(s.arena)
        gpu.cycle_device_to(s.arena.ptr + pd, s.P.ptr + ps, N, PS3, OFF)
        s.arena.sync()
        info = gpu.last_launch()
        assert info["variant"] == 5 and info["bytes"] == N and info["source_hash"] == gpu.to_kernel_source_hash(), info
        assert ("true" in info["kernel"]) == ((ps - pd) % 4 != 0), info
        s.check_guards(s.arena, pd, what)
        s.check_windows(s.arena.ptr + pd, ps, PS3, OFF, what)
        if k == 0:  # the compare is no rubber stamp: ciphertext against plaintext differs wherever the keystream byte is non-zero
            got, clean = s.compare(s.arena.ptr + pd, s.P.ptr + ps)
            assert all(g[0] > 0.99 * c[2] and g[1] < 4096 and g[2] == c[2] for g, c in zip(got, clean)), got
        s.check_whole(s.arena.ptr + pd, ps, PS3, OFF, what)
        s.check_guards(s.arena, pd, what)


def test_batch_to_with_an_entry_beyond_4gib(gpu, oracle, shared):
    """One modgpu_cycle_batch_device_to call: the big entry, then 17, CHUNK - 1, 3 * CHUNK + 5 and 0 bytes at odd phases with offsets of
    their own, sources beyond byte 2^32 of P (two inside the big entry's source, one behind it), destinations behind the big one.  In a
    shared launch the small entries' chunk starts lie beyond 65535.  The small entries and every gap whole, the big entry by windows."""
    s = shared
    sizes = [N, 17, CHUNK - 1, 3 * CHUNK + 5, 0]
    src_at = [9, (1 << 32) + 1, (1 << 32) + CHUNK + 6, N + 9 + 7, (1 << 32) + 2]
    offs = [OFF, 5, (1 << 63) + 11, (1 << 32) - 17, 99]
    dst_at, cur = [], 3
    for size, gap in zip(sizes, (0, 5, 11, 7, 3)):
        cur += gap
        dst_at.append(cur)
        cur += size
    assert cur <= ARENA_LEN and all(a + z <= P_LEN for a, z in zip(src_at, sizes))
    s.fill(s.arena)
    gpu.cycle_batch_device_to([s.arena.ptr + a for a in dst_at], [s.P.ptr + a for a in src_at], sizes, PS3, stream_offs=offs)
    s.arena.sync()
    behind = N + 3
    want = np.full(ARENA_LEN - behind, 0x5A, np.uint8)
    for a, q, z, o in list(zip(dst_at, src_at, sizes, offs))[1:4]:
        want[a - behind:a - behind + z] = oracle.cycle_at(s.plain(q, z), PS3, o)
    got = s.arena.download(ARENA_LEN - behind, offset=behind)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"behind the big entry: {bad.size} bytes differ, first at arena offset {behind + int(bad[0])}; entries at {dst_at}")
    assert (s.arena.download(3) == 0x5A).all(), "bytes in front of the big entry"
    s.check_windows(s.arena.ptr + 3, 9, PS3, OFF, "batch entry 0")


def test_rekey_beyond_4gib(gpu, oracle, shared):
    """modgpu_rekey_device_to of P under (PS3, 2^63 + 11) to (PS4, 2^32 - 17), funnel read with a cut first chunk: the shipped library,
    then both launch shapes of the testing flavour.  Windows against the oracle under the new key alone, the whole buffer undone under
    the new key and compared with P, the guard bytes; the source still decrypts to P under the old key."""
    s = shared
    ps, off_from, off_to = 9, (1 << 63) + 11, (1 << 32) - 17
    s.fill(s.arena)
    s.cipher_of_p(s.arena, 3, ps, PS3, off_from)

    def run(what):
        s.fill(s.arena2)
        gpu.rekey_device_to(s.arena2.ptr + 5, s.arena.ptr + 3, PS3, PS4, off_from, off_to, n=N)
        s.arena2.sync()
        info = gpu.last_launch()
        assert info["variant"] == 7 and info["bytes"] == N and "true" in info["kernel"], info
        s.check_guards(s.arena2, 5, what)
        s.check_windows(s.arena2.ptr + 5, ps, PS4, off_to, what)
        s.check_whole(s.arena2.ptr + 5, ps, PS4, off_to, what)
        return info["grid"]

    run("rekey, shipped")
    with gpu.testing_flavour():
        grids = {}
        try:
            for form in ("queue", "all"):
                gpu.debug_set_rekey_form(form)
                grids[form] = run(("rekey", form))
        finally:
            gpu.debug_set_rekey_form(None)
        assert grids["queue"] < grids["all"], grids
    s.check_whole(s.arena.ptr + 3, ps, PS3, off_from, "the rekey's source")
    s.check_guards(s.arena, 3, "the rekey's source")


class VerifyRig:
    """One modgpu_verify_device call over the big entry, as Rig.call of test_gpu_verify.py: a 0xEE result between two 4 KiB bands."""

    def __init__(self, s):
        self.s, self.M = s, s.M
        self.rb = s.M.DeviceBuffer(2 * BAND + 32)

    def call(self, expect, src, key, off):
        M = self.M
        self.rb.upload(np.full(2 * BAND + 32, 0xEE, np.uint8))
        before = M.path_stats()["gpu_launches"]
        M.verify_device(expect, src, key, off, result=self.rb.ptr + BAND, n=N)
        self.rb.sync()
        assert M.path_stats()["gpu_launches"] - before == 2
        got = self.rb.download()
        assert (got[:BAND] == 0xEE).all() and (got[BAND + 32:] == 0xEE).all(), "the bands around the result were written"
        assert np.array_equal(got[BAND:BAND + 32], M.verify_results(self.rb.ptr + BAND)[0:1].view(np.uint8))
        return triple(got[BAND:BAND + 32].view(M.VERIFY_RESULT_DTYPE)[0])


def test_verify_beyond_4gib(gpu, oracle, shared):
    """modgpu_verify_device with expect = P under (PS4, off), made in place: clean, then bytes of expect flipped at entry indices
    2^32 - 1, 2^32, 2^32 + CHUNK + 5 and n - 1 and restored one by one from the lowest (first_mismatch cut to 32 bits would read 0
    at the second step), a byte of src flipped, everything restored.  Plain and funnel read.  One step also on three workgroups
    (testing flavour), each walking some 21 800 chunks of the one entry with its count in registers."""
    s = shared
    rig = VerifyRig(s)
    J = [(1 << 32) - 1, 1 << 32, (1 << 32) + CHUNK + 5, N - 1]
    src_j = (1 << 32) + 7
    for pe, ps in ((0, 0), (6, 1)):
        s.cipher_of_p(s.arena, pe, ps, PS4, OFF)
        e, p = s.arena.ptr + pe, s.P.ptr + ps

        def call():
            return rig.call(e, p, PS4, OFF)

        assert call() == (0, NONE, N), (pe, ps)
        info = gpu.last_launch()
        assert info["variant"] == 10 and info["bytes"] == N and info["source_hash"] == gpu.verify_kernel_source_hash(), info
        assert info["kernel"].startswith("modgpu_cycle_verify_kernel<4, 1024, " + ("true" if (ps - pe) % 4 else "false") + ", true>"), info
        for j in J:
            flip(s.arena, pe + j)
        assert call() == (4, J[0], N), (pe, ps)
        flip(s.arena, pe + J[0])
        assert call() == (3, J[1], N), (pe, ps)
        if pe:
            with gpu.testing_flavour():
                try:
                    gpu.debug_set_verify_form(3)
                    assert call() == (3, J[1], N), (pe, ps, "three workgroups")
                    assert gpu.last_launch()["grid"] == 3
                finally:
                    gpu.debug_set_verify_form(0)
        flip(s.arena, pe + J[1])
        assert call() == (2, J[2], N), (pe, ps)
        flip(s.arena, pe + J[2])
        assert call() == (1, J[3], N), (pe, ps)  # (in the ragged tail)
        flip(s.P, ps + src_j)
        assert call() == (2, src_j, N), (pe, ps)
        flip(s.P, ps + src_j)
        flip(s.arena, pe + J[3])
        assert call() == (0, NONE, N), (pe, ps)
        assert np.array_equal(s.P.download(16, offset=ps + src_j - 8), s.plain(ps + src_j - 8, 16)), "P was not restored"
    rig.rb.free()


def test_verify_batch_with_an_entry_beyond_4gib(gpu, oracle, shared):
    """One modgpu_verify_batch_device call: the big entry with flips at 2^32 + 1 and n - 2, then 1, CHUNK + 1 and 2 * CHUNK + 3 bytes
    behind it in both buffers with offsets of their own, the last with a flip at its last byte.  Every triple exact; two launches."""
    s = shared
    pe, ps = 6, 1
    sizes = [N, 1, CHUNK + 1, 2 * CHUNK + 3]
    offs = [OFF, (1 << 32) + 5, (1 << 63) - 9, 7]
    e_at, s_at, ce, cs = [], [], pe, ps
    for size, ge, gs in zip(sizes, (0, 3, 9, 6), (0, 4, 1, 11)):
        ce, cs = ce + ge, cs + gs
        e_at.append(ce)
        s_at.append(cs)
        ce, cs = ce + size, cs + size
    assert ce <= ARENA_LEN and cs <= P_LEN
    s.cipher_of_p(s.arena, pe, ps, PS4, OFF)
    for a, q, z, o in list(zip(e_at, s_at, sizes, offs))[1:]:
        s.arena.upload(oracle.cycle_at(s.plain(q, z), PS4, o), offset=a)
    flips = [e_at[0] + (1 << 32) + 1, e_at[0] + N - 2, e_at[3] + sizes[3] - 1]
    want = [(2, (1 << 32) + 1, N), (0, NONE, 1), (0, NONE, CHUNK + 1), (1, sizes[3] - 1, sizes[3])]
    for at in flips:
        flip(s.arena, at)
    res = s.res.ptr + BAND
    s.res.upload(np.full(s.res.nbytes, 0xEE, np.uint8))
    before = gpu.path_stats()["gpu_launches"]
    gpu.verify_batch_device([s.arena.ptr + a for a in e_at], [s.P.ptr + q for q in s_at], sizes, PS4, res, stream_offs=offs)
    s.res.sync()
    assert gpu.path_stats()["gpu_launches"] - before == 1 + math.ceil(len(sizes) / 16) == 2
    assert [triple(r) for r in gpu.verify_results(res, len(sizes))] == want
    got = s.res.download()
    assert (got[:BAND] == 0xEE).all() and (got[BAND + 32 * len(sizes):] == 0xEE).all(), "bytes around the results were written"
    for at in flips:
        flip(s.arena, at)
    gpu.verify_batch_device([s.arena.ptr + a for a in e_at], [s.P.ptr + q for q in s_at], sizes, PS4, res, stream_offs=offs)
    s.res.sync()
    assert [triple(r) for r in gpu.verify_results(res, len(sizes))] == [(0, NONE, z) for z in sizes]
