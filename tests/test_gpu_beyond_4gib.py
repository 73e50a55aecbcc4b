"""GPU: the out-of-place, rekey, verify and rekey verify calls (single and batch), the move call (modgpu_rekey_move_device) and the move
table call (modgpu_rekey_move_table_device) on ONE entry beyond 4 GiB -- n = 2^32 + 3 chunks + 77 bytes: whole chunks on both sides
of chunk index 65536 (the first non-zero index into the third chunk-jump table), a ragged last chunk, a tail of fewer than 16 bytes and,
at the phases used, a cut first chunk.  Entry indices, chunk offsets, a batch's chunk starts and a move's flags, windows and tickets
all pass 32 bits (or chunk 65535) here; the last test makes a mismatch COUNT pass 2^32 in one entry.  Every streaming kernel TU keeps
its own copy of this arithmetic, so each call has a test of its own.

The calls under test never judge themselves at this size.  Two independent instruments do:
  1. oracle windows: up to 1 MiB at entry index 0, across byte 2^32, across the chunk boundary behind it and at the end, read back through
     a SMALL out-of-place call under another key (one host copy of a window that crosses 4 GiB inside an allocation is refused by the
     runtime) and compared with oracle.cycle_at over the plaintext rebuilt from the host's tile;
  2. the whole buffer: undone in place by modgpu_cycle_device (oracle-checked up to 48 GiB in test_gpu_parity.py) and compared with the
     plaintext by modgpu_verify_batch_device under key 0 in slices of at most 1 GiB (the sizes test_gpu_verify.py covers).
The plaintext is a seeded tile of 16 MiB + 13 bytes repeated: periodic in no whole number of chunks, so an addressing error of any whole
number of chunks shows.  All expectations are exact.  What a test reads is built only from calls pinned at this size elsewhere: copies
under key 0 in slices, the in-place modgpu_cycle_device and small uploads of the oracle's bytes -- never from modgpu_rekey_device_to
or from a move call.

Buffers: the plaintext P is n + 64 bytes and each arena n + 128 bytes, plus ROOM (six chunks) behind both -- the small entries of the
batch and table tests lie BEHIND the big entry, a move's source and destination lie up to 3 chunks + 4 bytes apart in ONE arena, and
64 / 128 bytes do not hold them.  The window at 2^32 + CHUNK - 4096 is cut at the entry's
end (n lies 2 chunks + 4173 bytes behind it).  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library loads, so every byte and every
number compared here came from a kernel."""
import math
import time

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

    def fill(self, buf, byte=0x5A):
        """`byte` everywhere: one 16 MiB upload, then doubled by key-0 out-of-place calls (copies) of at most 2 GiB"""
        buf.upload(self.seed if byte == 0x5A else np.full(self.seed.size, byte, np.uint8))
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


OFF_FROM, OFF_TO = (1 << 63) + 11, (1 << 32) - 17  # (their residues mod the period lie 5 and 15 below it: both streams wrap inside the entry)


def under(oracle, data, key, off, at=0):
    """`data` (changed in place and returned) as bytes at, at + 1, ... of an entry under (key, off), by the oracle"""
    return oracle.cycle_at(data, key, off % PERIOD + at)


def rekeyed(oracle, data, key_from, off_from, key_to, off_to, at=0):
    """what a rekey makes of a copy of `data`, bytes at, at + 1, ... of an entry, by the oracle: two passes of the cipher on the CPU"""
    return under(oracle, under(oracle, data.copy(), key_from, off_from, at), key_to, off_to, at)


class VerifyRekeyRig(VerifyRig):
    """One modgpu_verify_rekey_device call over the big entry, as Rig.call of test_gpu_verify_rekey.py: a 0xEE result between two 4 KiB
    bands, two launches (the result's initialisation and one compare launch: the two keystreams differ)."""

    def call(self, expect, src, keys, offs):
        M = self.M
        self.rb.upload(np.full(2 * BAND + 32, 0xEE, np.uint8))
        before = M.path_stats()["gpu_launches"]
        M.verify_rekey_device(expect, src, keys[0], keys[1], offs[0], offs[1], result=self.rb.ptr + BAND, n=N)
        self.rb.sync()
        assert M.path_stats()["gpu_launches"] - before == 2
        got = self.rb.download()
        assert (got[:BAND] == 0xEE).all() and (got[BAND + 32:] == 0xEE).all(), "the bands around the result were written"
        assert np.array_equal(got[BAND:BAND + 32], M.verify_results(self.rb.ptr + BAND)[0:1].view(np.uint8))
        return triple(got[BAND:BAND + 32].view(M.VERIFY_RESULT_DTYPE)[0])


def test_verify_rekey_beyond_4gib(gpu, oracle, shared):
    """modgpu_verify_rekey_device as test_verify_beyond_4gib: src = P under (PS3, 2^63 + 11) and expect = P under (PS4, 2^64 - 12345),
    both made in place (never by a rekey call): clean, then bytes of expect flipped at entry indices 2^32 - 1, 2^32, 2^32 + CHUNK + 5
    and n - 1 and restored one by one from the lowest (first_mismatch cut to 32 bits would read 0 at the second step), a byte of src
    flipped, everything restored; at the end both buffers undone in place and compared with P.  Plain and funnel read, the second with
    a cut first chunk.  One step also on three workgroups (modgpu_debug_set_verify_form bounds this call's grid too, as in
    test_gpu_verify_rekey.py), each walking some 21 800 chunks of the one entry with its count in registers."""
    s = shared
    rig = VerifyRekeyRig(s)
    keys, offs = (PS3, PS4), (OFF_FROM, OFF)
    J = [(1 << 32) - 1, 1 << 32, (1 << 32) + CHUNK + 5, N - 1]
    src_j = (1 << 32) + 7
    for pe, ps in ((0, 0), (6, 1)):
        q = 9 * ps  # where the entry starts in P
        s.cipher_of_p(s.arena, ps, q, PS3, OFF_FROM)
        s.cipher_of_p(s.arena2, pe, q, PS4, OFF)
        e, p = s.arena2.ptr + pe, s.arena.ptr + ps

        def call():
            return rig.call(e, p, keys, offs)

        assert call() == (0, NONE, N), (pe, ps)
        info = gpu.last_launch()
        assert info["variant"] == 12 and info["bytes"] == N and info["source_hash"] == gpu.rekey_verify_kernel_source_hash(), info
        assert info["kernel"] == "modgpu_cycle_rekey_verify_kernel<4, 1024, " + ("true" if (ps - pe) % 4 else "false") + ">", info
        for j in J:
            flip(s.arena2, pe + j)
        assert call() == (4, J[0], N), (pe, ps)
        flip(s.arena2, pe + J[0])
        assert call() == (3, J[1], N), (pe, ps)
        if pe:
            with gpu.testing_flavour():
                try:
                    gpu.debug_set_verify_form(3)
                    assert call() == (3, J[1], N), (pe, ps, "three workgroups")
                    assert gpu.last_launch()["grid"] == 3 and gpu.last_launch()["variant"] == 12
                finally:
                    gpu.debug_set_verify_form(0)
        flip(s.arena2, pe + J[1])
        assert call() == (2, J[2], N), (pe, ps)
        flip(s.arena2, pe + J[2])
        assert call() == (1, J[3], N), (pe, ps)  # (in the ragged tail)
        flip(s.arena, ps + src_j)
        assert call() == (2, src_j, N), (pe, ps)
        flip(s.arena, ps + src_j)
        flip(s.arena2, pe + J[3])
        assert call() == (0, NONE, N), (pe, ps)
        s.check_whole(p, q, PS3, OFF_FROM, ("the rekey verify's src", pe, ps))
        s.check_whole(e, q, PS4, OFF, ("the rekey verify's expect", pe, ps))
    rig.rb.free()


def test_verify_rekey_batch_with_an_entry_beyond_4gib(gpu, oracle, shared):
    """One modgpu_verify_rekey_batch_device call, as test_verify_batch_with_an_entry_beyond_4gib: the big entry (src and expect made in
    place) with flips at 2^32 + 1 and n - 2, then 1, CHUNK + 1 and 2 * CHUNK + 3 bytes behind it in both buffers with offsets of
    their own on both sides -- their sources bytes of P, their expect bytes the oracle's, uploaded --, the last with a flip at its last
    byte.  In the shared launch the small entries' chunk starts lie beyond 65535.  Every triple exact; two launches."""
    s = shared
    pe, ps, q = 6, 1, 9
    sizes = [N, 1, CHUNK + 1, 2 * CHUNK + 3]
    offs_from = [OFF_FROM, (1 << 32) + 5, (1 << 63) - 9, 7]
    offs_to = [OFF, 5, (1 << 64) - 3, OFF_TO]
    e_at, s_at, ce, cs = [], [], pe, ps
    for size, ge, gs in zip(sizes, (0, 3, 9, 6), (0, 4, 1, 11)):
        ce, cs = ce + ge, cs + gs
        e_at.append(ce)
        s_at.append(cs)
        ce, cs = ce + size, cs + size
    assert ce <= ARENA_LEN and cs <= ARENA_LEN
    s.cipher_of_p(s.arena, ps, q, PS3, offs_from[0])
    s.cipher_of_p(s.arena2, pe, q, PS4, offs_to[0])
    for i in (1, 2, 3):
        data = s.plain(N + 100 * i, sizes[i])
        s.arena.upload(data, offset=s_at[i])
        s.arena2.upload(rekeyed(oracle, data, PS3, offs_from[i], PS4, offs_to[i]), offset=e_at[i])
    flips = [e_at[0] + (1 << 32) + 1, e_at[0] + N - 2, e_at[3] + sizes[3] - 1]
    want = [(2, (1 << 32) + 1, N), (0, NONE, 1), (0, NONE, CHUNK + 1), (1, sizes[3] - 1, sizes[3])]
    for at in flips:
        flip(s.arena2, at)
    res = s.res.ptr + BAND
    s.res.upload(np.full(s.res.nbytes, 0xEE, np.uint8))
    e_ptrs, s_ptrs = [s.arena2.ptr + a for a in e_at], [s.arena.ptr + a for a in s_at]
    before = gpu.path_stats()["gpu_launches"]
    gpu.verify_rekey_batch_device(e_ptrs, s_ptrs, sizes, PS3, PS4, res, offs_from=offs_from, offs_to=offs_to)
    s.res.sync()
    assert gpu.path_stats()["gpu_launches"] - before == 1 + math.ceil(len(sizes) / 16) == 2
    assert gpu.last_launch()["variant"] == 12 and gpu.last_launch()["source_hash"] == gpu.rekey_verify_kernel_source_hash()
    assert [triple(r) for r in gpu.verify_results(res, len(sizes))] == want
    got = s.res.download()
    assert (got[:BAND] == 0xEE).all() and (got[BAND + 32 * len(sizes):] == 0xEE).all(), "bytes around the results were written"
    for at in flips:
        flip(s.arena2, at)
    gpu.verify_rekey_batch_device(e_ptrs, s_ptrs, sizes, PS3, PS4, res, offs_from=offs_from, offs_to=offs_to)
    s.res.sync()
    assert [triple(r) for r in gpu.verify_results(res, len(sizes))] == [(0, NONE, z) for z in sizes]


def test_rekey_move_beyond_4gib(gpu, oracle, shared):
    """modgpu_rekey_move_device of the big entry inside ONE arena, source and destination d bytes apart: d = 65537 down and up (the
    funnel; every chunk waits for two others, upward with positions walking from the top), 3 chunks + 4 down (the plain form, a window
    three chunks away), 5 up (a sub-chunk shift), and the compaction pair PS4 -> PS4 with off_to = off_from - d.  The destination
    lies 3 bytes past a chunk boundary: the head goes through scratch, and so does the tail, which lies at head + body beyond 2^32.
    The source is P under (key_from, 2^63 + 11), made in place.  After ONE call: the status, the launch, the d source bytes the
    destination does not cover (the oracle's), 0x5A everywhere around both ranges, then the windows against the oracle under the new
    key alone and the whole destination undone in place and compared with P.  Flags, tickets and the last window's chunks all pass
    65535 (test_gpu_rekey_move.py has the matrix of shifts, phases and keys up to 48 MiB)."""
    s = shared
    ps = 9
    ws = gpu.DeviceBuffer(gpu.move_workspace_bytes(N))
    cases = [(65537, False, PS3, PS4, OFF_TO), (65537, True, PS3, PS4, OFF_TO), (3 * CHUNK + 4, False, PS3, PS4, OFF_TO), (5, True, PS3, PS4, OFF_TO),
             (65537, False, PS4, PS4, OFF_FROM - 65537)]
    try:
        for d, up, kf, kt, off_to in cases:
            what = ("move", d, "up" if up else "down", hex(kf), hex(kt))
            t0 = time.perf_counter()
            dst = (3 - s.arena.ptr) % CHUNK
            while dst - (d if up else 0) < 3:
                dst += CHUNK
            src = dst - d if up else dst + d
            lo = min(dst, src)
            assert (s.arena.ptr + dst) % CHUNK == 3 and lo >= 3 and lo + N + d + 64 <= ARENA_LEN
            s.fill(s.arena)
            s.cipher_of_p(s.arena, src, ps, kf, OFF_FROM)
            gpu.rekey_move_device(s.arena.ptr + dst, s.arena.ptr + src, N, kf, kt, OFF_FROM, off_to, ws)
            s.arena.sync()
            info = gpu.last_launch()
            assert gpu.move_status(ws) is None, what
            assert info["variant"] == 14 and info["bytes"] == N and info["source_hash"] == gpu.rekey_kernel_source_hash(), info
            assert ("true" in info["kernel"]) == (d % 4 != 0), info
            # the source bytes the destination does not cover: entry indices [0, d) in front of it, or [n - d, n) behind it
            j0 = 0 if up else N - d
            rest = s.arena.download(d, offset=src + j0)
            assert np.array_equal(rest, under(oracle, s.plain(ps + j0, d), kf, OFF_FROM, j0)), (what, "source bytes outside the destination")
            s.check_guards(s.arena, lo, what, size=N + d)
            s.check_windows(s.arena.ptr + dst, ps, kt, off_to, what)
            s.check_whole(s.arena.ptr + dst, ps, kt, off_to, what)
            print(what, f"{time.perf_counter() - t0:.3f} s")  # (fill, build, call, windows, undo and compare: as a case of test_rekey_beyond_4gib)
    finally:
        ws.free()


def test_rekey_move_table_with_an_entry_beyond_4gib(gpu, oracle, shared):
    """One modgpu_rekey_move_table_device call in ONE arena: the big entry, then 17, CHUNK - 1, 3 * CHUNK + 5 and 0 bytes, every entry
    with offsets of its own, two pairs of keys in turn.  Downward the sources lie 5, 65537, 11 and 7 bytes further apart than the
    destinations and the move closes the gaps; upward (the mirror image, positions in reverse: the big entry's chunk 65536 is an early
    one) it opens them.  The big source is P made in place, the small ones the oracle's bytes, uploaded.  All global chunk numbers
    behind the big entry pass 65535.  Everything behind the big entry's packed end (under 1 MiB) is compared whole with the host
    model of test_gpu_rekey_move_table.py (Arena.model: each entry applied to the memory as the call found it), the big entry by
    windows and undone whole, the bytes in front by value.  The downward table at the shipped grid and, in the testing flavour, on
    four workgroups that draw some 16 000 tickets each and wait across entries; the upward one at the shipped grid."""
    s = shared
    ps = 9
    sizes = [N, 17, CHUNK - 1, 3 * CHUNK + 5, 0]
    gaps = [5, 65537, 11, 7, 0]
    q_at = [ps, (1 << 32) + 1, (1 << 32) + CHUNK + 6, N + 9 + 7, (1 << 32) + 2]  # where each entry's plaintext lies in P
    keys = [(PS3, PS4), (PS4, PS4), (PS3, PS4), (PS4, PS4), (PS3, PS4)]
    offs_from = [OFF_FROM, 5, (1 << 63) - 9, (1 << 32) + 5, 99]
    offs_to = [OFF_TO, (1 << 64) - 3, 7, OFF, 3]
    total = sum(sizes)
    lo = (3 - s.arena.ptr) % CHUNK  # the packed side starts 3 bytes past a chunk boundary: the big entry's first chunk is cut
    behind = lo + N                 # the end of the big entry's packed range: everything from here on is compared whole
    packed, spread, at_p, at_s = [], [], lo, lo
    for z, g in zip(sizes, gaps):
        at_s += g
        packed.append(at_p)
        spread.append(at_s)
        at_p, at_s = at_p + z, at_s + z
    assert lo >= 3 and at_s + 64 <= ARENA_LEN and all(a + z <= P_LEN for a, z in zip(q_at, sizes))
    table = gpu.DeviceBuffer(len(sizes) * 56)
    ws = gpu.DeviceBuffer(gpu.rekey_move_table_workspace_bytes(len(sizes), total))

    def run(down, grid, what):
        dst_at, src_at = (packed, spread) if down else (spread, packed)
        t0 = time.perf_counter()
        s.fill(s.arena)
        s.cipher_of_p(s.arena, src_at[0], ps, PS3, OFF_FROM)
        # the memory behind the big entry's packed end as the call finds it: downward the last 5 bytes of the big source, the small
        # sources, 0x5A between and behind them
        img = np.full(ARENA_LEN - behind, 0x5A, np.uint8)
        if down:
            img[:gaps[0]] = under(oracle, s.plain(ps + N - gaps[0], gaps[0]), PS3, OFF_FROM, N - gaps[0])
        for i in (1, 2, 3):
            data = under(oracle, s.plain(q_at[i], sizes[i]), keys[i][0], offs_from[i])
            s.arena.upload(data, offset=src_at[i])
            img[src_at[i] - behind:src_at[i] - behind + sizes[i]] = data
        assert np.array_equal(s.arena.download(img.size, offset=behind), img), (what, "the test's own picture of the memory before the call")
        want = img.copy()
        for i in (1, 2, 3):
            a, b, z = dst_at[i] - behind, src_at[i] - behind, sizes[i]
            want[a:a + z] = rekeyed(oracle, img[b:b + z], keys[i][0], offs_from[i], keys[i][1], offs_to[i])
        if not down:  # the last 5 bytes of the big destination
            want[:gaps[0]] = under(oracle, s.plain(ps + N - gaps[0], gaps[0]), PS4, OFF_TO, N - gaps[0])
        t = gpu.rekey_table(len(sizes))
        for i, z in enumerate(sizes):
            t[i]["dst"], t[i]["src"], t[i]["n"] = s.arena.ptr + dst_at[i], s.arena.ptr + src_at[i], z
            t[i]["off_from"], t[i]["off_to"] = offs_from[i], offs_to[i]
            t[i]["key_from"], t[i]["key_to"] = gpu.as_int32(keys[i][0]), gpu.as_int32(keys[i][1])
        gpu.rekey_move_table_validate(t)
        table.upload(t.view(np.uint8))
        before = gpu.path_stats()["gpu_launches"]
        gpu.rekey_move_table_device(table, total, ws, n=len(sizes))
        s.arena.sync()
        assert gpu.path_stats()["gpu_launches"] - before == 5, what
        info = gpu.last_launch()
        assert gpu.rekey_move_table_status(ws) == (None, None), what
        assert gpu.table_status(ws) is None, what
        assert info["variant"] == 15 and info["source_hash"] == gpu.rekey_move_table_kernel_source_hash(), info
        assert info["grid"] == grid if grid else 4 < info["grid"] <= 256, info
        got = s.arena.download(img.size, offset=behind)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what}: behind the big entry: {bad.size} bytes differ, first at arena offset {behind + int(bad[0])}; "
                                 f"destinations at {dst_at}, sources at {src_at}")
        assert (s.arena.download(lo) == 0x5A).all(), (what, "bytes in front of the big entry")
        if not down:  # the first 5 bytes of the big source are not covered by its destination
            assert np.array_equal(s.arena.download(gaps[0], offset=lo), under(oracle, s.plain(ps, gaps[0]), PS3, OFF_FROM)), (what, "the source's first bytes")
        s.check_windows(s.arena.ptr + dst_at[0], ps, PS4, OFF_TO, what)
        s.check_whole(s.arena.ptr + dst_at[0], ps, PS4, OFF_TO, what)
        print(what, f"{time.perf_counter() - t0:.3f} s")

    try:
        run(True, 0, "downward table, shipped grid")
        with gpu.testing_flavour():
            try:
                gpu.debug_set_move_table_grid(4)
                run(True, 4, "downward table, four workgroups")
            finally:
                gpu.debug_set_move_table_grid(0)
        run(False, 0, "upward table, shipped grid")
    finally:
        table.free()
        ws.free()


def test_counts_that_pass_2_to_the_32(gpu, oracle, shared):
    """Every byte of the entry a mismatch, so the count passes 2^32 in one entry: src = zeros, expect = 0xFF cycled in place under the
    call's key(s) -- the complement of what the call computes at every index --, size and fill as test_overflow_bounds_all_ones of
    test_gpu_digest.py.  modgpu_verify_device and modgpu_verify_rekey_device must say exactly (n, 0, n): a condition on the data, not a
    measurement.  (Per lane the counts are 32-bit and grow by at most 64 per chunk; the folded sums are 64-bit.)"""
    s = shared
    rig, rig2 = VerifyRig(s), VerifyRekeyRig(s)
    pe, ps = 6, 1
    e, p = s.arena2.ptr + pe, s.arena.ptr + ps
    try:
        s.fill(s.arena, 0x00)
        s.fill(s.arena2, 0xFF)
        gpu.cycle_device(e, N, PS4, OFF)
        s.arena2.sync()
        assert rig.call(e, p, PS4, OFF) == (N, 0, N)
        assert gpu.last_launch()["variant"] == 10 and gpu.last_launch()["bytes"] == N
        gpu.cycle_device(e, N, PS3, OFF_FROM)  # now 0xFF ^ ks(PS4)[OFF + j] ^ ks(PS3)[OFF_FROM + j]
        s.arena2.sync()
        assert rig2.call(e, p, (PS3, PS4), (OFF_FROM, OFF)) == (N, 0, N)
        assert gpu.last_launch()["variant"] == 12 and gpu.last_launch()["bytes"] == N
        # the fills stand around the entries, and the source is still zero where a window looks
        assert (s.arena2.download(pe) == 0xFF).all() and (s.arena2.download(ARENA_LEN - pe - N, offset=pe + N) == 0xFF).all()
        assert not s.arena.download(CHUNK, offset=ps + N - CHUNK).any() and not s.arena.download(CHUNK).any()
    finally:
        rig.rb.free()
        rig2.rb.free()
