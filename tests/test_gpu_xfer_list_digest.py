"""GPU: the digesting list transfers (modgpu_cycle_host_to_device_list_digest, modgpu_cycle_device_to_host_list_digest) against the CPU
oracle and zlib.

Every case lays its entries out as tests/test_gpu_xfer_list.py does (its Layout and its lists are imported: guard bytes around EVERY
entry, the whole arenas compared), runs the list up and down under BOTH sides, and compares every record -- n and the reserved word
included, and a guard record at either end of the records -- with zlib.adler32 of the bytes the oracle expects: an upload reads the
plaintext and stores the ciphertext, a download the other way round, MODGPU_DIGEST_INPUT is of what was read, MODGPU_DIGEST_OUTPUT of what
was stored.  The launches are counted (ONE per call, ceil(total / most) under a lowered limit) and last_launch() is variant 22, a funnel
kernel, the transfer TU's source hash.  The reference is never a list call.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library
loads, so every byte and every sum compared here came from a kernel.  No case injects a failure: tests/xfer_list_digest_main.cpp does
that on the CPU stand-in, where it also runs the lists below."""
import zlib

import numpy as np
import pytest

import test_gpu_xfer_list as X
from test_gpu_xfer_list import gpu, gpu_t, chunk  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PIECE, ADLER = X.PIECE, 65521
OUTPUT, INPUT = 0, 1
REC_FILL = 0xA7


class Records:
    """device memory for one record per entry of a list, a guard record at either end"""

    def __init__(self, M, n):
        self.M, self.n = M, n
        self.buf = M.DeviceBuffer(32 * (n + 2))
        self.fill()

    def fill(self):
        self.buf.upload(np.full(32 * (self.n + 2), REC_FILL, np.uint8))

    @property
    def ptr(self):
        return self.buf.ptr + 32

    def guards_intact(self):
        raw = self.buf.download()
        return bool(np.all(raw[:32] == REC_FILL) and np.all(raw[-32:] == REC_FILL))

    def raw(self):
        return self.buf.download()

    def free(self):
        self.buf.free()


def expected_adlers(L, plain):
    """zlib's Adler-32 per entry of the plaintext (the host sources) or of the ciphertext (the oracle's device image)"""
    arena, at = (L.src, L.h_at) if plain else (L.want_dev, L.d_at)
    return np.array([zlib.adler32(arena[a:a + s[0]].tobytes()) for s, a in zip(L.specs, at)], dtype=np.uint32)


def check_records(L, recs, adlers, plain, what):
    want_n = np.array([s[0] for s in L.specs], dtype=np.uint64)
    assert np.array_equal(recs["n"], want_n) and not recs["reserved"].any(), what
    empty = want_n == 0
    assert not recs["s1"][empty].any() and not recs["s2"][empty].any(), (what, "an empty entry's record")
    bad = np.flatnonzero(adlers != expected_adlers(L, plain))
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def digest_launches(M, before, upload, total, most=0):
    st = M.path_stats()
    k, last = X.windows(total, most)
    assert st["gpu_launches"] - before == (k if total else 0), (st["gpu_launches"] - before, k)
    if total:
        ll = M.last_launch()
        name = "modgpu_cycle_xfer_kernel<%s, true>" % ("true" if upload else "false")
        assert ll["variant"] == 22 and ll["kernel"] == name and ll["source_hash"] == M.xfer_kernel_source_hash() and ll["bytes"] == last, ll


def round_trip(M, L, side, most=0):
    """up, then down, under `side`: every record, every byte of the three arenas, the sources unchanged, the launches"""
    R = Records(M, len(L.specs))
    src_keep = L.src.copy()
    before = M.path_stats()["gpu_launches"]
    recs, adlers = M.cycle_host_to_device_list_digest(L.table(True), side, R.ptr)
    digest_launches(M, before, True, L.total, most)
    bad = np.flatnonzero(L.dev.download() != L.want_dev)
    assert bad.size == 0, ("upload", bad.size, bad[:8].tolist())
    assert np.array_equal(L.src, src_keep), "the upload changed a source"
    check_records(L, recs, adlers, side == INPUT, ("upload", side))
    assert R.guards_intact()
    R.fill()
    before = M.path_stats()["gpu_launches"]
    recs, adlers = M.cycle_device_to_host_list_digest(L.table(False), side, R.ptr)
    digest_launches(M, before, False, L.total, most)
    bad = np.flatnonzero(L.back != L.want_back)
    assert bad.size == 0, ("download", bad.size, bad[:8].tolist())
    assert np.array_equal(L.dev.download(), L.want_dev), "the download changed a source"
    check_records(L, recs, adlers, side == OUTPUT, ("download", side))
    assert R.guards_intact()
    R.free()


def both_sides(M, oracle, specs, most=0, prepare=None):
    L = X.Layout(M, oracle, specs)
    if prepare:
        prepare(L)
    for side in (OUTPUT, INPUT):
        round_trip(M, L, side, most)
        L.reset()  # (both destinations back to their fill: the second side proves itself)
    L.free()


def test_phases_and_sizes(gpu, oracle):
    assert sum(1 for k in X.KEYS if k % 0x7FFFFFFF == 0) == 2  # both identity keys
    both_sides(gpu, oracle, X.phases_and_sizes())


def test_boundaries(gpu, oracle, chunk):
    both_sides(gpu, oracle, X.boundaries(chunk))


def test_every_source_byte_ff(gpu, oracle):
    """One entry of 4 pieces + 77 bytes at an odd phase, every source byte 0xFF: the largest sums a lane and a wave can meet (side INPUT
    of the upload sums exactly these bytes), and five workgroups' segments, four with into != 0, landing on one record"""
    M = gpu
    n = 4 * PIECE + 77

    def ones(L):
        L.src[L.h_at[0]:L.h_at[0] + n] = 0xFF
        L.want_back[L.h_at[0]:L.h_at[0] + n] = 0xFF
        L.want_dev[L.d_at[0]:L.d_at[0] + n] = oracle.cycle_at(L.src[L.h_at[0]:L.h_at[0] + n].copy(), 0x90CFC0AB, 5)

    both_sides(M, oracle, [(n, 0x90CFC0AB, 5, 3, 9)], prepare=ones)


def test_the_position_wraps_twice(gpu, oracle):
    both_sides(gpu, oracle, [(2 * ADLER + 5, 0xC64EED30, 7, 11, 2)])


def test_ten_thousand_tiny_entries(gpu, oracle):
    """entries of 1-7 bytes: thousands of records per piece, only wave 0 with bytes"""
    specs = [(1 + i % 7, X.KEYS[i % 6], (X.OFFSETS[i % 7] + i) % (1 << 64), i % 16, (i * 11) % 16) for i in range(10000)]
    both_sides(gpu, oracle, specs)


def test_empty_entries(gpu, oracle):
    M = gpu
    both_sides(M, oracle, X.with_empties())
    both_sides(M, oracle, [X.NUL, X.EMPTY, X.NUL])  # only such entries: the records are written, nothing is launched
    before = M.path_stats()["gpu_launches"]
    recs, adlers = M.cycle_host_to_device_list_digest(M.table(0))
    assert recs.size == 0 and adlers.size == 0 and M.lib().modgpu_cycle_device_to_host_list_digest(None, 0, 7, None, -1) == 0
    assert M.path_stats()["gpu_launches"] == before


def test_long_entries(gpu, oracle):
    """8 MiB + 3 pieces + 77 at offset 2^64 - 3 and its siblings (32 MiB): into >= 2^23 and every slot refilled"""
    specs = X.long_entries()
    assert specs[1][0] > 1 << 23 and specs[1][2] == (1 << 64) - 3
    both_sides(gpu, oracle, specs)


@pytest.mark.parametrize("most", [300000, 3 * PIECE])
def test_windows(gpu_t, oracle, most):
    """the one-launch limit lowered: ceil(total / most) launches, an entry clipped by a window -- and every record the whole entry's"""
    M = gpu_t
    specs = X.phases_and_sizes()
    starts = np.cumsum([0] + [s[0] for s in specs])
    total = int(starts[-1])
    assert X.windows(total, most)[0] == -(-total // most) > 1
    assert any(a < w < b for w in range(most, total, most) for a, b in zip(starts[:-1], starts[1:])), "no entry is clipped by a window"
    M.debug_set_host_tunable("xfer_list_most_bytes", most)
    both_sides(M, oracle, specs, most)
    M.debug_set_host_tunable("xfer_list_most_bytes", 0)


def test_refusals_on_a_live_device(gpu, oracle):
    M = gpu
    lib = M.lib()
    L = X.Layout(M, oracle, [(1000, 0x90CFC0AB, 0, 1, 2), (2000, 0xC64EED30, 5, 3, 4), X.NUL, (3000, 1, 7, 5, 6), (4000, 0x90CFC0AB, 9, 7, 8)])
    R = Records(M, 5)
    src_keep, rec_keep, before = L.src.copy(), R.raw(), M.path_stats()["gpu_launches"]
    host_records = np.zeros(5, dtype=M.DIGEST_RESULT_DTYPE)
    import ctypes
    for upload in (True, False):
        call = lib.modgpu_cycle_host_to_device_list_digest if upload else lib.modgpu_cycle_device_to_host_list_digest
        t = L.table(upload)

        def refused(side, records, text):
            assert call(ctypes.c_void_p(t.ctypes.data), t.size, side, ctypes.c_void_p(records), -1) == 1, text
            assert text in lib.modgpu_last_error().decode(), lib.modgpu_last_error().decode()

        refused(OUTPUT, 0, "NULL records")
        refused(INPUT, R.ptr + 4, "not 8-byte aligned")
        refused(OUTPUT, host_records.ctypes.data, "the records are not device memory")
        refused(2, R.ptr, "a side other than")
        refused(OUTPUT, L.dev.ptr + (L.d_at[3] + 7) // 8 * 8, "entry 3: its device range meets the records")
        t[("dst" if upload else "src")][3] = L.back.ctypes.data + 64  # the plain calls' refusals, with their texts
        refused(OUTPUT, R.ptr, "entry 3: its device side is not device memory")
    assert M.path_stats()["gpu_launches"] == before
    assert np.all(L.dev.download() == X.DEV_FILL) and np.all(L.back == X.HOST_FILL) and np.array_equal(L.src, src_keep)
    assert np.array_equal(R.raw(), rec_keep)
    R.free()
    round_trip(M, L, INPUT)  # ... and the same buffers take a good list afterwards
    L.free()


def test_same_records_and_bytes_as_the_two_call_route(gpu, oracle):
    """one mixed list: the digesting call against the plain list call followed by modgpu_digest_table_device over the same ranges"""
    M = gpu
    specs = X.with_empties() + X.phases_and_sizes()[:25]
    A, B = X.Layout(M, oracle, specs, seed=7), X.Layout(M, oracle, specs, seed=7)
    ra, _ = M.cycle_host_to_device_list_digest(A.table(True), OUTPUT)
    M.cycle_host_to_device_list(B.table(True))
    t = B.table(True)
    t["src"] = t["dst"]  # what was stored, as the digest table call reads it: the device range under the identity key
    t["key"] = 0
    rb, _ = M.digest_table_device(t)
    assert np.array_equal(A.dev.download(), B.dev.download())
    for f in ("s1", "s2"):
        assert np.array_equal(ra[f] % ADLER, rb[f] % ADLER), f
    assert np.array_equal(ra["n"], rb["n"]) and not ra["reserved"].any()
    ra, _ = M.cycle_device_to_host_list_digest(A.table(False), INPUT)  # what was read: the same device ranges
    M.cycle_device_to_host_list(B.table(False))
    assert np.array_equal(A.back, B.back) and np.array_equal(A.back, A.want_back)
    for f in ("s1", "s2"):
        assert np.array_equal(ra[f] % ADLER, rb[f] % ADLER), f
    A.free()
    B.free()


def test_records_into_the_device_check_and_the_buffer_methods(gpu, oracle):
    M = gpu
    L = X.Layout(M, oracle, X.phases_and_sizes()[:30], seed=3)
    R = Records(M, len(L.specs))
    _, adlers = M.cycle_host_to_device_list_digest(L.table(True), INPUT, R.ptr)
    manifest = expected_adlers(L, True)
    assert np.array_equal(adlers, manifest)
    assert M.digest_check_device(R.ptr, manifest, manifest.size)[0] == 0
    planted = manifest.copy()
    planted[17] ^= 0x10000
    bad, lowest, which = M.digest_check_device(R.ptr, planted, planted.size)
    assert (bad, lowest, which.tolist()) == (1, 17, [17])
    R.free()
    L.free()
    # DeviceBuffer.upload_ranges_digest / download_ranges_checked end to end
    key, part_off = 0xC64EED30, (1 << 32) - 1000
    files = [oracle.splitmix_bytes(n, 40 + i) for i, n in enumerate((100, 0, 65536 + 5, 4097, 3 * PIECE + 1))]
    offs = [7, 200, 301, 70001, 80000]
    buf = M.DeviceBuffer(200000)
    buf.upload(np.zeros(200000, np.uint8))
    before = M.path_stats()["gpu_launches"]
    got = buf.upload_ranges_digest(list(zip(offs, files)), key, part_off)
    assert M.path_stats()["gpu_launches"] - before == 1
    want = np.array([zlib.adler32(f.tobytes()) for f in files], dtype=np.uint32)
    assert np.array_equal(got, want)
    for o, f in zip(offs, files):
        if f.size:
            assert np.array_equal(buf.download(f.size, offset=o), oracle.cycle_at(f.copy(), key, (part_off + o) % X.PERIOD))
    outs = [np.full(f.size, X.HOST_FILL, np.uint8) for f in files]
    adlers, outcome = buf.download_ranges_checked([(o, f.size) for o, f in zip(offs, files)], key, outs, want, part_off)
    assert np.array_equal(adlers, want) and outcome[0] == 0 and outcome[1] is None
    assert all(np.array_equal(a, f) for a, f in zip(outs, files))
    wrong = want.copy()
    wrong[3] ^= 1
    adlers, (bad, lowest, which) = buf.download_ranges_checked([(o, f.size) for o, f in zip(offs, files)], key, outs, wrong, part_off)
    assert np.array_equal(adlers, want) and (bad, lowest, which.tolist()) == (1, 3, [3])
    buf.free()


def test_twice_on_the_same_records(gpu, oracle):
    M = gpu
    L = X.Layout(M, oracle, X.phases_and_sizes(), seed=5)
    R = Records(M, len(L.specs))
    first, a1 = M.cycle_host_to_device_list_digest(L.table(True), OUTPUT, R.ptr)
    second, a2 = M.cycle_host_to_device_list_digest(L.table(True), OUTPUT, R.ptr)
    for f in ("s1", "s2"):
        assert np.array_equal(first[f] % ADLER, second[f] % ADLER), f
    assert np.array_equal(first["n"], second["n"]) and not second["reserved"].any() and np.array_equal(a1, a2)
    assert np.array_equal(a2, expected_adlers(L, False)) and R.guards_intact()
    R.free()
    L.free()
