"""Cases for the sanitizer builds of libmodgpu's host code: the REKEY entry points (modgpu_rekey_device_to /
modgpu_rekey_batch_device_to).

Not collected by a plain `pytest tests/`: tests/test_rekey_cpu.py runs this file in a child process with MODGPU_LIB pointing at
_san/libmodgpu_asan.so or _san/libmodgpu_tsan.so and the matching runtime preloaded (the pattern of tests/san_to_cases.py).  In those
builds a launch executes the launch PLAN on the CPU (tests/cpu_runtime_standin/standin_launch_rekey.cpp): it reads the source and
writes the destination exactly where the plan says the kernel would, so the sanitizers see every byte, and every case compares the
destination with the oracle -- dst = cycle_at(cycle_at(src, key_from, off_from), key_to, off_to) -- and checks that the source did not
change."""
import ctypes
import os
import threading

import numpy as np
import pytest

import modulate_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not os.environ.get("MODGPU_LIB"), reason="runs only against a sanitizer build (tests/test_rekey_cpu.py)")

CHUNK = 65536
GUARD = 32
PS3, PS4 = M.KEY_PS3, M.KEY_PS4


@pytest.fixture(scope="module")
def lib():
    L = M.lib()
    assert M.testing_hooks() and M.device_count() == 8, "expects the shim build with MODGPU_SHIM_DEVICES=8"
    for name in ("modgpu_shim_rekey_launches", "modgpu_shim_rekey_collisions", "modgpu_shim_rekey_plan_errors"):
        getattr(L, name).restype = ctypes.c_ulonglong
    yield L
    assert L.modgpu_shim_rekey_collisions() == 0 and L.modgpu_shim_rekey_plan_errors() == 0


def launches(lib):
    return lib.modgpu_shim_rekey_launches(0) + lib.modgpu_shim_rekey_launches(1)


def expected(pt, kf, of, kt, ot):
    want = pt.copy()
    O.cycle_at(want, kf, of)
    O.cycle_at(want, kt, ot)
    return want


def run(src, dst, pt, ps, pd, kf, of, kt, ot, device=-1, stream=None):
    n = pt.size
    s_img = np.full(src.nbytes, 0xA5, np.uint8)
    s_img[GUARD + ps:GUARD + ps + n] = pt
    d_img = np.full(dst.nbytes, 0x5A, np.uint8)
    src.upload(s_img)
    dst.upload(d_img)
    M.rekey_device_to(dst.ptr + GUARD + pd, src.ptr + GUARD + ps, kf, kt, of, ot, device=device, stream=stream, n=n)
    dst.sync(stream)
    want = d_img.copy()
    want[GUARD + pd:GUARD + pd + n] = expected(pt, kf, of, kt, ot)
    assert np.array_equal(dst.download(), want), (n, ps, pd, hex(kf), of, hex(kt), ot)
    assert np.array_equal(src.download(), s_img), ("source changed", n, ps, pd)


def test_single_calls_at_edges_phases_and_offsets(lib):
    """Sizes around 0, one word and a chunk; source phases 0..15 against a few destination phases; offsets of other phases mod 16,
    near 2^32 and near 2^64."""
    sizes = [0, 1, 15, 16, 17, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5]
    src, dst = M.DeviceBuffer(max(sizes) + 2 * GUARD + 16), M.DeviceBuffer(max(sizes) + 2 * GUARD + 16)
    rng = np.random.default_rng(21)
    before = launches(lib)
    calls = 0
    for n in sizes:
        pt = rng.integers(0, 256, size=n, dtype=np.uint8)
        for ps in range(16):
            for pd in (0, 5, 15):
                of, ot = [(0, 0), (3, 22), ((1 << 32) - 7, 5), ((1 << 63) + 9, (1 << 32) + 1)][(ps + pd) % 4]
                run(src, dst, pt, ps, pd, PS3, of, PS4, ot)
                calls += 1 if n else 0
    assert launches(lib) - before == calls  # one launch per non-empty call
    assert M.last_launch()["variant"] == 7
    src.free()
    dst.free()


def test_degenerate_keys_route_to_the_out_of_place_call(lib):
    n = CHUNK + 77
    src, dst = M.DeviceBuffer(n + 2 * GUARD + 16), M.DeviceBuffer(n + 2 * GUARD + 16)
    pt = O.splitmix_bytes(n, 4)
    before = launches(lib)
    for kf, of, kt, ot, variant in ((0, 9, PS4, 13, 5), (PS3, 9, 0x7FFFFFFF, 13, 5), (0, 1, 0x80000001, 2, None), (PS3, 7, PS3, 7 + O.PERIOD, None)):
        M.cycle_device(dst.ptr, 16, 1)  # a launch of a known variant: a copy must leave it the latest
        dst.sync()
        run(src, dst, pt, 3, 0, kf, of, kt, ot)
        assert M.last_launch()["variant"] == (variant if variant is not None else 0), (kf, kt)
    assert launches(lib) == before, "a degenerate keystream never takes the rekey kernel"
    run(src, dst, pt, 3, 0, PS3, 7, PS3, 8)  # same key, other offset: a real rekey
    assert launches(lib) == before + 1
    src.free()
    dst.free()


def test_in_place_alias_and_round_trip(lib):
    n = 3 * CHUNK + 5
    pt = O.splitmix_bytes(n + 64, 12)
    a = M.DeviceBuffer(n + 64)
    a.upload(pt)
    M.rekey_device_to(a.ptr + 3, a.ptr + 3, PS3, PS4, 11, 40, n=n)
    a.sync()
    got = a.download()
    assert np.array_equal(got[3:3 + n], expected(pt[3:3 + n], PS3, 11, PS4, 40)) and np.array_equal(got[:3], pt[:3])
    M.rekey_device_to(a.ptr + 3, a.ptr + 3, PS4, PS3, 40, 11, n=n)
    a.sync()
    assert np.array_equal(a.download(), pt)
    with pytest.raises(M.ModGpuError) as e:
        M.rekey_device_to(a.ptr + 4, a.ptr + 3, PS3, PS4, n=n)
    assert e.value.code == 1
    a.free()


def test_forty_entry_relocation_takes_three_launches(lib):
    """40 files of a PS3 part, sources overlapping, rekeyed to PS4 at new offsets of a new part: 16 + 16 + 8 entries, three launches;
    the new part equals the new plaintext layout encrypted directly."""
    rng = np.random.default_rng(40)
    sizes = [int(x) for x in rng.integers(0, CHUNK + 100, size=40)]
    sizes[7] = 0
    part_n = 2 * CHUNK + 999
    old_offs = [int(rng.integers(0, part_n - s + 1)) for s in sizes]
    plain = O.splitmix_bytes(part_n, 5)
    enc = plain.copy()
    O.cycle_at(enc, PS3, 0)
    part = M.DeviceBuffer(part_n + 16)
    part.upload(enc, offset=3)
    new_offs, at = [], 0
    for i, s in enumerate(sizes):
        at += i % 16
        new_offs.append(at)
        at += s + 16 - i % 16
    new = M.DeviceBuffer(at + 16)
    new.upload(np.zeros(at + 16, np.uint8))
    before = launches(lib)
    M.rekey_batch_device_to([new.ptr + o for o in new_offs], [part.ptr + 3 + o for o in old_offs], sizes, PS3, PS4,
                            offs_from=old_offs, offs_to=new_offs)
    new.sync()
    assert launches(lib) - before == 3
    layout = np.zeros(at + 16, np.uint8)
    for s, o, q in zip(sizes, old_offs, new_offs):
        layout[q:q + s] = plain[o:o + s]
    direct = layout.copy()
    O.cycle_at(direct, PS4, 0)
    got = new.download()
    for s, q in zip(sizes, new_offs):
        assert np.array_equal(got[q:q + s], direct[q:q + s]), q
    assert np.array_equal(part.download(part_n, offset=3), enc)
    # NULL offsets mean 0 for every entry
    M.rekey_batch_device_to([new.ptr], [part.ptr + 3], [1000], PS3, PS4)
    new.sync()
    assert np.array_equal(new.download(1000), expected(enc[:1000], PS3, 0, PS4, 0))
    # a destination that meets another entry's source: the whole call is refused, nothing queued
    n_before = launches(lib)
    with pytest.raises(M.ModGpuError) as e:
        M.rekey_batch_device_to([new.ptr, part.ptr + 3], [part.ptr + 3, part.ptr + 100], [10, 10], PS3, PS4)
    assert e.value.code == 1 and launches(lib) == n_before
    part.free()
    new.free()


def test_streams_share_the_ring(lib):
    """Eight threads, each on a stream of its own on one device, rekey at once: the ticket ring, the per-thread launch record and the
    counters under ThreadSanitizer; every result bit-exact."""
    n = CHUNK + 333
    errors = []

    def worker(t):
        try:
            h = ctypes.c_void_p()
            assert lib.modgpu_shim_stream_create(ctypes.byref(h)) == 0 and h.value
            src, dst = M.DeviceBuffer(n + 2 * GUARD + 16, device=0), M.DeviceBuffer(n + 2 * GUARD + 16, device=0)
            pt = O.splitmix_bytes(n, 100 + t)
            for k in range(4):
                run(src, dst, pt, (t + k) % 16, (3 * t + k) % 16, PS3, t << 32, PS4, k, device=0, stream=h.value)
                assert M.last_launch()["variant"] == 7
            src.free()
            dst.free()
            lib.modgpu_shim_stream_destroy(h)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


def test_no_ticket_falls_back_to_two_passes(lib):
    """A ring of one line, held by a rekey in flight on another stream: the call finds no ticket pair and takes two passes on its own
    stream (out of place under key_from, then in place under key_to) -- the same bytes, and the in-place launch is the one reported."""
    big_n, n = 4 << 20, 2 * CHUNK + 45
    hold_src, hold_dst = M.DeviceBuffer(big_n, device=0), M.DeviceBuffer(big_n, device=0)
    src, dst = M.DeviceBuffer(n + 16, device=0), M.DeviceBuffer(n + 16, device=0)
    pt = O.splitmix_bytes(n, 31)
    src.upload(pt, offset=5)
    dst.upload(np.zeros(n + 16, np.uint8))
    h = ctypes.c_void_p()
    assert lib.modgpu_shim_stream_create(ctypes.byref(h)) == 0 and h.value
    with M.testing_flavour():
        M.debug_set_queue_ring(1)
    try:
        before = launches(lib)
        M.rekey_device_to(hold_dst, hold_src, PS3, PS4, device=0, stream=h.value)  # takes the only line for a while
        M.rekey_device_to(dst.ptr, src.ptr + 5, PS3, PS4, 70, 3, device=0, n=n)
        info = M.last_launch()
        dst.sync()
        hold_dst.sync(h.value)
    finally:
        with M.testing_flavour():
            M.debug_set_queue_ring(0)
        lib.modgpu_shim_stream_destroy(h)
    assert launches(lib) - before == 1, "only the holder took the rekey kernel"
    assert info["variant"] in (0, 1, 2), info
    assert np.array_equal(dst.download(n), expected(pt, PS3, 70, PS4, 3))
    assert np.array_equal(src.download(n, offset=5), pt)
    for b in (hold_src, hold_dst, src, dst):
        b.free()
