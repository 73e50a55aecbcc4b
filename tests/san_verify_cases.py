"""Cases for the sanitizer builds of libmodgpu's host code: the VERIFY entry points (modgpu_verify_device /
modgpu_verify_batch_device / modgpu_verify_results).

Not collected by a plain `pytest tests/`: tests/test_verify_cpu.py runs this file in a child process with MODGPU_LIB pointing at
_san/libmodgpu_asan.so or _san/libmodgpu_tsan.so and the matching runtime preloaded (the pattern of tests/san_rekey_cases.py).  In those
builds a launch executes the launch PLAN on the CPU (tests/cpu_runtime_standin/standin_launch_verify.cpp): it reads `expect` and `src`
exactly where the plan says the kernels would and writes only the result, so the sanitizers see every byte, and every case states the
exact {mismatches, first_mismatch, n} it expects, with the expected bytes taken from the oracle."""
import ctypes
import os
import threading

import numpy as np
import pytest

import modulate_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not os.environ.get("MODGPU_LIB"), reason="runs only against a sanitizer build (tests/test_verify_cpu.py)")

CHUNK = 65536
GUARD = 32
NONE = M.VERIFY_NONE
PS3, PS4 = M.KEY_PS3, M.KEY_PS4


@pytest.fixture(scope="module")
def lib():
    L = M.lib()
    assert M.testing_hooks() and M.device_count() == 8, "expects the shim build with MODGPU_SHIM_DEVICES=8"
    for name in ("modgpu_shim_verify_launches", "modgpu_shim_verify_inits", "modgpu_shim_verify_plan_errors"):
        getattr(L, name).restype = ctypes.c_ulonglong
    L.modgpu_shim_xfer_alloc.restype = ctypes.c_void_p
    L.modgpu_shim_xfer_alloc.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
    L.modgpu_shim_xfer_free.argtypes = [ctypes.c_void_p]
    yield L
    assert L.modgpu_shim_verify_plan_errors() == 0


class Res:
    """results in "device memory" of the stand-in: what modgpu_shim_xfer_alloc hands out is what it reports as device memory of
    `device` (memory from modgpu_alloc is not on its record), filled with 0xEE so that a result nobody initialised shows"""

    def __init__(self, L, count, device=0):
        self.L, self.nbytes, self.device = L, 32 * count, device
        self.ptr = L.modgpu_shim_xfer_alloc(self.nbytes, device)
        assert self.ptr
        ctypes.memset(self.ptr, 0xEE, self.nbytes)

    def raw(self, n, off):
        out = np.empty(n, np.uint8)
        ctypes.memmove(out.ctypes.data, self.ptr + off, n)
        return out

    def sync(self, stream=None):
        assert self.L.modgpu_sync(self.device, ctypes.c_void_p(stream or 0)) == 0

    def free(self):
        self.L.modgpu_shim_xfer_free(self.ptr)


def launches(lib):
    return sum(lib.modgpu_shim_verify_launches(f) for f in range(4))


def triple(r):
    assert int(r["reserved"]) == 0
    return int(r["mismatches"]), int(r["first_mismatch"]), int(r["n"])


def cipher(pt, key, off):
    out = pt.copy()
    O.cycle_at(out, key, off)
    return out


def test_single_calls_at_edges_and_phases(lib):
    """Sizes 0..48 and around a chunk x every expect phase x a few src phases: clean, then with bytes flipped in `expect`."""
    sizes = list(range(49)) + [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
    cap = max(sizes) + 2 * GUARD + 16
    eb, sb, res = M.DeviceBuffer(cap), M.DeviceBuffer(cap), Res(lib, 2)
    rng = np.random.default_rng(11)
    inits, comp = lib.modgpu_shim_verify_inits(), launches(lib)
    calls = nonempty = 0
    for n in sizes:
        src = rng.integers(0, 256, size=n, dtype=np.uint8)
        for pe in range(16):
            for ps in (0, 5, (pe + 4) % 16):
                off = [0, 3, (1 << 32) - 7, (1 << 64) - 3][(pe + ps) % 4]
                want = cipher(src, PS3, off)
                flips = sorted({(n * 7) // 11, n - 1, 0 if pe % 2 else n // 2}) if n else []
                sb.upload(np.concatenate([np.full(GUARD + ps, 0xA5, np.uint8), src, np.full(GUARD, 0xA5, np.uint8)]))
                for bad in (False, True):
                    img = want.copy()
                    if bad:
                        img[flips] ^= 0x40
                    eb.upload(np.concatenate([np.full(GUARD + pe, 0x5A, np.uint8), img, np.full(GUARD, 0x5A, np.uint8)]))
                    M.verify_device(eb.ptr + GUARD + pe, sb.ptr + GUARD + ps, PS3, off, result=res.ptr + 32, n=n)
                    res.sync()
                    got = triple(M.verify_results(res.ptr + 32)[0])
                    assert got == ((len(flips), flips[0], n) if bad and n else (0, NONE, n)), (n, pe, ps, off, bad, got)
                    calls += 1
                    nonempty += 1 if n else 0
    assert lib.modgpu_shim_verify_inits() - inits == calls and launches(lib) - comp == nonempty
    assert M.last_launch()["variant"] == 10
    for b in (eb, sb, res):
        b.free()


def test_identity_key_and_aliases(lib):
    n = CHUNK + 77
    a, res = M.DeviceBuffer(n + 64), Res(lib, 1)
    data = O.splitmix_bytes(n + 64, 4)
    a.upload(data)
    before = lib.modgpu_shim_verify_launches(2) + lib.modgpu_shim_verify_launches(3)
    for key in (0, 0x7FFFFFFF, 0x80000001):  # expect == src, identity keystream: clean
        M.verify_device(a.ptr + 3, a.ptr + 3, key, 9, result=res.ptr, n=n)
        res.sync()
        assert triple(M.verify_results(res.ptr)[0]) == (0, NONE, n)
    assert lib.modgpu_shim_verify_launches(2) + lib.modgpu_shim_verify_launches(3) - before == 3
    # overlapping, shifted by one byte, identity: a memcmp of the buffer with itself one byte on
    diff = np.flatnonzero(data[3:3 + n] != data[4:4 + n])
    M.verify_device(a.ptr + 3, a.ptr + 4, 0, result=res.ptr, n=n)
    res.sync()
    assert triple(M.verify_results(res.ptr)[0]) == (diff.size, int(diff[0]), n)
    # expect == src with a real key: every byte whose keystream byte is nonzero
    ks = cipher(np.zeros(n, np.uint8), PS4, 5)
    nz = np.flatnonzero(ks)
    M.verify_device(a.ptr + 3, a.ptr + 3, PS4, 5, result=res.ptr, n=n)
    res.sync()
    assert triple(M.verify_results(res.ptr)[0]) == (nz.size, int(nz[0]), n)
    assert np.array_equal(a.download(), data)
    a.free()
    res.free()


def test_forty_entry_batch_takes_one_init_and_three_launches(lib):
    rng = np.random.default_rng(40)
    sizes = [int(x) for x in rng.integers(0, CHUNK + 100, size=40)]
    for i in (0, 7, 39):
        sizes[i] = 0
    part_n = 2 * CHUNK + 999
    src_offs = [int(rng.integers(0, part_n - s + 1)) for s in sizes]  # sources overlap each other
    plain = O.splitmix_bytes(part_n, 5)
    part = M.DeviceBuffer(part_n + 16)
    part.upload(plain, offset=3)
    e_offs, at = [], 0
    for i, s in enumerate(sizes):
        at += i % 16
        e_offs.append(at)
        at += s + 16 - i % 16
    stream_offs = [o + (i << 33) for i, o in enumerate(src_offs)]
    image = np.zeros(at + 16, np.uint8)
    for s, o, q, so in zip(sizes, src_offs, e_offs, stream_offs):
        image[q:q + s] = cipher(plain[o:o + s], PS4, so)
    want = [(0, NONE, s) for s in sizes]
    for i, js in ((3, [0]), (20, [sizes[20] - 1]), (33, [sizes[33] // 2, sizes[33] // 2 + 1])):
        for j in js:
            image[e_offs[i] + j] ^= 1
        want[i] = (len(js), js[0], sizes[i])
    exp = M.DeviceBuffer(at + 16)
    exp.upload(image)
    res = Res(lib, 41)
    inits, comp = lib.modgpu_shim_verify_inits(), launches(lib)
    M.verify_batch_device([exp.ptr + q for q in e_offs], [part.ptr + 3 + o for o in src_offs], sizes, PS4, res.ptr, stream_offs=stream_offs)
    res.sync()
    assert lib.modgpu_shim_verify_inits() - inits == 1 and launches(lib) - comp == 3  # 37 non-empty: 16 + 16 + 5
    got = [triple(r) for r in M.verify_results(res.ptr, 40)]
    assert got == want
    assert np.all(res.raw(32, 32 * 40) == 0xEE), "the result behind the last entry's was written"
    assert np.array_equal(exp.download(), image) and np.array_equal(part.download(part_n, offset=3), plain)
    # NULL offsets mean 0 for every entry; an empty batch queues nothing
    exp.upload(cipher(plain[:1000], PS3, 0))
    M.verify_batch_device([exp.ptr], [part.ptr + 3], [1000], PS3, res.ptr)
    res.sync()
    assert triple(M.verify_results(res.ptr)[0]) == (0, NONE, 1000)
    inits = lib.modgpu_shim_verify_inits()
    M.verify_batch_device([], [], [], PS3, 0)
    assert lib.modgpu_shim_verify_inits() == inits
    for b in (part, exp, res):
        b.free()


def test_invalid_results_are_refused_before_anything_is_queued(lib):
    a, res = M.DeviceBuffer(256), Res(lib, 2)
    host = np.zeros(64, np.uint8)
    inits, comp = lib.modgpu_shim_verify_inits(), launches(lib)

    def code(fn, *args, **kw):
        with pytest.raises(M.ModGpuError) as e:
            fn(*args, **kw)
        return e.value.code

    assert code(M.verify_device, a.ptr, a.ptr + 100, PS3, result=res.ptr + 4, n=10) == 1         # misaligned
    assert code(M.verify_device, a.ptr, a.ptr + 100, PS3, result=host.ctypes.data, n=10) == 1    # not device memory
    assert code(M.verify_device, a.ptr, a.ptr + 100, PS3, result=res.ptr + 40, n=10) == 1        # runs off the allocation
    assert code(M.verify_device, a.ptr, a.ptr + 100, PS3, result=a.ptr, n=10) == 1               # memory the runtime does not report as device memory
    assert code(M.verify_device, a.ptr, a.ptr + 100, PS3, result=res.ptr, device=1, n=10) == 1   # another device's memory
    assert code(M.verify_device, 0, a.ptr, PS3, result=res.ptr, n=10) == 1
    assert code(M.verify_device, a.ptr, 0, PS3, result=res.ptr, n=10) == 1
    assert code(M.verify_batch_device, [a.ptr, a.ptr], [a.ptr, a.ptr], [1, 1], PS3, res.ptr + 32) == 1   # two results, room for one
    assert code(M.verify_batch_device, [a.ptr, 0], [a.ptr, a.ptr], [1, 1], PS3, res.ptr) == 1
    assert M.lib().modgpu_verify_batch_device(None, None, None, None, -1, 1, None, -1, None) == 1
    assert M.lib().modgpu_verify_batch_device(None, None, None, None, 2, 1, None, -1, None) == 1
    assert code(M.verify_results, host.ctypes.data, 1) == 1
    assert lib.modgpu_shim_verify_inits() == inits and launches(lib) == comp
    M.verify_device(0, 0, PS3, result=res.ptr + 32, n=0)  # n == 0 with NULL buffers: still a result, from the init launch alone
    res.sync()
    assert triple(M.verify_results(res.ptr + 32)[0]) == (0, NONE, 0) and np.all(res.raw(32, 0) == 0xEE)
    assert lib.modgpu_shim_verify_inits() == inits + 1 and launches(lib) == comp and M.last_launch()["variant"] == 10
    a.free()
    res.free()


def test_eight_threads_on_eight_devices(lib):
    """Eight threads, each on a device and a stream of its own with a result of its own: the per-thread launch record and the counters
    under ThreadSanitizer; every result exact."""
    n = CHUNK + 333
    errors = []

    def worker(t):
        try:
            h = ctypes.c_void_p()
            assert lib.modgpu_shim_stream_create(ctypes.byref(h)) == 0 and h.value
            eb, sb, res = M.DeviceBuffer(n + 64, device=t), M.DeviceBuffer(n + 64, device=t), Res(lib, 1, device=t)
            src = O.splitmix_bytes(n, 100 + t)
            sb.upload(src, offset=t)
            for k in range(4):
                img = cipher(src, PS3, (t << 32) + k)
                if k % 2:
                    img[1000 * t + k] ^= 0x80
                eb.upload(img, offset=(3 * t + k) % 16)
                M.verify_device(eb.ptr + (3 * t + k) % 16, sb.ptr + t, PS3, (t << 32) + k, result=res.ptr, device=t, stream=h.value, n=n)
                res.sync(h.value)
                assert triple(M.verify_results(res.ptr, 1, device=t)[0]) == ((1, 1000 * t + k, n) if k % 2 else (0, NONE, n)), (t, k)
                assert M.last_launch()["variant"] == 10
            for b in (eb, sb, res):
                b.free()
            lib.modgpu_shim_stream_destroy(h)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
