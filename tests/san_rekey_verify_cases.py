"""Cases for the sanitizer builds of libmodgpu's host code: the REKEY VERIFY entry points (modgpu_verify_rekey_device /
modgpu_verify_rekey_batch_device).

Not collected by a plain `pytest tests/`: tests/test_verify_rekey_cpu.py runs this file in a child process with MODGPU_LIB pointing at
_san/libmodgpu_asan.so or _san/libmodgpu_tsan.so and the matching runtime preloaded (the pattern of tests/san_verify_cases.py).  In those
builds a launch executes the launch PLAN on the CPU (tests/cpu_runtime_standin/standin_launch_rekey_verify.cpp, and
standin_launch_verify.cpp for the entries whose keystreams are degenerate): it reads `expect` and `src` exactly where the plan says the
kernels would and writes only the result, so the sanitizers see every byte.  Every case states the exact {mismatches, first_mismatch, n}
it expects against a Python statement of the arithmetic: the oracle's cipher under key_from at off_from, then under key_to at off_to."""
import ctypes
import os
import threading

import numpy as np
import pytest

import modulate_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not os.environ.get("MODGPU_LIB"), reason="runs only against a sanitizer build (tests/test_verify_rekey_cpu.py)")

CHUNK = 65536
GUARD = 32
NONE = M.VERIFY_NONE
PS3, PS4 = M.KEY_PS3, M.KEY_PS4
PERIOD = (1 << 31) - 2


@pytest.fixture(scope="module")
def lib():
    L = M.lib()
    assert M.testing_hooks() and M.device_count() == 8, "expects the shim build with MODGPU_SHIM_DEVICES=8"
    for name in ("modgpu_shim_verify_launches", "modgpu_shim_verify_inits", "modgpu_shim_verify_plan_errors", "modgpu_shim_rekey_verify_launches",
                 "modgpu_shim_rekey_verify_plan_errors"):
        getattr(L, name).restype = ctypes.c_ulonglong
    L.modgpu_shim_xfer_alloc.restype = ctypes.c_void_p
    L.modgpu_shim_xfer_alloc.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
    L.modgpu_shim_xfer_free.argtypes = [ctypes.c_void_p]
    yield L
    assert L.modgpu_shim_verify_plan_errors() == 0 and L.modgpu_shim_rekey_verify_plan_errors() == 0


class Res:
    """results in "device memory" of the stand-in (what modgpu_shim_xfer_alloc hands out is what it reports as device memory of
    `device`), filled with 0xEE so that a result nobody initialised shows"""

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


def two(lib):
    return lib.modgpu_shim_rekey_verify_launches(0) + lib.modgpu_shim_rekey_verify_launches(1)


def one(lib, forms=range(4)):
    return sum(lib.modgpu_shim_verify_launches(f) for f in forms)


def triple(r):
    assert int(r["reserved"]) == 0
    return int(r["mismatches"]), int(r["first_mismatch"]), int(r["n"])


def rekeyed(pt, key_from, off_from, key_to, off_to):
    out = pt.copy()
    O.cycle_at(out, key_from, off_from)
    O.cycle_at(out, key_to, off_to)
    return out


def test_single_calls_at_edges_and_phases(lib):
    """Sizes 0..48 and around a chunk x every expect phase x a few src phases: clean, then with bytes flipped in `expect`."""
    sizes = list(range(49)) + [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
    cap = max(sizes) + 2 * GUARD + 16
    eb, sb, res = M.DeviceBuffer(cap), M.DeviceBuffer(cap), Res(lib, 2)
    rng = np.random.default_rng(11)
    inits, comp, plain = lib.modgpu_shim_verify_inits(), two(lib), one(lib)
    calls = nonempty = 0
    for n in sizes:
        src = rng.integers(0, 256, size=n, dtype=np.uint8)
        for pe in range(16):
            for ps in (0, 5, (pe + 4) % 16):
                off_from = [0, 3, (1 << 32) - 7, (1 << 64) - 3][(pe + ps) % 4]
                off_to = [11, (1 << 63) + 5, 0][pe % 3]
                want = rekeyed(src, PS3, off_from, PS4, off_to)
                flips = sorted({(n * 7) // 11, n - 1, 0 if pe % 2 else n // 2}) if n else []
                sb.upload(np.concatenate([np.full(GUARD + ps, 0xA5, np.uint8), src, np.full(GUARD, 0xA5, np.uint8)]))
                for bad in (False, True):
                    img = want.copy()
                    if bad:
                        img[flips] ^= 0x40
                    eb.upload(np.concatenate([np.full(GUARD + pe, 0x5A, np.uint8), img, np.full(GUARD, 0x5A, np.uint8)]))
                    M.verify_rekey_device(eb.ptr + GUARD + pe, sb.ptr + GUARD + ps, PS3, PS4, off_from, off_to, result=res.ptr + 32, n=n)
                    res.sync()
                    got = triple(M.verify_results(res.ptr + 32)[0])
                    assert got == ((len(flips), flips[0], n) if bad and n else (0, NONE, n)), (n, pe, ps, off_from, off_to, bad, got)
                    calls += 1
                    nonempty += 1 if n else 0
    assert lib.modgpu_shim_verify_inits() - inits == calls and two(lib) - comp == nonempty and one(lib) == plain
    info = M.last_launch()
    assert info["variant"] == 12 and info["source_hash"] == M.rekey_verify_kernel_source_hash()
    assert np.all(res.raw(32, 0) == 0xEE)
    for b in (eb, sb, res):
        b.free()


def test_degenerate_keystreams_run_on_the_verify_launches(lib):
    """A zero key on one side leaves the other keystream (keyed verify launch), on both a plain compare; the same reduced key at the
    same stream position (offsets equal mod 2^31-2) is a plain compare; none of them reaches the two-keystream launch."""
    n = CHUNK + 77
    eb, sb, res = M.DeviceBuffer(n + 64), M.DeviceBuffer(n + 64), Res(lib, 1)
    src = O.splitmix_bytes(n, 4)
    sb.upload(src, offset=6)
    same_res = (12345 - ((1 << 31) - 1)) & 0xFFFFFFFF
    cases = [((0, PS4), (3, 9), False), ((0x7FFFFFFF, PS3), (3, 9), False), ((PS4, 0x80000001), (3, 9), False), ((0, 0x7FFFFFFF), (3, 9), True),
             ((PS4, PS4), (5, 5), True), ((PS3, PS3), (5, 5 + PERIOD), True), ((PS3, PS3), ((1 << 63) + PERIOD, 1 << 63), True),
             ((12345, same_res), (8, 8), True)]
    for keys, offs, ident in cases:
        before_two, before_keyed, before_ident = two(lib), one(lib, (0, 1)), one(lib, (2, 3))
        want = rekeyed(src, keys[0], offs[0], keys[1], offs[1])
        if ident:
            assert np.array_equal(want, src)
        for flips in ([], [0, n // 2, n - 1]):
            img = want.copy()
            img[flips] ^= 0x08
            eb.upload(img, offset=3)
            M.verify_rekey_device(eb.ptr + 3, sb.ptr + 6, keys[0], keys[1], offs[0], offs[1], result=res.ptr, n=n)
            res.sync()
            assert triple(M.verify_results(res.ptr)[0]) == ((3, 0, n) if flips else (0, NONE, n)), (keys, offs, flips)
            assert M.last_launch()["variant"] == 10
        assert two(lib) == before_two
        assert one(lib, (0, 1)) - before_keyed == (0 if ident else 2) and one(lib, (2, 3)) - before_ident == (2 if ident else 0), (keys, offs)
    # the same key at different positions IS two streams; expect == src under them: every byte whose two keystream bytes differ
    a = M.DeviceBuffer(n + 64)
    data = O.splitmix_bytes(n + 64, 9)
    a.upload(data)
    ks = rekeyed(np.zeros(n, np.uint8), PS4, 5, PS4, 6)
    nz = np.flatnonzero(ks)
    before = two(lib)
    M.verify_rekey_device(a.ptr + 3, a.ptr + 3, PS4, PS4, 5, 6, result=res.ptr, n=n)
    res.sync()
    assert triple(M.verify_results(res.ptr)[0]) == (nz.size, int(nz[0]), n) and two(lib) - before == 1
    # ... and a partial overlap
    diff = np.flatnonzero(data[3:3 + n] != rekeyed(data[4:4 + n], PS3, 0, PS4, 0))
    M.verify_rekey_device(a.ptr + 3, a.ptr + 4, PS3, PS4, result=res.ptr, n=n)
    res.sync()
    assert triple(M.verify_results(res.ptr)[0]) == (diff.size, int(diff[0]), n)
    assert np.array_equal(a.download(), data)
    for b in (eb, sb, a, res):
        b.free()


def test_forty_entry_batch_takes_one_init_and_one_launch_per_started_group(lib):
    rng = np.random.default_rng(40)
    sizes = [int(x) for x in rng.integers(1, CHUNK + 100, size=40)]
    for i in (0, 7, 39):
        sizes[i] = 0
    same = {2, 7, 9, 10, 25, 31}  # coinciding streams (7 is empty): 5 launches' worth of one group
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
    offs_from = [o + (i << 33) for i, o in enumerate(src_offs)]
    offs_to = [f + (PERIOD * (i % 2) if i in same else 3 + i) for i, f in enumerate(offs_from)]
    image = np.zeros(at + 16, np.uint8)
    for s, o, q, f, t in zip(sizes, src_offs, e_offs, offs_from, offs_to):
        image[q:q + s] = rekeyed(plain[o:o + s], PS4, f, PS4, t)
    want = [(0, NONE, s) for s in sizes]
    for i, js in ((3, [0]), (20, [sizes[20] - 1]), (33, [sizes[33] // 2, sizes[33] // 2 + 1]), (9, [1])):
        for j in js:
            image[e_offs[i] + j] ^= 1
        want[i] = (len(js), js[0], sizes[i])
    exp = M.DeviceBuffer(at + 16)
    exp.upload(image)
    res = Res(lib, 41)
    inits, comp, ident = lib.modgpu_shim_verify_inits(), two(lib), one(lib, (2, 3))
    M.verify_rekey_batch_device([exp.ptr + q for q in e_offs], [part.ptr + 3 + o for o in src_offs], sizes, PS4, PS4, res.ptr, offs_from=offs_from,
                                offs_to=offs_to)
    res.sync()
    # 37 non-empty: 32 with two streams (16 + 16) and 5 whose streams coincide
    assert lib.modgpu_shim_verify_inits() - inits == 1 and two(lib) - comp == 2 and one(lib, (2, 3)) - ident == 1
    got = [triple(r) for r in M.verify_results(res.ptr, 40)]
    assert got == want
    assert np.all(res.raw(32, 32 * 40) == 0xEE), "the result behind the last entry's was written"
    assert np.array_equal(exp.download(), image) and np.array_equal(part.download(part_n, offset=3), plain)
    # NULL offsets mean 0 for every entry; an empty batch queues nothing
    exp.upload(rekeyed(plain[:1000], PS3, 0, PS4, 0))
    M.verify_rekey_batch_device([exp.ptr], [part.ptr + 3], [1000], PS3, PS4, res.ptr)
    res.sync()
    assert triple(M.verify_results(res.ptr)[0]) == (0, NONE, 1000)
    inits = lib.modgpu_shim_verify_inits()
    M.verify_rekey_batch_device([], [], [], PS3, PS4, 0)
    assert lib.modgpu_shim_verify_inits() == inits
    for b in (part, exp, res):
        b.free()


def test_invalid_results_are_refused_before_anything_is_queued(lib):
    a, res = M.DeviceBuffer(256), Res(lib, 2)
    host = np.zeros(64, np.uint8)
    inits, comp, plain = lib.modgpu_shim_verify_inits(), two(lib), one(lib)

    def code(fn, *args, **kw):
        with pytest.raises(M.ModGpuError) as e:
            fn(*args, **kw)
        return e.value.code

    vr, vb = M.verify_rekey_device, M.verify_rekey_batch_device
    assert code(vr, a.ptr, a.ptr + 100, PS3, PS4, result=res.ptr + 4, n=10) == 1         # misaligned
    assert code(vr, a.ptr, a.ptr + 100, PS3, PS4, result=host.ctypes.data, n=10) == 1    # not device memory
    assert code(vr, a.ptr, a.ptr + 100, PS3, PS4, result=res.ptr + 40, n=10) == 1        # runs off the allocation
    assert code(vr, a.ptr, a.ptr + 100, PS3, PS4, result=a.ptr, n=10) == 1               # memory the runtime does not report as device memory
    assert code(vr, a.ptr, a.ptr + 100, PS3, PS4, result=res.ptr, device=1, n=10) == 1   # another device's memory
    assert code(vr, a.ptr, a.ptr + 100, 0, PS4, result=host.ctypes.data, n=10) == 1      # ... on the degenerate routes too
    assert code(vr, a.ptr, a.ptr + 100, PS4, PS4, result=host.ctypes.data, n=10) == 1
    assert code(vr, 0, a.ptr, PS3, PS4, result=res.ptr, n=10) == 1
    assert code(vr, a.ptr, 0, PS3, PS4, result=res.ptr, n=10) == 1
    assert code(vb, [a.ptr, a.ptr], [a.ptr, a.ptr], [1, 1], PS3, PS4, res.ptr + 32) == 1   # two results, room for one
    assert code(vb, [a.ptr, 0], [a.ptr, a.ptr], [1, 1], PS3, PS4, res.ptr) == 1
    assert M.lib().modgpu_verify_rekey_batch_device(None, None, None, None, None, -1, 1, 2, None, -1, None) == 1
    assert M.lib().modgpu_verify_rekey_batch_device(None, None, None, None, None, 2, 1, 2, None, -1, None) == 1
    assert code(M.time_verify_rekey_device, a.ptr, a.ptr + 100, 10, PS3, PS4, res.ptr + 4) == 1
    assert lib.modgpu_shim_verify_inits() == inits and two(lib) == comp and one(lib) == plain
    vr(0, 0, PS3, PS4, result=res.ptr + 32, n=0)  # n == 0 with NULL buffers: still a result, from the init launch alone
    res.sync()
    assert triple(M.verify_results(res.ptr + 32)[0]) == (0, NONE, 0) and np.all(res.raw(32, 0) == 0xEE)
    assert lib.modgpu_shim_verify_inits() == inits + 1 and two(lib) == comp and M.last_launch()["variant"] == 10
    assert M.time_verify_rekey_device(a.ptr, a.ptr + 100, 10, PS3, PS4, res.ptr, iters=3) >= 0.0
    assert lib.modgpu_shim_verify_inits() == inits + 4 and two(lib) == comp + 3
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
                img = rekeyed(src, PS3, (t << 32) + k, PS4, 7 * t + k)
                if k % 2:
                    img[1000 * t + k] ^= 0x80
                eb.upload(img, offset=(3 * t + k) % 16)
                M.verify_rekey_device(eb.ptr + (3 * t + k) % 16, sb.ptr + t, PS3, PS4, (t << 32) + k, 7 * t + k, result=res.ptr, device=t,
                                      stream=h.value, n=n)
                res.sync(h.value)
                assert triple(M.verify_results(res.ptr, 1, device=t)[0]) == ((1, 1000 * t + k, n) if k % 2 else (0, NONE, n)), (t, k)
                assert M.last_launch()["variant"] == 12
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
