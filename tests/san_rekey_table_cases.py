"""Cases for the sanitizer builds of libmodgpu's host code: the REKEY TABLE call (modgpu_rekey_table_device & co.).

Not collected by a plain `pytest tests/`: tests/test_rekey_table_cpu.py runs this file in a child process with MODGPU_LIB pointing at
_san/libmodgpu_asan.so or _san/libmodgpu_tsan.so and the matching runtime preloaded (the pattern of tests/san_table_cases.py).  In those
builds the three launches run on the CPU (tests/cpu_runtime_standin/standin_launch_rekey_table.cpp): the plan reads the table from
"device" memory when it runs, the finish writes the search levels and the ragged edges, the stream finds every chunk's entry through the
levels and rekeys it -- all inside the workspace layout the host planned, so the sanitizers see every byte.  "Device memory" is what
modgpu_shim_xfer_alloc hands out (the stand-in's record of device allocations); every case compares whole arenas with the oracle."""
import ctypes
import os
import threading

import numpy as np
import pytest

import modulate_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not os.environ.get("MODGPU_LIB"), reason="runs only against a sanitizer build (tests/test_rekey_table_cpu.py)")

CHUNK = 65536
KEYS = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, M.KEY_PS3, M.KEY_PS4, 1, 0x80000001]
SIZES = [0] + list(range(1, 16)) + [16, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 7]


@pytest.fixture(scope="module")
def lib():
    L = M.lib()
    assert M.testing_hooks() and M.device_count() == 8, "expects the shim build with MODGPU_SHIM_DEVICES=8"
    L.modgpu_shim_xfer_alloc.restype = ctypes.c_void_p
    L.modgpu_shim_xfer_alloc.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
    L.modgpu_shim_xfer_free.argtypes = [ctypes.c_void_p]
    L.modgpu_shim_rekey_table_launches.restype = ctypes.c_ulonglong
    return L


class Dev:
    """a "device" allocation of the stand-in (host memory it knows as device memory of `device`)"""

    def __init__(self, L, n, device=0):
        self.L, self.n = L, n
        self.ptr = L.modgpu_shim_xfer_alloc(max(n, 1), device)
        assert self.ptr

    def write(self, a, off=0):
        a = np.ascontiguousarray(a)
        ctypes.memmove(self.ptr + off, a.ctypes.data, a.nbytes)

    def read(self, n=None, off=0):
        n = self.n - off if n is None else n
        out = np.empty(n, np.uint8)
        ctypes.memmove(out.ctypes.data, self.ptr + off, n)
        return out

    def free(self):
        self.L.modgpu_shim_xfer_free(self.ptr)


def launches(L):
    return [L.modgpu_shim_rekey_table_launches(k) for k in range(3)]


def build(L, sizes, rng, phases=None, device=0, in_place=()):
    """a table over a source arena of random bytes and a destination arena of 0x5A; destinations disjoint with gaps"""
    k = len(sizes)
    dst_off, cur = [], 64
    for i, s in enumerate(sizes):
        if phases is not None:
            cur = ((cur + 15) & ~15) + phases[i][0]
        dst_off.append(cur)
        cur += s + int(rng.integers(1, 40))
    dst = Dev(L, cur + 64, device)
    src_n = max(4 * CHUNK, max(sizes) + 64)
    src = Dev(L, src_n, device)
    src_img = rng.integers(0, 256, size=src_n, dtype=np.uint8)
    src.write(src_img)
    dst.write(np.full(dst.n, 0x5A, np.uint8))
    t = M.rekey_table(k)
    t["dst"] = [dst.ptr + o for o in dst_off]
    if phases is not None:
        t["src"] = [src.ptr + 16 * (i % 64) + phases[i][1] for i in range(k)]
    else:
        t["src"] = [src.ptr + int(rng.integers(0, src_n - s + 1)) for s in sizes]
    t["n"] = sizes
    for f in ("off_from", "off_to"):
        offs = rng.integers(0, 1 << 63, size=k, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=k, dtype=np.uint64)
        offs[::5] = (1 << 64) - 1 - np.arange(len(offs[::5]), dtype=np.uint64)
        t[f] = offs
    for f in ("key_from", "key_to"):
        t[f] = np.array([KEYS[int(x)] for x in rng.integers(0, len(KEYS), size=k)], dtype=np.uint32).view(np.int32)
    same = np.arange(k) % 9 == 4  # the same key at offsets equal mod the period: a copy
    t["key_to"][same] = t["key_from"][same]
    t["off_to"][same] = t["off_from"][same] % np.uint64(0x7FFFFFFE) + np.uint64(0x7FFFFFFE)
    for i in in_place:
        t["src"][i] = t["dst"][i]
    return t, src, dst, src_img


def expected(t, src, dst, src_img, before=None):
    want = np.full(dst.n, 0x5A, np.uint8) if before is None else before.copy()
    for e in t:
        n = int(e["n"])
        if not n:
            continue
        d = int(e["dst"]) - dst.ptr
        seg = want[d:d + n].copy() if int(e["src"]) == int(e["dst"]) else src_img[int(e["src"]) - src.ptr:][:n].copy()
        O.cycle_at(seg, int(e["key_from"]) & 0xFFFFFFFF, int(e["off_from"]))
        O.cycle_at(seg, int(e["key_to"]) & 0xFFFFFFFF, int(e["off_to"]))
        want[d:d + n] = seg
    return want


def call(L, t, device=0, stream=None, ws=None):
    tb = Dev(L, t.nbytes, device)
    tb.write(t.view(np.uint8))
    own = ws is None
    if own:
        ws = Dev(L, M.rekey_table_workspace_bytes(len(t)), device)
    M.rekey_table_device(tb.ptr, ws.ptr, device=device, stream=stream, n=len(t))
    M.lib().modgpu_sync(device, ctypes.c_void_p(stream or 0))
    status = M.table_status(ws.ptr, device=device)
    tb.free()
    if own:
        ws.free()
    return status


def test_random_tables_all_phases_keys_and_offsets(lib):
    """Every size of SIZES at all 16 x 16 destination / source phases, keys incl. 0, 0x7FFFFFFF, INT_MIN, -1 and both platform keys,
    offsets up to 2^64-1; in-place entries mixed in; whole destination arena compared (guards), sources unchanged."""
    rng = np.random.default_rng(1)
    n = 256 * 3
    sizes = [SIZES[int(x)] for x in rng.integers(0, len(SIZES), size=n)]
    phases = [(i % 16, (i // 16) % 16) for i in range(n)]
    t, src, dst, img = build(lib, sizes, rng, phases)
    M.rekey_table_validate(t)
    want = expected(t, src, dst, img)
    before = launches(lib)
    assert call(lib, t) is None
    assert [b - a for a, b in zip(before, launches(lib))] == [1, 1, 1]
    info = M.last_launch()
    assert info["variant"] == 9 and info["source_hash"] == M.rekey_table_kernel_source_hash(), info
    assert np.array_equal(dst.read(), want)
    assert np.array_equal(src.read(), img)
    # in place: every fourth entry cycles its own destination
    t2 = t.copy()
    t2["src"][::4] = t2["dst"][::4]
    pre = dst.read()
    want2 = expected(t2, src, dst, img, before=pre)
    assert call(lib, t2) is None
    assert np.array_equal(dst.read(), want2)
    src.free()
    dst.free()


def test_hundred_thousand_entries_in_three_launches(lib):
    rng = np.random.default_rng(2)
    sizes = [int(x) for x in rng.integers(0, 300, size=100000)]
    t, src, dst, img = build(lib, sizes, rng)
    want = expected(t, src, dst, img)
    before = launches(lib)
    st0 = M.path_stats()["gpu_launches"]
    assert call(lib, t) is None
    assert [b - a for a, b in zip(before, launches(lib))] == [1, 1, 1]
    assert M.path_stats()["gpu_launches"] - st0 == 3
    assert np.array_equal(dst.read(), want)
    src.free()
    dst.free()


def test_device_tier_refusal_writes_nothing(lib):
    """A NULL source, a NULL destination, nonzero flags, nonzero reserved, an entry of 1 TiB: the whole call writes nothing and the
    status names the lowest; the next call on the same workspace runs clean."""
    rng = np.random.default_rng(3)
    t, src, dst, img = build(lib, [int(x) for x in rng.integers(0, 2 * CHUNK, size=3000)], rng)
    ws = Dev(lib, M.rekey_table_workspace_bytes(len(t)))
    for bad_at, field, value in ((2500, "src", 0), (1700, "dst", 0), (1025, "flags", 1), (1030, "reserved", 7), (3, "n", 1 << 40), (0, "reserved", 1 << 31)):
        tb = t.copy()
        tb[field][bad_at] = value
        tb["flags"][2999] = 4
        assert call(lib, tb, ws=ws) == bad_at, (field, bad_at)
        assert np.array_equal(dst.read(), np.full(dst.n, 0x5A, np.uint8)), field
    assert call(lib, t, ws=ws) is None
    assert np.array_equal(dst.read(), expected(t, src, dst, img))
    ws.free()
    src.free()
    dst.free()


def test_two_threads_separate_workspaces(lib):
    errors = []

    def worker(k):
        try:
            h = ctypes.c_void_p()
            assert lib.modgpu_shim_stream_create(ctypes.byref(h)) == 0 and h.value
            rng = np.random.default_rng(10 + k)
            for rep in range(3):
                t, src, dst, img = build(lib, [int(x) for x in rng.integers(0, 3 * CHUNK, size=40)], rng)
                assert call(lib, t, stream=h.value) is None
                assert np.array_equal(dst.read(), expected(t, src, dst, img)), (k, rep)
                src.free()
                dst.free()
            lib.modgpu_shim_stream_destroy(h)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


def test_host_tier_queues_nothing(lib):
    """Memory the stand-in does not know as device memory of the call's device, a short or misaligned workspace, too many entries:
    MODGPU_ERR_INVALID before anything is queued."""
    rng = np.random.default_rng(4)
    t, src, dst, img = build(lib, [100, 200], rng)
    tb, ws = Dev(lib, t.nbytes), Dev(lib, M.rekey_table_workspace_bytes(2))
    tb.write(t.view(np.uint8))
    other = Dev(lib, M.rekey_table_workspace_bytes(2), device=1)
    host_ws = np.zeros(M.rekey_table_workspace_bytes(2) // 8 + 1, np.uint64)
    L = lib
    wb = M.rekey_table_workspace_bytes(2)
    before, st0 = launches(lib), M.path_stats()["gpu_launches"]
    assert L.modgpu_rekey_table_device(tb.ptr, 2, host_ws.ctypes.data, wb, 0, None) == 1
    assert L.modgpu_rekey_table_device(tb.ptr, 2, other.ptr, wb, 0, None) == 1
    assert L.modgpu_rekey_table_device(t.ctypes.data, 2, ws.ptr, wb, 0, None) == 1
    assert L.modgpu_rekey_table_device(tb.ptr, 2, ws.ptr, wb - 8, 0, None) == 1
    assert L.modgpu_rekey_table_device(tb.ptr + 4, 2, ws.ptr, wb, 0, None) == 1
    assert L.modgpu_rekey_table_device(tb.ptr, (1 << 22) + 1, ws.ptr, 1 << 40, 0, None) == 1
    assert L.modgpu_rekey_table_device(tb.ptr, 0, None, 0, 0, None) == 0
    assert launches(lib) == before and M.path_stats()["gpu_launches"] == st0
    assert np.array_equal(dst.read(), np.full(dst.n, 0x5A, np.uint8))
    assert L.modgpu_rekey_table_device(tb.ptr, 2, ws.ptr, wb, 0, None) == 0
    L.modgpu_sync(0, None)
    assert np.array_equal(dst.read(), expected(t, src, dst, img))
    for b in (tb, ws, other, src, dst):
        b.free()
