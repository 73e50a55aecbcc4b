"""Cases for the sanitizer builds of libmodgpu's host code: the VERIFY TABLE call (modgpu_verify_table_device & co.).

Not collected by a plain `pytest tests/`: tests/test_verify_table_cpu.py runs this file in a child process with MODGPU_LIB pointing at
_san/libmodgpu_asan.so or _san/libmodgpu_tsan.so and the matching runtime preloaded (the pattern of tests/san_rekey_table_cases.py).  In
those builds the three launches run on the CPU (tests/cpu_runtime_standin/standin_launch_verify_table.cpp): the plan reads the table
from "device" memory when it runs, the finish writes the search levels, compares the ragged edges and stores every result whole, the
stream finds every chunk's entry through the levels and compares it -- all inside the workspace layout the host planned, so the
sanitizers see every byte.  "Device memory" is what modgpu_shim_xfer_alloc hands out; every case compares results and summary with
numpy over host images and checks that neither arena changed."""
import ctypes
import os
import threading

import numpy as np
import pytest

import modulate_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not os.environ.get("MODGPU_LIB"), reason="runs only against a sanitizer build (tests/test_verify_table_cpu.py)")

CHUNK = 65536
KEYS = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, M.KEY_PS3, M.KEY_PS4, 1, 0x80000001]
SIZES = [0] + list(range(1, 18)) + [CHUNK - 1, CHUNK + 1, 2 * CHUNK + 7]
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    L = M.lib()
    assert M.testing_hooks() and M.device_count() == 8, "expects the shim build with MODGPU_SHIM_DEVICES=8"
    L.modgpu_shim_xfer_alloc.restype = ctypes.c_void_p
    L.modgpu_shim_xfer_alloc.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
    L.modgpu_shim_xfer_free.argtypes = [ctypes.c_void_p]
    L.modgpu_shim_verify_table_launches.restype = ctypes.c_ulonglong
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
    return [L.modgpu_shim_verify_table_launches(k) for k in range(3)]


class Case:
    """a table over a source arena of random bytes and a comparand arena made with the oracle, mismatches planted in every third entry"""

    def __init__(self, L, sizes, rng, device=0, dirty=3):
        k = len(sizes)
        off, cur = [], 64
        for i, s in enumerate(sizes):
            cur = ((cur + 15) & ~15) + i % 16
            off.append(cur)
            cur += s + int(rng.integers(1, 40))
        self.exp, self.sizes, self.off, self.device = Dev(L, cur + 64, device), sizes, off, device
        src_n = max(4 * CHUNK, max(sizes) + 64)
        self.src = Dev(L, src_n, device)
        self.src_img = rng.integers(0, 256, size=src_n, dtype=np.uint8)
        self.src.write(self.src_img)
        t = M.table(k)
        t["dst"] = [self.exp.ptr + o for o in off]
        t["src"] = [self.src.ptr + 16 * (i % 64) + (i // 16) % 16 for i in range(k)]
        t["n"] = sizes
        offs = rng.integers(0, 1 << 63, size=k, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=k, dtype=np.uint64)
        offs[::5] = (1 << 64) - 1 - np.arange(len(offs[::5]), dtype=np.uint64)
        t["stream_off"] = offs
        t["key"] = np.array([KEYS[int(x)] for x in rng.integers(0, len(KEYS), size=k)], dtype=np.uint32).view(np.int32)
        self.t = t
        clean = np.full(self.exp.n, 0x5A, np.uint8)
        for i, e in enumerate(t):
            n = int(e["n"])
            if n:
                seg = self.src_img[int(e["src"]) - self.src.ptr:][:n].copy()
                O.cycle_at(seg, int(e["key"]) & 0xFFFFFFFF, int(e["stream_off"]))
                clean[off[i]:off[i] + n] = seg
        img = clean.copy()
        for i in range(0, k, dirty):
            n = sizes[i]
            if n:
                head = min(n, (16 - ((self.exp.ptr + off[i]) & 15)) & 15)
                for p in {0, n - 1, max(head - 1, 0), min(head, n - 1), int(rng.integers(0, n)), min(n - 1, CHUNK - (self.exp.ptr + off[i] + head) % CHUNK + head)}:
                    img[off[i] + p] ^= np.uint8(1 + p % 200)
        self.exp.write(img)
        self.img = img
        want = np.zeros(k, dtype=M.VERIFY_RESULT_DTYPE)
        want["n"] = sizes
        want["first_mismatch"] = NONE
        for i in range(k):
            seg = img[off[i]:off[i] + sizes[i]] != clean[off[i]:off[i] + sizes[i]]
            if seg.any():
                want["mismatches"][i] = int(seg.sum())
                want["first_mismatch"][i] = int(np.argmax(seg))
        self.want = want
        self.res = Dev(L, 32 * k + 128, device)
        self.res.write(np.full(32 * k + 128, 0xA5, np.uint8))

    def summary(self):
        dirty = np.flatnonzero(self.want["mismatches"])
        return {"mismatches": int(self.want["mismatches"].sum()), "first_bad_entry": int(dirty[0]) if dirty.size else None, "entries": len(self.t)}

    def call(self, t=None, stream=None, ws=None):
        t = self.t if t is None else t
        tb = Dev(M.lib(), t.nbytes, self.device)
        tb.write(t.view(np.uint8))
        own = ws is None
        if own:
            ws = Dev(M.lib(), M.verify_table_workspace_bytes(len(t)), self.device)
        M.verify_table_device(tb.ptr, self.res.ptr + 64, ws.ptr, device=self.device, stream=stream, n=len(t))
        M.lib().modgpu_sync(self.device, ctypes.c_void_p(stream or 0))
        status = M.table_status(ws.ptr, device=self.device)
        summary = M.verify_table_summary(ws.ptr, device=self.device) if status is None else None
        tb.free()
        if own:
            ws.free()
        return status, summary

    def results(self):
        raw = self.res.read()
        assert (raw[:64] == 0xA5).all() and (raw[64 + 32 * len(self.t):] == 0xA5).all(), "guard bytes around the results were written"
        return raw[64:64 + 32 * len(self.t)].view(M.VERIFY_RESULT_DTYPE)

    def check(self, what=""):
        got = self.results()
        assert np.array_equal(got, self.want), (what, np.flatnonzero(got != self.want)[:5])
        assert np.array_equal(self.exp.read(), self.img) and np.array_equal(self.src.read(), self.src_img), (what, "an arena changed")

    def free(self):
        for b in (self.exp, self.src, self.res):
            b.free()


def test_parity_of_results_and_summary(lib):
    """A few hundred entries of every size of SIZES at all comparand phases, keys incl. 0, 0x7FFFFFFF, INT_MIN, -1 and both platform
    keys, offsets up to 2^64-1, every third entry dirty at its seams: results and summary equal numpy's, three launches, variant 11."""
    rng = np.random.default_rng(1)
    c = Case(lib, [SIZES[int(x)] for x in rng.integers(0, len(SIZES), size=400)], rng)
    before, st0 = launches(lib), M.path_stats()["gpu_launches"]
    status, summary = c.call()
    assert status is None and summary == c.summary() and summary["mismatches"] > 0
    assert [b - a for a, b in zip(before, launches(lib))] == [1, 1, 1] and M.path_stats()["gpu_launches"] - st0 == 3
    info = M.last_launch()
    assert info["variant"] == 11 and info["bytes"] == 0 and info["source_hash"] == M.verify_table_kernel_source_hash(), info
    c.check()
    c.free()


def test_host_tier_queues_nothing(lib):
    """Every tier-1 refusal: NULL / misaligned / host / other-device results, table and workspace, a short workspace, too many entries:
    MODGPU_ERR_INVALID before anything is queued; n_entries == 0 is a no-op."""
    rng = np.random.default_rng(4)
    c = Case(lib, [100, 200], rng)
    wb = M.verify_table_workspace_bytes(2)
    assert wb >= M.table_workspace_bytes(2) + 64
    tb, ws = Dev(lib, c.t.nbytes), Dev(lib, wb)
    tb.write(c.t.view(np.uint8))
    other = Dev(lib, max(wb, 64), device=1)
    host = np.zeros(wb // 8 + 8, np.uint64)
    L, r = lib, c.res.ptr + 64
    before, st0 = launches(lib), M.path_stats()["gpu_launches"]
    assert L.modgpu_verify_table_device(tb.ptr, 2, None, ws.ptr, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, 2, r + 4, ws.ptr, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, 2, host.ctypes.data, ws.ptr, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, 2, other.ptr, ws.ptr, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, 2, r, host.ctypes.data, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, 2, r, other.ptr, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(c.t.ctypes.data, 2, r, ws.ptr, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(None, 2, r, ws.ptr, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, 2, r, None, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, 2, r, ws.ptr, wb - 8, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, 2, r, ws.ptr, M.table_workspace_bytes(2), 0, None) == 1  # the cycle table's size is short
    assert L.modgpu_verify_table_device(tb.ptr + 4, 2, r, ws.ptr, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, 2, r, ws.ptr + 4, wb, 0, None) == 1
    assert L.modgpu_verify_table_device(tb.ptr, (1 << 22) + 1, r, ws.ptr, 1 << 40, 0, None) == 1
    assert L.modgpu_verify_table_device(None, 0, None, None, 0, 0, None) == 0
    assert launches(lib) == before and M.path_stats()["gpu_launches"] == st0
    assert (c.res.read() == 0xA5).all()
    assert M.verify_table_workspace_bytes(0) == 0 and M.verify_table_workspace_bytes((1 << 22) + 1) == 0
    assert L.modgpu_verify_table_device(tb.ptr, 2, r, ws.ptr, wb, 0, None) == 0
    L.modgpu_sync(0, None)
    c.check()
    for b in (tb, ws, other, c):
        b.free()


def test_device_tier_refusal_leaves_the_results_untouched(lib):
    """A NULL source, a NULL comparand, nonzero flags, an entry of 1 TiB: no result is written, the status names the lowest, the
    summary is refused; the next call on the same workspace runs clean."""
    rng = np.random.default_rng(3)
    c = Case(lib, [int(x) for x in rng.integers(0, 2 * CHUNK, size=1500)], rng)
    ws = Dev(lib, M.verify_table_workspace_bytes(1500))
    for bad_at, field, value in ((1200, "src", 0), (700, "dst", 0), (1025, "flags", 1), (3, "n", 1 << 40), (0, "flags", 1 << 31)):
        tb = c.t.copy()
        tb[field][bad_at] = value
        tb["flags"][1499] = 4
        status, _ = c.call(tb, ws=ws)
        assert status == bad_at, (field, bad_at)
        assert (c.res.read() == 0xA5).all(), field
        with pytest.raises(M.ModGpuError):
            M.verify_table_summary(ws.ptr, device=0)
    status, summary = c.call(ws=ws)
    assert status is None and summary == c.summary()
    c.check()
    ws.free()
    c.free()


def test_two_threads_separate_workspaces(lib):
    errors = []

    def worker(k):
        try:
            h = ctypes.c_void_p()
            assert lib.modgpu_shim_stream_create(ctypes.byref(h)) == 0 and h.value
            rng = np.random.default_rng(10 + k)
            for rep in range(3):
                c = Case(lib, [int(x) for x in rng.integers(0, 3 * CHUNK, size=40)], rng)
                status, summary = c.call(stream=h.value)
                assert status is None and summary == c.summary(), (k, rep)
                c.check((k, rep))
                c.free()
            lib.modgpu_shim_stream_destroy(h)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


def test_eight_devices(lib):
    rng = np.random.default_rng(6)
    for dev in range(8):
        c = Case(lib, [SIZES[int(x)] for x in rng.integers(0, len(SIZES), size=30)], rng, device=dev)
        status, summary = c.call()
        assert status is None and summary == c.summary(), dev
        c.check(dev)
        c.free()
