"""GPU: modgpu_rekey_move_device -- rekey with memmove rules, any overlap of destination and source -- against the CPU oracle.

The model is the oracle applied to a host copy: the source bytes as they were, XORed with both keystreams (computed ONCE per key, from
one base offset, and sliced), put in place in a copy of the arena.  Every case runs in one arena whose payload is surrounded by 0xA5
guard bands, and the WHOLE window of the arena is compared, guards and the source bytes outside the destination included.  After every
case modgpu_move_status is OK.  The matrix runs in the testing flavour with the body launch's grid forced to 4, so that the 40 chunks
of the largest size make every workgroup draw many tickets and wait for its neighbours.  conftest.py sets MODGPU_REQUIRE_GPU=1 before
the library loads, so every byte compared here came from a kernel (or a device-to-device copy the call queued)."""
import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
CHUNK = 65536
G = 256                                   # guard bytes on either side of the payload
BIG = (2 << 20) + (512 << 10) + 77        # 40 chunks and 77 bytes
SIZES = [1, 15, 17, 65535, 65537, 131071, 131073, BIG]
BASE = (1 << 32) + 12345                  # where the precomputed keystreams start: 64-bit offsets, a phase of its own
SPAN = 3 * BIG + (1 << 20)                # bytes of keystream kept per key
MID = BIG                                 # the compaction pair's off_from, counted from BASE: room for off_to = off_from -+ d
# (name, key_from, key_to, off_from - BASE, off_to - BASE or None = off_from -+ d)
KEY_PAIRS = [("ps3->ps4", PS3, PS4, 3, 22), ("compaction", PS4, PS4, MID, None), ("plain", PS3, PS3, 77, 77),
             ("from-identity", 0, PS4, 5, 9), ("to-identity", PS3, 0x7FFFFFFF, 5, 9), ("both-identity", 0, 0x80000001, 1, 2)]


def shifts(n):
    return [d for d in [1, 3, 4, 15, 16, 17, 4096] + list(range(65532, 65541)) + [3 * CHUNK + 5, n - 1] if 0 < d < n]


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


@pytest.fixture(scope="module")
def streams(oracle):
    """the keystream bytes of both keys from BASE on, once for every test of the module (read-only); a zero key's are zero"""
    ks = {}
    for key in (PS3, PS4):
        z = np.zeros(SPAN, np.uint8)
        oracle.cycle_at(z, key, BASE)
        z.setflags(write=False)
        ks[key] = z
    zero = np.zeros(SPAN, np.uint8)
    zero.setflags(write=False)
    return lambda key: ks.get(key, zero)


@pytest.fixture(scope="module")
def payload(oracle):
    p = oracle.splitmix_bytes(2 * BIG + 64, 31)
    p.setflags(write=False)
    return p


class Arena:
    """Device memory whose offset 0 (self.base) lies on a 64 KiB boundary with room below for the guard."""

    def __init__(self, M, cap):
        self.buf = M.DeviceBuffer(cap + 3 * CHUNK)
        self.at = (-self.buf.ptr) % CHUNK + CHUNK  # offset of `base` inside the buffer
        self.base = self.buf.ptr + self.at
        self.ws = M.DeviceBuffer(M.move_workspace_bytes(cap))

    def case(self, M, streams, payload, lo, d, up, n, pair):
        """payload in [lo, lo + d + n) counted from base, 0xA5 around it; moved down (dst = lo, src = lo + d) or up"""
        name, kf, kt, of, ot = pair
        dst, src = (lo + d, lo) if up else (lo, lo + d)
        ot = of + (d if up else -d) if ot is None else ot
        img = np.full(2 * G + d + n, 0xA5, np.uint8)
        img[G:G + d + n] = payload[:d + n]
        self.buf.upload(img, offset=self.at + lo - G)
        want = img.copy()
        s0, d0 = G + src - lo, G + dst - lo
        want[d0:d0 + n] = img[s0:s0 + n] ^ streams(kf)[of:of + n] ^ streams(kt)[ot:ot + n]
        M.rekey_move_device(self.base + dst, self.base + src, n, kf, kt, BASE + of, BASE + ot, self.ws)
        self.buf.sync()
        assert M.move_status(self.ws) is None, (name, n, lo, d, up)
        got = self.buf.download(img.size, offset=self.at + lo - G)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError((name, "n", n, "lo", lo, "d", d, "up", up, "first/last/count of differing bytes (window offsets; payload starts at G)",
                                  int(bad[0]), int(bad[-1]), bad.size))

    def free(self):
        self.buf.free()
        self.ws.free()


@pytest.mark.parametrize("n", SIZES)
def test_matrix_at_a_grid_of_4(gpu, streams, payload, n):
    """every shift in both directions x every destination phase x every pair of keys, at one size"""
    with gpu.testing_flavour():
        gpu.debug_set_move_grid(4)
        arena = Arena(gpu, 2 * BIG + 2 * CHUNK)
        try:
            for d in shifts(n):
                for up in (False, True):
                    for at in (0, 12345):
                        for ph in (0, 1, 7):
                            for pair in KEY_PAIRS:
                                arena.case(gpu, streams, payload, at + ph, d, up, n, pair)
        finally:
            gpu.debug_set_move_grid(0)
            arena.free()


def test_shipped_grid_past_the_first_tickets(gpu, oracle):
    """48 MiB + 77 bytes at the shipped grid: 768 chunks, more than two per workgroup of any grid the device holds, shifted by 65 537
    down and up (the funnel form; every chunk waits for two others)."""
    n, d = (48 << 20) + 77, 65537
    pt = oracle.splitmix_bytes(n + d, 48)
    ks = np.zeros(n, np.uint8)
    oracle.cycle_at(ks, PS3, 11)
    kt = np.zeros(n, np.uint8)
    oracle.cycle_at(kt, PS4, 40)
    ks ^= kt
    arena = Arena(gpu, n + d + 2 * CHUNK)
    try:
        for up in (False, True):
            lo = 12345 + 7
            dst, src = (lo + d, lo) if up else (lo, lo + d)
            img = np.full(2 * G + d + n, 0xA5, np.uint8)
            img[G:G + d + n] = pt
            arena.buf.upload(img, offset=arena.at + lo - G)
            want = img.copy()
            want[G + dst - lo:G + dst - lo + n] = img[G + src - lo:G + src - lo + n] ^ ks
            gpu.rekey_move_device(arena.base + dst, arena.base + src, n, PS3, PS4, 11, 40, arena.ws)
            arena.buf.sync()
            info = gpu.last_launch()
            assert gpu.move_status(arena.ws) is None
            assert info["variant"] == 14 and info["bytes"] == n and 4 < info["grid"] <= 256 and "true" in info["kernel"], info
            assert np.array_equal(arena.buf.download(img.size, offset=arena.at + lo - G), want), ("up" if up else "down")
    finally:
        arena.free()


def test_disjoint_and_exact_alias_are_the_rekey_call(gpu, payload):
    """ranges that do not meet, and dst == src, give modgpu_rekey_device_to's bytes (and its launch: variant 7)"""
    n = 3 * CHUNK + 5
    arena = Arena(gpu, 4 * n)
    ref = gpu.DeviceBuffer(4 * n)
    try:
        for dst, src in ((7, 7 + n), (7 + n, 7), (2 * n, 3), (5, 5)):
            img = payload[:4 * n]
            arena.buf.upload(img, offset=arena.at)
            ref.upload(img)
            gpu.rekey_move_device(arena.base + dst, arena.base + src, n, PS3, PS4, 11, 40, arena.ws)
            arena.buf.sync()
            assert gpu.last_launch()["variant"] == 7 and gpu.move_status(arena.ws) is None
            gpu.rekey_device_to(ref.ptr + dst, ref.ptr + src, PS3, PS4, 11, 40, n=n)
            ref.sync()
            assert np.array_equal(arena.buf.download(4 * n, offset=arena.at), ref.download()), (dst, src)
    finally:
        arena.free()
        ref.free()


def test_captured_call_replayed_twice(gpu, streams, payload):
    """a captured move replays: two replays equal the model applied twice (the workspace is reset inside the graph)"""
    n, d, lo = 5 * CHUNK + 33, 65537, 12345 + 1
    arena = Arena(gpu, n + d + 2 * CHUNK)
    st = Stream()
    try:
        img = np.full(2 * G + d + n, 0xA5, np.uint8)
        img[G:G + d + n] = payload[:d + n]
        arena.buf.upload(img, offset=arena.at + lo - G)
        with Graph.capture(st) as g:
            gpu.rekey_move_device(arena.base + lo, arena.base + lo + d, n, PS3, PS4, BASE + 3, BASE + 22, arena.ws, stream=st.handle)
        want = img.copy()
        for k in range(2):
            want[G:G + n] = want[G + d:G + d + n] ^ streams(PS3)[3:3 + n] ^ streams(PS4)[22:22 + n]
            g.launch(st)
            st.sync()
            assert gpu.move_status(arena.ws) is None
            assert np.array_equal(arena.buf.download(img.size, offset=arena.at + lo - G), want), ("replay", k)
        g.destroy()
    finally:
        st.destroy()
        arena.free()


def test_launch_counts_and_last_launch(gpu, payload):
    """gpu_launches counts each kernel launch -- the pieces' (if there are any) and the body's (if there is one) --, and
    modgpu_last_launch reports the body launch as variant 14 with bytes = n; a range without a body goes through scratch in one
    ordinary rekey launch (variant 7)."""
    with gpu.testing_flavour():
        gpu.debug_set_move_grid(4)
        arena = Arena(gpu, BIG + 4 * CHUNK)
        try:
            arena.buf.upload(payload[:BIG + 2 * CHUNK], offset=arena.at)
            # (dst offset from a chunk boundary, n, shift) -> launches, variant, funnel
            for lo, n, d, launches, variant in ((12345, BIG, 5, 2, 14), (0, 10 * CHUNK, 4, 1, 14), (0, 10 * CHUNK + 3, CHUNK, 2, 14), (100, 1000, 7, 1, 7),
                                                (CHUNK - 16, 31, 1, 1, 7)):
                before = gpu.path_stats()["gpu_launches"]
                gpu.rekey_move_device(arena.base + lo, arena.base + lo + d, n, PS3, PS4, 0, 0, arena.ws)
                arena.buf.sync()
                info = gpu.last_launch()
                assert gpu.path_stats()["gpu_launches"] - before == launches, (lo, n, d)
                assert info["variant"] == variant and info["source_hash"] == gpu.rekey_kernel_source_hash(), info
                if variant == 14:
                    assert info["bytes"] == n and info["grid"] == 4 and info["block"] == 1024 and ("true" in info["kernel"]) == (d % 4 != 0), info
                assert gpu.move_status(arena.ws) is None
            # a forced grid is never more than there are chunks (40 and a cut one) ...
            gpu.debug_set_move_grid(4096)
            gpu.rekey_move_device(arena.base, arena.base + 5, BIG, PS3, PS4, 0, 0, arena.ws)
            arena.buf.sync()
            assert gpu.last_launch()["grid"] == 41, gpu.last_launch()
            # ... and, with chunks to spare (320), capped at what the device holds at once: one 1024-thread workgroup of this kernel
            # per CU, 256 on MI355X (a partitioned device has fewer CUs)
            big = Arena(gpu, 20 << 20)
            try:
                gpu.rekey_move_device(big.base, big.base + 5, 20 << 20, PS3, PS4, 0, 0, big.ws)
                big.buf.sync()
                assert 32 <= gpu.last_launch()["grid"] <= 256 and gpu.move_status(big.ws) is None, gpu.last_launch()
            finally:
                big.free()
            # DeviceBuffer.move: a plain memmove inside one buffer, with a workspace of its own
            img = payload[:4 * CHUNK]
            arena.buf.upload(img, offset=arena.at)
            arena.buf.move(arena.at + 1, arena.at + 70001, 2 * CHUNK)
            want = img.copy()
            want[1:1 + 2 * CHUNK] = img[70001:70001 + 2 * CHUNK]
            assert np.array_equal(arena.buf.download(4 * CHUNK, offset=arena.at), want)
        finally:
            gpu.debug_set_move_grid(0)
            arena.free()
