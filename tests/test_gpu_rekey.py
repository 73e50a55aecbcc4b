"""GPU: the rekey entry points (modgpu_rekey_device_to / modgpu_rekey_batch_device_to) against the CPU oracle.

expected = cycle_at(cycle_at(src, key_from, off_from), key_to, off_to).  Every single-call case checks the destination bytes, guard
bytes on both sides of the destination, and that the source is unchanged.  conftest.py sets MODGPU_REQUIRE_GPU=1 before the library
loads, so every byte compared here came from a kernel."""
import numpy as np
import pytest

from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

PS3, PS4 = 0xC64EED30, 0x90CFC0AB
KEYS = [PS4, PS3, 1, 0xFFFFFFFF, 0x80000000, 12345, (-127772) & 0xFFFFFFFF, 0xDEADBEEF]  # test_gpu_parity.py's
ZERO_KEYS = [0, 0x7FFFFFFF, 0x80000001]
CHUNK = 65536
GUARD = 64
EDGE_SIZES = [0, 1, 15, 16, 17, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5]


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


def expected(oracle, pt, kf, of, kt, ot):
    w = pt.copy()
    oracle.cycle_at(w, kf, of)
    oracle.cycle_at(w, kt, ot)
    return w


class Pair:
    """A source and a destination allocation, each with room for any phase and GUARD bytes on both sides."""

    def __init__(self, M, cap):
        self.src = M.DeviceBuffer(cap + 2 * GUARD + 16)
        self.dst = M.DeviceBuffer(cap + 2 * GUARD + 16)

    def run(self, M, oracle, pt, ps, pd, kf, of, kt, ot, want=None):
        n = pt.size
        s_off, d_off = GUARD + ps, GUARD + pd
        src_img = np.full(n + 2 * GUARD + 16, 0xA5, np.uint8)
        src_img[s_off:s_off + n] = pt
        dst_img = np.full(n + 2 * GUARD + 16, 0x5A, np.uint8)
        self.src.upload(src_img)
        self.dst.upload(dst_img)
        M.rekey_device_to(self.dst.ptr + d_off, self.src.ptr + s_off, kf, kt, of, ot, n=n)
        self.dst.sync()
        got = self.dst.download(n + 2 * GUARD, offset=d_off - GUARD)
        want = expected(oracle, pt, kf, of, kt, ot) if want is None else want
        assert np.array_equal(got[GUARD:GUARD + n], want), (n, ps, pd, hex(kf), of, hex(kt), ot)
        assert (got[:GUARD] == 0x5A).all() and (got[GUARD + n:] == 0x5A).all(), ("guard", n, ps, pd)
        assert np.array_equal(self.src.download(src_img.size), src_img), ("source changed", n, ps, pd)

    def free(self):
        self.src.free()
        self.dst.free()


def test_source_phases_at_edge_sizes(gpu, oracle):
    """PS3 -> PS4 at every source phase against destination phase 0, at the sizes where heads, tails and chunk edges meet, with offsets
    of other phases mod 16 (both forms of the kernel: (src - dst) mod 4 == 0 reads plain, the rest through the funnel)."""
    pair = Pair(gpu, max(EDGE_SIZES))
    rng = np.random.default_rng(7)
    for n in EDGE_SIZES:
        pt = rng.integers(0, 256, size=n, dtype=np.uint8)
        of, ot = 3, 22 + n % 16
        want = expected(oracle, pt, PS3, of, PS4, ot)
        for ps in range(16):
            pair.run(gpu, oracle, pt, ps, 0, PS3, of, PS4, ot, want=want)
            if n > 16:
                info = gpu.last_launch()
                assert info["variant"] == 7 and info["source_hash"] == gpu.rekey_kernel_source_hash(), info
                assert ("true" in info["kernel"]) == (ps % 4 != 0), info
    pair.free()


def test_keys_and_offsets(gpu, oracle):
    """test_gpu_parity.py's keys against each other; offsets that differ in phase mod 16, near 2^32 and near 2^63."""
    pair = Pair(gpu, 3 * CHUNK + 5)
    pt = oracle.splitmix_bytes(3 * CHUNK + 5, 3)
    for i, kf in enumerate(KEYS):
        kt = KEYS[(i + 3) % len(KEYS)]
        pair.run(gpu, oracle, pt, 5, 0, kf, i, kt, 7 * i + 1)
    for of, ot in (((1 << 32) - 17, 1 << 32), ((1 << 32) + 5, (1 << 32) - 1), ((1 << 63) - 9, 4), (3, (1 << 63) + 11), ((1 << 64) - 3, (1 << 63))):
        pair.run(gpu, oracle, pt, 9, 0, PS3, of, PS4, ot)
        pair.run(gpu, oracle, pt, 0, 7, PS4, of, PS4, ot)  # one key, moved to another offset: a relocation
    pair.free()


def test_alias_round_trip_and_degenerate_keys(gpu, oracle):
    n = 3 * CHUNK + 5
    pt = oracle.splitmix_bytes(n + 64, 12)
    a = gpu.DeviceBuffer(n + 64)
    a.upload(pt)
    gpu.rekey_device_to(a.ptr + 3, a.ptr + 3, PS3, PS4, 11, 40, n=n)
    a.sync()
    got = a.download()
    assert np.array_equal(got[3:3 + n], expected(oracle, pt[3:3 + n], PS3, 11, PS4, 40)) and np.array_equal(got[:3], pt[:3])
    assert gpu.last_launch()["variant"] == 7
    gpu.rekey_device_to(a.ptr + 3, a.ptr + 3, PS4, PS3, 40, 11, n=n)  # B -> A gives the input back
    a.sync()
    assert np.array_equal(a.download(), pt)
    a.free()
    # degenerate keystreams: the out-of-place call (variant 5) or a copy (no launch at all)
    pair = Pair(gpu, n)
    small = gpu.DeviceBuffer(64)
    for kf, of, kt, ot, variant in [(z, 9, PS4, 13, 5) for z in ZERO_KEYS] + [(PS3, 9, z, 13, 5) for z in ZERO_KEYS] + \
            [(0, 1, 0x80000001, 2, None), (PS3, 7, PS3, 7 + 0x7FFFFFFE, None)]:
        gpu.cycle_device(small.ptr, 16, 1)
        small.sync()
        mark = gpu.last_launch()
        launches = gpu.path_stats()["gpu_launches"]
        pair.run(gpu, oracle, pt[:n], 5, 0, kf, of, kt, ot)
        info = gpu.last_launch()
        if variant is None:
            assert info == mark and gpu.path_stats()["gpu_launches"] == launches, (kf, kt, info)
        else:
            assert info["variant"] == variant, (kf, kt, info)
    small.free()
    pair.free()


def test_batch_relocation_ps3_to_ps4(gpu, oracle):
    """Files laid into a PS3 part at one set of offsets are rekeyed, in ONE call of 40 entries, to PS4 at a new layout; the new part
    equals the new plaintext layout encrypted directly."""
    rng = np.random.default_rng(40)
    sizes = [int(x) for x in rng.integers(0, 3 * CHUNK, size=40)]
    sizes[7] = 0
    plain_files = [oracle.splitmix_bytes(s, 1000 + i) for i, s in enumerate(sizes)]
    old_offs, at = [], 0
    for i, s in enumerate(sizes):
        at += (7 * i) % 16
        old_offs.append(at)
        at += s
    old_layout = np.zeros(at + 16, np.uint8)
    for f, o in zip(plain_files, old_offs):
        old_layout[o:o + f.size] = f
    old_part = old_layout.copy()
    oracle.cycle_at(old_part, PS3, 0)
    new_offs, at = [], 0
    for i, s in enumerate(sizes[::-1]):  # the new layout: reversed order, other phases
        at += (5 * i + 3) % 16
        new_offs.append(at)
        at += s
    new_offs = new_offs[::-1]
    new_layout = np.zeros(at + 16, np.uint8)
    for f, o in zip(plain_files, new_offs):
        new_layout[o:o + f.size] = f
    direct = new_layout.copy()
    oracle.cycle_at(direct, PS4, 0)
    src, dst = gpu.DeviceBuffer(old_part.size), gpu.DeviceBuffer(direct.size)
    src.upload(old_part)
    dst.upload(np.zeros(direct.size, np.uint8))
    gpu.rekey_batch_device_to([dst.ptr + o for o in new_offs], [src.ptr + o for o in old_offs], sizes, PS3, PS4,
                              offs_from=old_offs, offs_to=new_offs)
    dst.sync()
    got = dst.download()
    for s, o in zip(sizes, new_offs):
        assert np.array_equal(got[o:o + s], direct[o:o + s]), o
    assert np.array_equal(src.download(), old_part)
    assert gpu.last_launch()["variant"] == 7
    src.free()
    dst.free()


def test_4gib_conversion_equals_the_two_pass_route(gpu):
    """A 4 GiB PS3 -> PS4 conversion through the work-queue shape, compared whole with the two-pass route (cycle_device_to under PS3,
    then cycle_device under PS4) computed on the GPU -- both routes are oracle-pinned by the other tests."""
    n = 4 << 30
    src, fused, two = gpu.DeviceBuffer(n), gpu.DeviceBuffer(n), gpu.DeviceBuffer(n)
    tile = np.random.default_rng(4).integers(0, 256, size=(16 << 20) + 13, dtype=np.uint8)
    for off in range(0, n, tile.size):
        src.upload(tile[:min(tile.size, n - off)], offset=off)
    gpu.rekey_device_to(fused.ptr, src.ptr, PS3, PS4, n=n)
    info = gpu.last_launch()
    gpu.cycle_device_to(two.ptr, src.ptr, n, PS3, 0)
    gpu.cycle_device(two.ptr, n, PS4, 0)
    two.sync()
    assert info["variant"] == 7 and info["bytes"] == n, info
    win = 256 << 20
    for off in range(0, n, win):
        assert np.array_equal(fused.download(win, offset=off), two.download(win, offset=off)), off
    for b in (src, fused, two):
        b.free()


def test_graph_replay_streams_and_pinned_source(gpu, oracle):
    """A captured rekey replays to the eager result; eager calls on four streams at once are each right; a page-locked source works."""
    n = (2 << 20) + 77
    pt = oracle.splitmix_bytes(n, 21)
    want = expected(oracle, pt, PS3, 5, PS4, 9)
    src, dst = gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(n + 16)
    src.upload(pt, offset=3)
    st = Stream()
    with Graph.capture(st) as g:
        gpu.rekey_device_to(dst.ptr, src.ptr + 3, PS3, PS4, 5, 9, n=n, stream=st.handle)
    for k in range(2):
        dst.upload(np.zeros(n + 16, np.uint8))
        g.launch(st)
        st.sync()
        assert np.array_equal(dst.download(n), want), ("graph replay", k)
    g.destroy()
    st.destroy()
    src.free()
    dst.free()

    streams = [Stream() for _ in range(4)]
    bufs = [(gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(n + 16)) for _ in streams]
    pts = [oracle.splitmix_bytes(n, 50 + i) for i in range(4)]
    for i, (s, d) in enumerate(bufs):
        s.upload(pts[i], offset=i)
    for i, (st, (s, d)) in enumerate(zip(streams, bufs)):
        gpu.rekey_device_to(d.ptr + 2 * i, s.ptr + i, PS3, PS4, i, 3 * i, n=n, stream=st.handle)
    for i, (st, (s, d)) in enumerate(zip(streams, bufs)):
        st.sync()
        assert np.array_equal(d.download(n, offset=2 * i), expected(oracle, pts[i], PS3, i, PS4, 3 * i)), i
        s.free()
        d.free()
        st.destroy()

    pb = gpu.PinnedBuffer(n + 8)
    pb.array[:] = 0
    pb.array[5:5 + n] = pt
    d = gpu.DeviceBuffer(n)
    gpu.rekey_device_to(d.ptr, pb.ptr + 5, PS3, PS4, 5, 9, n=n)
    d.sync()
    assert np.array_equal(d.download(), want)
    d.free()
    pb.free()


def test_both_launch_shapes(gpu, oracle):
    """The work-queue grid and one workgroup per CU (testing flavour) give the same bytes."""
    with gpu.testing_flavour():
        n = (64 << 20) + 21
        pt = oracle.splitmix_bytes(n, 8)
        want = expected(oracle, pt, PS3, 0, PS4, 17)
        src, dst = gpu.DeviceBuffer(n + 16), gpu.DeviceBuffer(n + 16)
        src.upload(pt, offset=5)
        grids = {}
        try:
            for form in ("queue", "all"):
                gpu.debug_set_rekey_form(form)
                dst.upload(np.zeros(n + 16, np.uint8))
                gpu.rekey_device_to(dst.ptr, src.ptr + 5, PS3, PS4, 0, 17, n=n)
                dst.sync()
                grids[form] = gpu.last_launch()["grid"]
                assert np.array_equal(dst.download(n), want), form
        finally:
            gpu.debug_set_rekey_form(None)
            src.free()
            dst.free()
        assert grids["queue"] < grids["all"], grids
