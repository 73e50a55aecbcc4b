"""GPU: the keystream arithmetic over its whole state domain, and its threshold states on every kernel family.

Every kernel of the library is a loop around one block of arithmetic: byte J of a 16-byte word is the word's first state times a^J,
folded to X = hi + lo31 and canonicalised by "+1 if X >= 2^31" (ks_word_carry and ks_word2_carry take the +1 from a carry-out, the
small shape's put_byte from X >> 31).  The generator has period P = 2^31 - 2 and meets every state once per period, so the states
at that threshold fall into a compared window of the other GPU files almost never (tests/test_keystream_domain_cpu.py says where
they did).  Here:

* the sweeps run the three implementations over P bytes at each of the 16 phases of stream against word: every (state, word
  position) pair, (2^31 - 2) x 16 inputs each, compared with the oracle's keystream byte for byte -- nothing sampled;
* the directed cases put the states 1, 2, m - 2 and m - 1 at chosen bytes (first word and head bytes, the 64 KiB chunk edge, last
  word and ragged tail) of a small buffer, for every kernel family: each translation unit compiles its own copy of a block between
  its own head, tail and funnel code.

tests/keystream_domain.py holds the shared helpers; nothing of the library takes part in an expected byte.  The file runs on
libmodgpu_testing.so (the same device code; it has the hooks that force a launch shape, a form or a grid)."""
import ctypes
import zlib

import numpy as np
import pytest

import keystream_domain as K

pytestmark = pytest.mark.gpu

P, M31, CHUNK, N = K.P, K.M, K.CHUNK, K.DIRECTED_N
G = 64                       # guard bytes on either side of a buffer under test
NONE = (1 << 64) - 1
KEEP = "modgpu_cycle_keep_kernel<4, 1024>"
MAIN = "modgpu_cycle_queue_kernel<4, 1024>"
ORD_KEY, ORD_OFF = 0x90CFC0AB, (1 << 40) + 77  # the "ordinary" stream of the two-key families
SLOT = 3 * CHUNK             # bytes of arena per table entry: the entry at a phase of its own, guards around it
# (destination phase, source phase): co-aligned at both phases, and the source at phase 3 (the funnel form) against both
COMBOS = ((0, 0), (5, 5), (0, 3), (5, 3))
PLACEMENTS = ("from", "to", "both")


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    with modgpu.testing_flavour():
        assert modgpu.testing_hooks() and modgpu.gpu_required()
        yield modgpu
    assert modgpu.active_flavour() == "shipped"


class Room:
    """Device memory whose offset 0 (self.base) lies on a 64 KiB boundary, with 64 KiB of room below it."""

    def __init__(self, M, cap):
        self.M = M
        try:
            self.buf = M.DeviceBuffer(cap + 3 * CHUNK)
        except M.ModGpuError as e:
            raise AssertionError(f"no device memory for {cap} bytes: {e}") from e
        self.at = (-self.buf.ptr) % CHUNK + CHUNK
        self.base = self.buf.ptr + self.at
        self.cap = cap
        assert self.base % CHUNK == 0

    def put(self, data, off=0):
        self.buf.upload(data, offset=self.at + off)

    def get(self, n, off=0):
        return self.buf.download(n, offset=self.at + off)

    def get_into(self, host_ptr, n, off=0):
        """n bytes from base + off into host memory at host_ptr (page-locked: a fast copy)"""
        rc = self.M.lib().modgpu_d2h(ctypes.c_void_p(host_ptr), ctypes.c_void_p(self.base + off), n, -1)
        assert rc == 0, self.M.lib().modgpu_last_error()

    def put_from(self, host_ptr, n, off=0):
        rc = self.M.lib().modgpu_h2d(ctypes.c_void_p(self.base + off), ctypes.c_void_p(host_ptr), n, -1)
        assert rc == 0, self.M.lib().modgpu_last_error()

    def free(self):
        self.buf.free()


# =====================================================================================================================================
# 1. the exhaustive sweeps
# =====================================================================================================================================
class Sweep:
    pass


@pytest.fixture(scope="module")
def sweep(gpu, oracle):
    """ks[0 : P + 64] of key 1 (the oracle's, built once); A (zeros) and B (scratch) of P + 64 bytes at 64 KiB-aligned addresses, their
    last 64 bytes guards; one page-locked host buffer of P bytes"""
    s = Sweep()
    s.ks = K.full_period_keystream(oracle, 1, 64)
    s.ks.setflags(write=False)
    s.a, s.b = Room(gpu, P + G), Room(gpu, P + G)
    try:
        s.pinned = gpu.PinnedBuffer(P)
    except gpu.ModGpuError as e:
        raise AssertionError(f"the host lacks the memory for a page-locked buffer of {P} bytes: {e}") from e
    assert s.pinned.pinned and s.pinned.ptr % 4096 == 0
    zeros = np.zeros(64 << 20, np.uint8)
    for o in range(0, P, zeros.size):
        s.a.put(zeros[:min(zeros.size, P - o)], o)
    for room in (s.a, s.b):
        room.put(np.full(G, 0xA5, np.uint8), P)
    yield s
    s.pinned.free()
    s.a.free()
    s.b.free()


def _guards(s, what):
    for name, room in (("A", s.a), ("B", s.b)):
        assert (room.get(G, P) == 0xA5).all(), f"{what}: the 64 guard bytes behind {name} were written"


def _same(oracle, got, want, index0, what):
    line = K.report_mismatch(oracle, got, want, 1, index0, word0=0)  # (64 KiB-aligned buffers: byte j sits at word position j mod 16)
    assert line is None, f"{what}: {line}"


@pytest.mark.parametrize("p", range(16))
def test_sweep_every_state_at_every_word_position(gpu, oracle, sweep, p):
    """One phase of the sweep: byte j of a buffer at a 64 KiB-aligned address has stream index p + j and word position j mod 16, so
    over p = 0..15 every (state, position) pair of the block is produced exactly once per implementation (n = P: a whole period).

    ALG 2, one stream: A (zeros) cycled in place under key 1 from offset p by what ships at this size (the work-queue kernel's copy
    with a resident slice) must be ks[p : p + P]; the restoring pass at the end runs the main work-queue kernel.  Two streams: rekeyed
    from (1, p) to (1, q), q = 16 + (5p + 3) mod 16, into B it must be ks[q : q + P]: q mod 16 runs over all residues as p does and
    q != p, so both streams of ks_word2_carry see every pair with the other stream elsewhere in its period.  ALG 1: A downloaded
    through the transfer kernel under (1, p) into page-locked memory must be all zero, and so must B after the forced small shape of
    modgpu_cycle_device under (1, q) -- that shape accepts n = P (a grid of 16 384 workgroups striding over it), and it runs on B, a
    verified copy of the keystream, instead of a third 2 GiB buffer.  Then A is cycled back: zero again for the next phase, which
    the last phase checks, so the involution is covered over the full domain too.  The guards behind A and B stay untouched."""
    s, q = sweep, 16 + (5 * p + 3) % 16
    pin = s.pinned.array
    # ALG 2, one stream
    s.a.buf.cycle(1, n=P, offset=s.a.at, stream_off=p)
    s.a.buf.sync()
    info = gpu.last_launch()
    assert info["variant"] == 2 and info["kernel"] in (KEEP, MAIN) and info["bytes"] == P and info["chunk_bytes"] == CHUNK, info
    assert info["kernel"] == (KEEP if gpu.keep_policy(P)[0] else MAIN), info
    s.a.get_into(s.pinned.ptr, P)
    _same(oracle, pin, s.ks[p:p + P], p, f"phase {p}, in place ({info['kernel']})")
    # the two-stream block
    gpu.rekey_device_to(s.b.base, s.a.base, 1, 1, p, q, n=P)
    s.b.buf.sync()
    info = gpu.last_launch()
    assert info["variant"] == 7 and info["bytes"] == P and info["source_hash"] == gpu.rekey_kernel_source_hash(), info  # no degenerate route
    s.b.get_into(s.pinned.ptr, P)
    _same(oracle, pin, s.ks[q:q + P], q, f"phase {p}, rekey to offset {q}")
    _guards(s, f"phase {p}, after the rekey")
    # ALG 1: the transfer kernel
    gpu.cycle_device_to_host(s.pinned, s.a.base, 1, stream_off=p)
    info = gpu.last_launch()
    assert info["variant"] == 6 and "modgpu_cycle_xfer_kernel<false" in info["kernel"] and info["bytes"] == P, info
    if not K.all_zero(pin):
        _same(oracle, pin, np.zeros(P, np.uint8), p, f"phase {p}, download through the transfer kernel")
    # ALG 1: the small shape
    gpu.debug_set_launch("small", 0)
    try:
        s.b.buf.cycle(1, n=P, offset=s.b.at, stream_off=q)
        s.b.buf.sync()
        info = gpu.last_launch()
    finally:
        gpu.debug_set_launch(None, 0)
    assert info["variant"] == 0 and info["kernel"].startswith("modgpu_cycle_kernel<1, 256,") and info["bytes"] == P, info
    s.b.get_into(s.pinned.ptr, P)
    if not K.all_zero(pin):
        _same(oracle, pin, np.zeros(P, np.uint8), q, f"phase {p}, small shape at offset {q}")
    # restore, through the other copy of the block
    gpu.debug_set_keep(gpu.KEEP_OFF, 1, 0)
    try:
        s.a.buf.cycle(1, n=P, offset=s.a.at, stream_off=p)
        s.a.buf.sync()
        info = gpu.last_launch()
    finally:
        gpu.debug_set_keep(0, 0, 0)
    assert info["variant"] == 2 and info["kernel"] == MAIN and info["bytes"] == P and info["source_hash"] == gpu.kernel_source_hash(), info
    _guards(s, f"phase {p}, at the end")
    if p == 15:
        s.a.get_into(s.pinned.ptr, P)
        if not K.all_zero(pin):
            _same(oracle, pin, np.zeros(P, np.uint8), p, "A after the last phase's restoring pass")


# =====================================================================================================================================
# 2. the threshold states, directed, on every kernel family
# =====================================================================================================================================
# A buffer under test starts `phase` bytes past a 64 KiB boundary (Room.base + phase, or a slot of the table arena + phase), so the
# positions of keystream_domain.DIRECTED_POSITIONS are the kernel's own first word, chunk edge and last word; G guard bytes lie on
# either side of it and are compared with it.
class Directed:
    pass


def build_directed(oracle):
    """The cases of keystream_domain.directed_cases() -- (state, position, offset, key) -- with, per case, the oracle's keystream over
    the buffer, the expected bytes of the plaintext under it, and their Adler-32; the same for the two-key families (the other stream
    ordinary, or the same state at the same byte of another offset's stream); and the in-place call's host-path edges.  Applying
    oracle.cycle_at twice is XORing both of its keystreams, which is how the two-key bytes are put together."""
    d = Directed()
    d.cases = K.directed_cases()
    n_pos, n_off = len(K.DIRECTED_POSITIONS), len(K.DIRECTED_OFFS)
    assert len({o % P for o in K.DIRECTED_OFFS}) == n_off and len(d.cases) == 4 * n_off * n_pos
    d.pt = oracle.splitmix_bytes(N, 0x7468726573)
    d.ks = np.empty((len(d.cases), N), np.uint8)
    for i, (state, pos, off, key) in enumerate(d.cases):
        assert oracle.state_at(key, off + pos) == state and off + N < (1 << 64)
        d.ks[i] = oracle.cycle_at(np.zeros(N, np.uint8), key, off)
        assert d.ks[i, pos] == ~state & 0xFF
    d.keys = np.array([c[3] for c in d.cases], np.int32)
    d.offs = np.array([c[2] for c in d.cases], np.uint64)
    d.pos = np.array([c[1] for c in d.cases], np.int64)
    d.want = d.pt[None, :] ^ d.ks
    d.adler = np.array([zlib.adler32(w) for w in d.want], np.uint32)
    d.pt_adler = zlib.adler32(d.pt)
    # two keys: the partner of a case is the case of the same state and position at the next offset of the list
    d.partner = np.array([(i // n_pos // n_off * n_off + (i // n_pos + 1) % n_off) * n_pos + i % n_pos for i in range(len(d.cases))])
    for i, j in enumerate(d.partner):
        assert d.cases[j][:2] == d.cases[i][:2] and d.cases[j][2] != d.cases[i][2] and d.cases[j][3] % M31 != d.cases[i][3] % M31
    ks_ord = oracle.cycle_at(np.zeros(N, np.uint8), ORD_KEY, ORD_OFF)
    d.want2 = {"from": d.want ^ ks_ord[None, :], "both": d.want ^ d.ks[d.partner]}
    d.want2["to"] = d.want2["from"]
    # host-path edges, on the in-place call: state 1 at an index = -1 (mod P) -- the exponent of key_for wraps to 0, the key is 1 --
    # in both sign forms of the key
    d.edges = []
    for pos in K.DIRECTED_POSITIONS:
        off = 3 * P - 1 - pos
        ks = oracle.cycle_at(np.zeros(N, np.uint8), 1, off)
        for neg in (False, True):
            key = K.key_for(1, off + pos, neg)
            assert key == (1 - M31 if neg else 1) and oracle.state_at(key, off + pos) == 1 and ks[pos] == 0xFE
            d.edges.append((1, pos, off, key, d.pt ^ ks))
    for a in (d.pt, d.ks, d.want, d.want2["from"], d.want2["both"]):
        a.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def directed(oracle):
    """build_directed's cases and expected bytes: built once, read-only"""
    return build_directed(oracle)


def two_keys(d, i, where):
    """(key_from, off_from, key_to, off_to) of case i with the threshold state in stream `where`"""
    _, _, off, key = d.cases[i]
    if where == "from":
        return key, off, ORD_KEY, ORD_OFF
    if where == "to":
        return ORD_KEY, ORD_OFF, key, off
    _, _, off2, key2 = d.cases[d.partner[i]]
    return key, off, key2, off2


def window(data, fill):
    img = np.full(data.size + 2 * G, fill, np.uint8)
    img[G:G + data.size] = data
    return img


def check_window(oracle, got, want_img, case, phase, what):
    """a downloaded window (guards, N bytes, guards) against its expected image; a mismatch names the byte, its state and its place"""
    if np.array_equal(got, want_img):
        return
    state, pos, off, key = case[:4]
    assert (got[:G] == want_img[:G]).all() and (got[G + N:] == want_img[G + N:]).all(), (what, "guard bytes written", state, pos, off)
    raise AssertionError((what, f"state {state:#x} placed at byte {pos}, offset {off}, key {key}, phase {phase}",
                          K.report_mismatch(oracle, got[G:G + N], want_img[G:G + N], key, off, word0=phase % 16)))


@pytest.mark.parametrize("shape", ("small", "large", "queue"))
def test_directed_in_place(gpu, oracle, directed, shape):
    """modgpu_cycle_device with each launch shape forced, at both phases: every case and the host-path edges (the key 1 reached through
    an exponent that wraps, and 1 - m, the negative int32 of the same residue; every fourth case of the main list has a negative key
    too).  Each call is undone by a second one: the plaintext is back at the end."""
    d = directed
    room = Room(gpu, N + G + 16)
    gpu.debug_set_launch(shape, 0)
    try:
        for phase in K.DIRECTED_PHASES:
            img = window(d.pt, 0xA5)
            room.put(img, phase - G)
            want = img.copy()
            for i, case in enumerate(d.cases + d.edges):
                _, _, off, key = case[:4]
                want[G:G + N] = d.want[i] if i < len(d.cases) else case[4]
                room.buf.cycle(key, n=N, offset=room.at + phase, stream_off=off)
                check_window(oracle, room.get(img.size, phase - G), want, case, phase, shape)
                info = gpu.last_launch()
                assert info["variant"] == {"small": 0, "large": 1, "queue": 2}[shape] and info["bytes"] == N, info
                room.buf.cycle(key, n=N, offset=room.at + phase, stream_off=off)
            assert np.array_equal(room.get(img.size, phase - G), img), ("the second pass did not give the plaintext back", shape, phase)
    finally:
        gpu.debug_set_launch(None, 0)
        room.free()


SRC_PHASES = (0, 3, 5)


def _src_room(gpu, d):
    """the plaintext in device memory once per source phase, three chunks apart: (the room, {phase: address})"""
    room = Room(gpu, 3 * SLOT)
    addr = {}
    for k, ph in enumerate(SRC_PHASES):
        room.put(window(d.pt, 0xA5), k * SLOT + ph - G)
        addr[ph] = room.base + k * SLOT + ph
    return room, addr


def _src_intact(room, d):
    for k, ph in enumerate(SRC_PHASES):
        assert np.array_equal(room.get(N + 2 * G, k * SLOT + ph - G), window(d.pt, 0xA5)), ("a source was written", ph)


def test_directed_out_of_place(gpu, oracle, directed):
    """modgpu_cycle_device_to: co-aligned at both destination phases, and the source at phase 3 read by both forms the family's own
    file forces (unaligned loads, the funnel)"""
    d = directed
    src, at = _src_room(gpu, d)
    dst = Room(gpu, N + G + 16)
    try:
        for pd, ps in COMBOS:
            for form in ((None,) if ps == pd else ("unaligned", "funnel")):
                gpu.debug_set_to_form(form)
                dst.put(np.full(N + 2 * G, 0x5A, np.uint8), pd - G)
                want = np.full(N + 2 * G, 0x5A, np.uint8)
                for i, case in enumerate(d.cases):
                    want[G:G + N] = d.want[i]
                    gpu.cycle_device_to(dst.base + pd, at[ps], N, case[3], case[2])
                    check_window(oracle, dst.get(want.size, pd - G), want, case, pd, ("out of place", pd, ps, form))
                    assert gpu.last_launch()["variant"] == 5
        _src_intact(src, d)
    finally:
        gpu.debug_set_to_form(None)
        src.free()
        dst.free()


@pytest.mark.parametrize("grid", (1, 3, 256, 0))
def test_directed_digest(gpu, oracle, directed, grid):
    """modgpu_digest_device, digest only (the source at phases 0, 5 and 3) and fused (every combination of phases), at the grids the
    family's own file forces: the record is zlib's Adler-32 of the oracle's bytes, and the fused call stores exactly those bytes"""
    d = directed
    src, at = _src_room(gpu, d)
    dst = Room(gpu, N + G + 16)
    rec = gpu.DeviceBuffer(32)
    gpu.debug_set_digest_grid(grid)
    try:
        for ps in SRC_PHASES:
            for i, case in enumerate(d.cases):
                gpu.digest_device(at[ps], case[3], case[2], None, rec, n=N)
                rec.sync()
                assert int(gpu.digest_results(rec)[1][0]) == d.adler[i], ("digest only", grid, ps, case)
                assert gpu.last_launch()["variant"] == 16
        for pd, ps in COMBOS:
            dst.put(np.full(N + 2 * G, 0x5A, np.uint8), pd - G)
            want = np.full(N + 2 * G, 0x5A, np.uint8)
            for i, case in enumerate(d.cases):
                want[G:G + N] = d.want[i]
                gpu.digest_device(at[ps], case[3], case[2], dst.base + pd, rec, n=N)
                rec.sync()
                assert int(gpu.digest_results(rec)[1][0]) == d.adler[i], ("fused", grid, pd, ps, case)
                check_window(oracle, dst.get(want.size, pd - G), want, case, pd, ("fused digest", pd, ps, grid))
        _src_intact(src, d)
    finally:
        gpu.debug_set_digest_grid(0)
        for b in (src, dst, rec):
            b.free()


def _verify_both_ways(gpu, verify, exp, pd, want, pos, rec, what):
    """the comparand `want` at phase pd of exp: 0 mismatches; with the byte at the threshold position flipped: exactly that index"""
    exp.put(want, pd)
    verify()
    rec.sync()
    r = gpu.verify_results(rec)[0]
    assert (int(r["mismatches"]), int(r["first_mismatch"]), int(r["n"])) == (0, NONE, N), (what, r)
    exp.put(want[pos:pos + 1] ^ np.uint8(0x01), pd + pos)
    verify()
    rec.sync()
    r = gpu.verify_results(rec)[0]
    assert (int(r["mismatches"]), int(r["first_mismatch"])) == (1, pos), (what, r)


@pytest.mark.parametrize("grid", (1, 3, 200, 0))
def test_directed_verify(gpu, directed, grid):
    """modgpu_verify_device against the oracle's bytes, at the grids the family's own file forces"""
    d = directed
    src, at = _src_room(gpu, d)
    exp = Room(gpu, N + G + 16)
    rec = gpu.DeviceBuffer(32)
    gpu.debug_set_verify_form(grid)
    try:
        for pd, ps in COMBOS:
            for i, (state, pos, off, key) in enumerate(d.cases):
                _verify_both_ways(gpu, lambda: gpu.verify_device(exp.base + pd, at[ps], key, off, rec, n=N), exp, pd, d.want[i], pos, rec,
                                  ("verify", grid, pd, ps, state, pos, off))
                assert gpu.last_launch()["variant"] == 10
    finally:
        gpu.debug_set_verify_form(0)
        for b in (src, exp, rec):
            b.free()


@pytest.mark.parametrize("form", ("queue", "all", None))
def test_directed_rekey(gpu, oracle, directed, form):
    """modgpu_rekey_device_to in the forms the family's own file forces: the threshold state in the stream that is removed (the other
    ordinary), in the one that is applied, and in both at the same byte"""
    d = directed
    src, at = _src_room(gpu, d)
    dst = Room(gpu, N + G + 16)
    gpu.debug_set_rekey_form(form)
    try:
        for pd, ps in COMBOS:
            dst.put(np.full(N + 2 * G, 0x5A, np.uint8), pd - G)
            want = np.full(N + 2 * G, 0x5A, np.uint8)
            for where in PLACEMENTS:
                for i, case in enumerate(d.cases):
                    kf, of, kt, ot = two_keys(d, i, where)
                    want[G:G + N] = d.want2[where][i]
                    gpu.rekey_device_to(dst.base + pd, at[ps], kf, kt, of, ot, n=N)
                    check_window(oracle, dst.get(want.size, pd - G), want, case, pd, ("rekey", form, where, pd, ps))
                    assert gpu.last_launch()["variant"] == 7
        _src_intact(src, d)
    finally:
        gpu.debug_set_rekey_form(None)
        src.free()
        dst.free()


@pytest.mark.parametrize("grid", (0, 1, 3))
def test_directed_verify_rekey(gpu, directed, grid):
    """modgpu_verify_rekey_device against the oracle's bytes, the threshold state in either stream and in both"""
    d = directed
    src, at = _src_room(gpu, d)
    exp = Room(gpu, N + G + 16)
    rec = gpu.DeviceBuffer(32)
    gpu.debug_set_verify_form(grid)
    try:
        for pd, ps in COMBOS:
            for where in PLACEMENTS:
                for i, (state, pos, off, key) in enumerate(d.cases):
                    kf, of, kt, ot = two_keys(d, i, where)
                    _verify_both_ways(gpu, lambda: gpu.verify_rekey_device(exp.base + pd, at[ps], kf, kt, of, ot, rec, n=N), exp, pd,
                                      d.want2[where][i], pos, rec, ("verify rekey", grid, where, pd, ps, state, pos, off))
                    assert gpu.last_launch()["variant"] == 12
    finally:
        gpu.debug_set_verify_form(0)
        for b in (src, exp, rec):
            b.free()


# (destination phase, source address minus destination address): the ranges overlap in all of them; the source co-aligned at both
# destination phases, and at phase 3 above the destination (moved down) and below it (moved up)
MOVES = ((0, 16), (5, 16), (0, 3), (5, -2))


@pytest.mark.parametrize("where", PLACEMENTS)
def test_directed_move(gpu, oracle, directed, where):
    """modgpu_rekey_move_device over ranges that overlap, down and up, at the grid the family's own file forces"""
    d = directed
    room = Room(gpu, N + G + 64)
    ws = gpu.DeviceBuffer(gpu.move_workspace_bytes(N))
    gpu.debug_set_move_grid(4)
    try:
        for pd, shift in MOVES:
            do, so = G + pd, G + pd + shift  # destination and source in the window, which starts G bytes below the 64 KiB boundary
            img = np.full(N + 2 * G + 32, 0xA5, np.uint8)
            img[so:so + N] = d.pt
            for i, case in enumerate(d.cases):
                kf, of, kt, ot = two_keys(d, i, where)
                room.put(img, -G)
                gpu.rekey_move_device(room.base + pd, room.base + pd + shift, N, kf, kt, of, ot, ws)
                room.buf.sync()
                assert gpu.move_status(ws) is None, (where, pd, shift, case)
                info = gpu.last_launch()
                assert info["variant"] == 14 and info["bytes"] == N and info["source_hash"] == gpu.rekey_kernel_source_hash(), info
                want = img.copy()
                want[do:do + N] = d.want2[where][i]
                got = room.get(img.size, -G)
                if not np.array_equal(got, want):
                    raise AssertionError(("move", where, pd, shift, case,
                                          K.report_mismatch(oracle, got[do:do + N], want[do:do + N], case[3], case[2], word0=pd % 16)))
    finally:
        gpu.debug_set_move_grid(0)
        room.free()
        ws.free()


def _transfers(gpu, oracle, d, dev, host_src, host_dst, combos, what):
    """every case up from host_src into dev and down again into host_dst, at (host phase, device phase) combinations; the host buffers
    start on a 16-byte boundary"""
    for ph, pd in combos:
        host_src[:] = 0xA5
        host_src[G + ph:G + ph + N] = d.pt
        keep = host_src.copy()
        dev.put(np.full(N + 2 * G, 0x5A, np.uint8), pd - G)
        want = np.full(N + 2 * G, 0x5A, np.uint8)
        back = np.full(host_dst.size, 0x33, np.uint8)
        back[G + ph:G + ph + N] = d.pt
        host_dst[:] = 0x33
        for i, case in enumerate(d.cases):
            want[G:G + N] = d.want[i]
            gpu.cycle_host_to_device(dev.base + pd, host_src[G + ph:G + ph + N], case[3], case[2])
            info = gpu.last_launch()
            assert info["variant"] == 6 and "modgpu_cycle_xfer_kernel<true" in info["kernel"], info
            check_window(oracle, dev.get(want.size, pd - G), want, case, pd, (what, "upload", ph, pd))
            gpu.cycle_device_to_host(host_dst[G + ph:G + ph + N], dev.base + pd, case[3], case[2])
            info = gpu.last_launch()
            assert info["variant"] == 6 and "modgpu_cycle_xfer_kernel<false" in info["kernel"], info
            if not np.array_equal(host_dst, back):
                got = host_dst[G + ph:G + ph + N] ^ d.want[i]  # the keystream the download applied, against the oracle's
                raise AssertionError((what, "download", ph, pd, case, K.report_mismatch(oracle, got, d.ks[i], case[3], case[2], word0=ph % 16)))
        assert np.array_equal(host_src, keep), "an upload changed its source"


def test_directed_transfers_page_locked(gpu, oracle, directed):
    """modgpu_cycle_host_to_device / _device_to_host on the caller's page-locked pages: co-aligned at both phases (the plain form) and
    the host side at phase 3 (the funnel form)"""
    dev = Room(gpu, N + G + 16)
    pa, pb = gpu.PinnedBuffer(N + 2 * G + 16), gpu.PinnedBuffer(N + 2 * G + 16)
    try:
        assert pa.pinned and pb.pinned and pa.ptr % 16 == 0 and pb.ptr % 16 == 0
        _transfers(gpu, oracle, directed, dev, pa.array, pb.array, ((0, 0), (5, 5), (3, 0), (3, 5)), "page-locked")
    finally:
        pa.free()
        pb.free()
        dev.free()


def test_directed_transfers_pageable(gpu, oracle, directed):
    """the same calls on pageable memory (staged through the library's slots, which take the device's phase)"""
    dev = Room(gpu, N + G + 16)
    raw = [np.empty(N + 2 * G + 32, np.uint8) for _ in range(2)]
    a, b = [r[(-r.ctypes.data) % 16:][:N + 2 * G + 16] for r in raw]
    try:
        _transfers(gpu, oracle, directed, dev, a, b, ((0, 0), (3, 5)), "pageable")
    finally:
        dev.free()


# ---- the table calls: all cases of a family in one table --------------------------------------------------------------------------------
class Arena:
    """One slot of 3 x 64 KiB per case in device memory, each at a 64 KiB-aligned address, behind one blank slot; a page-locked image
    of what the device arena is expected to hold (self.rows: the cases' slots) and a page-locked buffer to download into."""

    def __init__(self, M, entries):
        self.M, self.entries, self.bytes = M, entries, (entries + 1) * SLOT
        self.room = Room(M, self.bytes)
        self.pin, self.scratch = M.PinnedBuffer(self.bytes), M.PinnedBuffer(self.bytes)
        self.img = self.pin.array.reshape(entries + 1, SLOT)
        self.rows = self.img[1:]
        self.addr = np.uint64(self.room.base + SLOT) + np.arange(entries, dtype=np.uint64) * np.uint64(SLOT)

    def at(self, off):
        """the address `off` bytes into every case's slot (a uint64 array)"""
        return self.addr + np.uint64(off)

    def fill(self, value):
        self.img[:] = value
        self.push()

    def push(self):
        self.room.put_from(self.pin.ptr, self.bytes)

    def check(self, oracle, d, lo, what):
        """the whole device arena against the image; a mismatch names the first bad slot and, in it, the byte (an entry's bytes start
        `lo` bytes into its slot)"""
        self.room.get_into(self.scratch.ptr, self.bytes)
        got = self.scratch.array.reshape(self.entries + 1, SLOT)
        if np.array_equal(got, self.img):
            return
        r = int(np.flatnonzero((got != self.img).any(axis=1))[0])
        assert r >= 1, (what, "the blank slot below the first entry was written")
        g, w, case = got[r], self.img[r], d.cases[r - 1]
        assert np.array_equal(g[:lo], w[:lo]) and np.array_equal(g[lo + N:], w[lo + N:]), (what, "entry", r - 1, case, "bytes outside the entry were written")
        raise AssertionError((what, "entry", r - 1, case, K.report_mismatch(oracle, g[lo:lo + N].copy(), w[lo:lo + N].copy(), case[3], case[2], word0=lo % 16)))

    def free(self):
        self.img = self.rows = None
        for b in (self.room, self.pin, self.scratch):
            b.free()


@pytest.fixture(scope="module")
def arena(gpu, directed):
    a = Arena(gpu, len(directed.cases))
    yield a
    a.free()


def _table(gpu, d, dst, src):
    t = gpu.table(len(d.cases))
    t["dst"], t["src"], t["n"], t["stream_off"], t["key"] = dst, src, N, d.offs, d.keys
    return t


def _rekey_table(gpu, d, dst, src, where):
    t = gpu.rekey_table(len(d.cases))
    t["dst"], t["src"], t["n"] = dst, src, N
    quad = [two_keys(d, i, where) for i in range(len(d.cases))]
    t["key_from"] = np.array([gpu.as_int32(q[0]) for q in quad], np.int32)
    t["off_from"] = np.array([q[1] for q in quad], np.uint64)
    t["key_to"] = np.array([gpu.as_int32(q[2]) for q in quad], np.int32)
    t["off_to"] = np.array([q[3] for q in quad], np.uint64)
    return t


def test_directed_cycle_table(gpu, oracle, directed, arena):
    """modgpu_cycle_table_device: one table of all cases per combination of phases, every entry with its own key and offset"""
    d = directed
    src, at = _src_room(gpu, d)
    try:
        arena.fill(0x5A)
        for pd, ps in COMBOS:
            arena.rows[:, pd:pd + N] = d.want
            gpu.cycle_table_device(_table(gpu, d, arena.at(pd), at[ps]))
            assert gpu.last_launch()["variant"] == 8
            arena.check(oracle, d, pd, ("cycle table", pd, ps))
        _src_intact(src, d)
    finally:
        src.free()


@pytest.mark.parametrize("grid", (200, 256, 0))
def test_directed_rekey_table(gpu, oracle, directed, arena, grid):
    """modgpu_rekey_table_device at the grids the family's own file forces, the threshold state in either stream and in both"""
    d = directed
    src, at = _src_room(gpu, d)
    gpu.debug_set_rekey_table_grid(grid)
    try:
        arena.fill(0x5A)
        for pd, ps in COMBOS:
            for where in PLACEMENTS:
                arena.rows[:, pd:pd + N] = d.want2[where]
                gpu.rekey_table_device(_rekey_table(gpu, d, arena.at(pd), at[ps], where))
                assert gpu.last_launch()["variant"] == 9
                arena.check(oracle, d, pd, ("rekey table", grid, where, pd, ps))
        _src_intact(src, d)
    finally:
        gpu.debug_set_rekey_table_grid(0)
        src.free()


def _verify_table_both_ways(d, arena, call, want, pd, what):
    """the comparands `want` at phase pd of every slot: every entry clean; the byte at each entry's threshold position flipped: every
    entry reports exactly that index"""
    arena.rows[:, pd:pd + N] = want
    arena.push()
    r = call()
    assert not r["mismatches"].any() and (r["first_mismatch"] == NONE).all() and (r["n"] == N).all(), (what, np.flatnonzero(r["mismatches"])[:4])
    arena.rows[np.arange(len(d.cases)), pd + d.pos] ^= 0x01
    arena.push()
    r = call()
    assert (r["mismatches"] == 1).all() and np.array_equal(r["first_mismatch"].astype(np.int64), d.pos), (what, np.flatnonzero(r["mismatches"] != 1)[:4])


@pytest.mark.parametrize("grid", (1, 3, 0))
def test_directed_verify_table(gpu, directed, arena, grid):
    """modgpu_verify_table_device against the oracle's bytes in the arena, at the grids the family's own file forces"""
    d = directed
    src, at = _src_room(gpu, d)
    gpu.debug_set_verify_table_grid(grid)
    try:
        arena.img[:] = 0x5A
        for pd, ps in COMBOS:
            t = _table(gpu, d, arena.at(pd), at[ps])
            _verify_table_both_ways(d, arena, lambda: gpu.verify_table_device(t), d.want, pd, ("verify table", grid, pd, ps))
            assert gpu.last_launch()["variant"] == 11
    finally:
        gpu.debug_set_verify_table_grid(0)
        src.free()


@pytest.mark.parametrize("grid", (1, 3, 0))
def test_directed_verify_rekey_table(gpu, directed, arena, grid):
    """modgpu_verify_rekey_table_device, the threshold state in either stream and in both"""
    d = directed
    src, at = _src_room(gpu, d)
    gpu.debug_set_rekey_verify_table_grid(grid)
    try:
        arena.img[:] = 0x5A
        for pd, ps in COMBOS:
            for where in PLACEMENTS:
                t = _rekey_table(gpu, d, arena.at(pd), at[ps], where)
                _verify_table_both_ways(d, arena, lambda: gpu.verify_rekey_table_device(t), d.want2[where], pd, ("verify rekey table", grid, where, pd, ps))
                assert gpu.last_launch()["variant"] == 13
    finally:
        gpu.debug_set_rekey_verify_table_grid(0)
        src.free()


@pytest.mark.parametrize("grid", (1, 2, 3, 0))
def test_directed_digest_table(gpu, directed, grid):
    """modgpu_digest_table_device: one record per case, the source at phases 0, 5 and 3"""
    d = directed
    src, at = _src_room(gpu, d)
    gpu.debug_set_digest_table_grid(grid)
    try:
        for ps in SRC_PHASES:
            rec, adler = gpu.digest_table_device(_table(gpu, d, 0, at[ps]))
            assert gpu.last_launch()["variant"] == 17
            assert np.array_equal(adler, d.adler) and (rec["n"] == N).all(), ("digest table", grid, ps, np.flatnonzero(adler != d.adler)[:4])
    finally:
        gpu.debug_set_digest_table_grid(0)
        src.free()


@pytest.mark.parametrize("grid", (1, 2, 3, 0))
def test_directed_cycle_digest_table(gpu, oracle, directed, arena, grid):
    """modgpu_cycle_digest_table_device: the stored bytes as the cycle table call's, the records of the output side zlib's Adler-32 of
    them, those of the input side the plaintext's"""
    d = directed
    src, at = _src_room(gpu, d)
    gpu.debug_set_cycle_digest_table_grid(grid)
    try:
        for pd, ps in COMBOS:
            for side, adlers in ((gpu.DIGEST_OUTPUT, d.adler), (gpu.DIGEST_INPUT, np.full(len(d.cases), d.pt_adler, np.uint32))):
                arena.fill(0x5A)
                arena.rows[:, pd:pd + N] = d.want
                rec, adler = gpu.cycle_digest_table_device(_table(gpu, d, arena.at(pd), at[ps]), None, side)
                assert gpu.last_launch()["variant"] == 18
                assert np.array_equal(adler, adlers) and (rec["n"] == N).all(), ("cycle digest table", grid, side, pd, ps, np.flatnonzero(adler != adlers)[:4])
                arena.check(oracle, d, pd, ("cycle digest table", grid, side, pd, ps))
        _src_intact(src, d)
    finally:
        gpu.debug_set_cycle_digest_table_grid(0)
        src.free()


@pytest.mark.parametrize("grid", (4, 0))
def test_directed_move_table(gpu, oracle, directed, arena, grid):
    """modgpu_rekey_move_table_device: downward tables (every source 16 or 3 bytes above its destination) and an upward one (2 bytes
    below), every entry overlapping its own source, at the grid the family's own file forces and at the shipped one"""
    d = directed
    gpu.debug_set_move_table_grid(grid)
    try:
        for pd, shift in MOVES:
            for where in PLACEMENTS:
                arena.img[:] = 0xA5
                arena.rows[:, pd + shift:pd + shift + N] = d.pt
                arena.push()
                arena.rows[:, pd:pd + N] = d.want2[where]
                gpu.rekey_move_table_device(_rekey_table(gpu, d, arena.at(pd), arena.at(pd + shift), where))
                assert gpu.last_launch()["variant"] == 15
                arena.check(oracle, d, pd, ("move table", grid, where, pd, shift))
    finally:
        gpu.debug_set_move_table_grid(0)
