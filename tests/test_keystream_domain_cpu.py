"""The keystream arithmetic's state domain, the part that needs no GPU: the helpers of tests/keystream_domain.py against the C
oracle, the closed-form facts that make 1 and m - 1 THE threshold states of the kernels' fold, the library's host loop on the
directed threshold cases and over one full period, and the evidence that an off-by-one threshold is all but invisible to the key and
offset lists of the older GPU files and visible to the directed cases of tests/test_gpu_keystream_domain.py."""
import os

import numpy as np
import pytest

import keystream_domain as K

M, A, P = K.M, K.A, K.P
ISAS = ("generic", "avx2", "avx512")
# (as tests/test_host_cpu.py and tests/test_capi_cpu.py have it: on a machine with a GPU conftest.py forbids the host loop)
needs_host_loop = pytest.mark.skipif(os.environ.get("MODGPU_REQUIRE_GPU", "0") not in ("", "0"),
                                     reason="MODGPU_REQUIRE_GPU forbids the host loop in this process")
HOST_N = 3 * 64 + 5  # three blocks of the widest body and a ragged end: every position of a block and of both its neighbours
HOST_LEADS = (0, 5)  # bytes past a 64-byte boundary at which the buffer starts


def _offered(modgpu, isa):
    """whether this machine's CPU runs the named body of the host loop (the widest one is never missing a narrower one)"""
    try:
        modgpu.cycle_scalar_host_isa(np.zeros(1, np.uint8), 1, isa)
    except modgpu.ModGpuError as e:
        assert e.code == 1 and isa != "generic"  # this CPU does not run that body
        return False
    return True


@pytest.fixture(scope="module")
def period_ks(oracle):
    """ks[0 : P + 64] of key 1 from the oracle: built once, never written to"""
    ks = K.full_period_keystream(oracle, 1, 64)
    ks.setflags(write=False)
    return ks


def test_constants_are_the_oracles(oracle):
    assert (K.M, K.A, K.P) == (oracle.LCG_M, oracle.LCG_A, oracle.PERIOD)
    assert pow(A, P, M) == 1 and all(pow(A, P // q, M) != 1 for q in (2, 3, 7, 11, 31, 151, 331))  # a is a primitive root: period P
    assert 2 * 3 * 3 * 7 * 11 * 31 * 151 * 331 == P


def test_full_period_keystream_equals_one_serial_pass(oracle):
    """the threaded slices against one serial oracle.cycle_at, at a reduced length that is no multiple of a slice, at two keys"""
    n = (5 << 20) + 77
    for key in (1, 0x90CFC0AB):
        got = K.full_period_keystream(oracle, key, 64, length=n)
        assert got.size == n + 64 and got.dtype == np.uint8
        assert np.array_equal(got, oracle.cycle_at(np.zeros(n + 64, np.uint8), key, 0)), hex(key)


def test_period_array_wraps(period_ks):
    """the 64 bytes behind P repeat the first 64: the array really spans the whole period"""
    assert period_ks.size == P + 64 and np.array_equal(period_ks[P:], period_ks[:64]) and period_ks[0] == (~A) & 0xFF


def test_key_for_against_the_oracle(oracle):
    idx = [0, 1, 15, 16, 65535, P - 2, P - 1, P, P + 1, 2 * P - 1, (1 << 32) + 5, (1 << 63) + 11, (1 << 64) - 1]
    for state in K.THRESHOLD_STATES + (12345, 0x40000000):
        for i in idx:
            for neg in (False, True):
                key = K.key_for(state, i, neg)
                assert -(1 << 31) <= key < (1 << 31) and (key < 0) == neg and key % M != 0
                assert oracle.state_at(key, i) == state, (state, i, neg)
    assert K.key_for(1, P - 1) == 1 and K.key_for(1, 3 * P - 1) == 1 and K.key_for(1, P - 1, True) == 1 - M  # the exponent wraps to 0
    for state, pos, off, key in K.directed_cases():
        assert oracle.state_at(key, off + pos) == state
    assert any(c[3] < 0 for c in K.directed_cases()) and any(c[3] > 0 for c in K.directed_cases())


def test_why_these_are_the_threshold_states():
    """mul_fold's X = hi + lo31 (modulate_amd/csrc/cycle_kernel_impl.h) of the word state that puts a given state at byte J, for every
    J = 1..15: state 1 always appears as X = 2^31, the lowest value that must carry, m - 1 as 2^31 - 2, the highest that must not (X
    = m itself cannot occur: m is prime), 2 as 2^31 + 1 and m - 2 as 2^31 - 3.  Fails if the byte table or the modulus changes."""
    assert K.BYTE_POW[:3] == [1, 16807, 282475249] and len(K.BYTE_POW) == 16
    for j in range(1, 16):
        word_state = lambda state: state * pow(A, -j, M) % M
        assert K.fold(word_state(1), j) == 0x80000000
        assert K.fold(word_state(M - 1), j) == 0x7FFFFFFE
        assert K.fold(word_state(2), j) == 0x80000001
        assert K.fold(word_state(M - 2), j) == 0x7FFFFFFD
        for state in K.THRESHOLD_STATES:  # canonicalising rule and the two forms the kernels take it in
            x = K.fold(word_state(state), j)
            assert x + (x >> 31) & 0xFF == state & 0xFF and (x + (1 << 31) >> 32) == x >> 31 == (1 if state <= 2 else 0)


def test_reporter_names_the_byte(oracle):
    key = K.key_for(M - 1, 1000 + 37)
    want = oracle.keystream(key, 100, 1000)
    got = want.copy()
    assert K.report_mismatch(oracle, got, want, key, 1000) is None
    got[37] ^= 1
    got[90] ^= 1
    line = K.report_mismatch(oracle, got, want, key, 1000, word0=3)
    assert line.startswith("first bad byte 37 of 100: stream index 1037, state 0x7ffffffe, word position 8, ") and f"want {int(want[37]):#04x}" in line
    big = np.zeros((5 << 20) + 3, np.uint8)
    assert K.first_mismatch(big, big.copy()) is None and K.all_zero(big)
    other = big.copy()
    other[(4 << 20) + 9] = other[-1] = 1
    assert K.first_mismatch(other, big) == (4 << 20) + 9 and not K.all_zero(other)


@needs_host_loop
@pytest.mark.parametrize("isa", ISAS)
def test_host_loop_directed_threshold_states(modgpu, oracle, isa):
    """each body of the host loop the machine offers: the four threshold states at every position of a 64-byte block, of the block in
    front of it and of the one behind it with its ragged end, at the four offsets and two alignments, keys of either sign"""
    pt = oracle.splitmix_bytes(HOST_N + 64, 0x686F7374)
    cases = K.directed_cases(positions=range(HOST_N), offs=K.DIRECTED_OFFS[:3] + ((1 << 64) - HOST_N - 1,))
    if not _offered(modgpu, isa):
        return
    for lead in HOST_LEADS:
        for state, pos, off, key in cases:
            got, want = pt.copy(), pt.copy()
            modgpu.cycle_scalar_host_isa(got[lead:lead + HOST_N], key, isa, off)
            oracle.cycle_at(want[lead:lead + HOST_N], key, off)
            assert np.array_equal(got, want), (isa, lead, K.report_mismatch(oracle, got[lead:lead + HOST_N], want[lead:lead + HOST_N], key, off))
            assert got[lead + pos] == pt[lead + pos] ^ (~state & 0xFF)  # (the case is what it says it is)


@needs_host_loop
@pytest.mark.parametrize("isa", ISAS)
def test_host_loop_full_period(modgpu, oracle, period_ks, isa):
    """One pass of a body over n = P + 64 bytes that start as the oracle's keystream of key 1: all zero afterwards.  NOT exhaustive for
    the host loop: a body holds W = 16, 32 or 64 lanes and steps each by a^W; a pass of P bytes is P / W blocks, so a lane sees a share
    of 1 / W of the states (which ones depends on how the call is cut into spans: each span starts its lanes afresh) -- every state is
    met by exactly one lane, not by each.  Since W and P are even, a^W has order P / 2 and no number of passes from one starting
    point shows a lane more than half of the states.  The directed test above puts the threshold states into every lane instead."""
    if not _offered(modgpu, isa):
        return
    buf = period_ks.copy()
    modgpu.cycle_scalar_host_isa(buf, 1, isa)
    if not K.all_zero(buf):
        raise AssertionError((isa, K.report_mismatch(oracle, buf, np.zeros_like(buf), 1, 0)))


# ---- sensitivity: a deliberately wrong model of the fold, carry when X > 2^31 instead of X >= 2^31 --------------------------------------
WRONG = (1 << 31) + 1


@pytest.mark.parametrize("state", K.THRESHOLD_STATES)
def test_directed_cases_see_the_off_by_one_threshold(oracle, state):
    """The directed cases of tests/test_gpu_keystream_domain.py (positions, offsets, both phases) against a Python model of the
    kernels' keystream.  The faithful model equals the oracle everywhere; the wrong one differs in exactly one byte -- the byte the
    case placed, which the reporter names -- whenever that byte holds state 1 and is one a word computes with the fold, and nowhere
    in any other case: one wrong byte per 2 GiB of stream and word position, which only a test that puts state 1 there can see."""
    seen = 0
    for _, pos, off, key in K.directed_cases(states=(state,)):
        want = oracle.keystream(key, K.DIRECTED_N, off)
        for phase in K.DIRECTED_PHASES:
            word0 = phase % K.WORD
            assert np.array_equal(K.model_keystream(key, off, K.DIRECTED_N, word0), want), (state, pos, off, phase)
            wrong = K.model_keystream(key, off, K.DIRECTED_N, word0, carry_from=WRONG)
            bad = np.flatnonzero(wrong != want)
            if state == 1 and K.is_folded(pos, word0):
                assert bad.tolist() == [pos], (pos, off, phase, bad[:4])
                line = K.report_mismatch(oracle, wrong, want, key, off, word0)
                assert line.startswith(f"first bad byte {pos} of {K.DIRECTED_N}: stream index {off + pos}, state 0x00000001, "
                                       f"word position {(word0 + pos) % 16}, got 0xff, want 0xfe"), line
                seen += 1
            else:
                assert bad.size == 0, (state, pos, off, phase, bad[:4])
    positions = sum(K.is_folded(pos, ph % K.WORD) for pos in K.DIRECTED_POSITIONS for ph in K.DIRECTED_PHASES)
    assert seen == (len(K.DIRECTED_OFFS) * positions if state == 1 else 0) and positions > 80


def test_what_the_older_key_and_offset_lists_see_of_it(oracle):
    """The same wrong model over the keys, offsets, sizes and alignments that tests/test_gpu_parity.py and tests/test_gpu_digest.py
    compare.  On every list of test_gpu_parity.py it equals the oracle: the in-place kernels' threshold was never looked at.  On
    test_gpu_digest.py's lists (they are test_gpu_verify.py's and test_gpu_rekey.py's too) it differs in ONE place, by an accident of
    the numbers: key 1 has state 1 at every index = -1 (mod P), 2P = 2^32 - 4, and the offset 2^32 - 17 of that list, chosen for the
    32-bit edge, puts index 2P - 1 at byte 12.  So those families did meet state 1, at the few word positions (12 + phase) mod 16
    that the file's phases make of byte 12, and nowhere else; m - 1 they never met where it matters no more than any other state.
    Every differing byte is checked to be state 1 at a folded position, so the list below is exactly what the old lists could see."""
    import test_gpu_digest as D
    import test_gpu_parity as G
    hits = []

    def run(tag, key, off, n, word0s):
        want = oracle.keystream(key, n, off)
        for word0 in word0s:
            for j in np.flatnonzero(K.model_keystream(oracle.as_int32(key), off, n, word0, carry_from=WRONG) != want).tolist():
                assert oracle.state_at(key, off + j) == 1 and K.is_folded(j, word0), (tag, hex(key), off, word0, j)
                hits.append((tag, key, off, word0, j))

    for key in G.KEYS:  # test_device_sizes_and_alignments: every size is a prefix of the largest, at every base misalignment
        run("parity", key, 0, max(G.SIZES), range(16))
    offs = [1, 15, 16, 4095, 4096, 4097, (1 << 24) + 5, P - 100, P - 1, P, P + 1, (1 << 32) - 17, (1 << 32) - 1, 1 << 32,
            (1 << 40) + 123, (1 << 63) + 99, (1 << 64) - 70000]  # test_stream_offsets
    for key in (0x90CFC0AB, 0xC64EED30, 12345):
        for off in offs:
            run("parity", key, off, 66000, (0,))
    word0s = sorted({ph % 16 for ph in D.PHASES})
    for key in D.KEYS:
        for off in [0] + D.OFFSETS:
            run("digest", key, off, max(D.EDGE_SIZES), word0s)
    assert [h for h in hits if h[0] == "parity"] == []
    assert hits == [("digest", 1, (1 << 32) - 17, w, 12) for w in word0s if K.is_folded(12, w)] and (1 << 32) - 17 + 12 == 2 * P - 1, hits
    assert 1 <= len(hits) < 15  # a few of a word's fifteen folded positions, in the families that use this list
