"""Shared by tests/test_gpu_keystream_domain.py and tests/test_keystream_domain_cpu.py (a plain module, no fixtures).

The keystream block's state domain: the generator s_i = a^(i+1) * k mod m has period P = m - 1 = 2^31 - 2 and visits every
non-zero residue once per period; a kernel computes byte J of a 16-byte word from the word's first state by one multiply
and a Mersenne fold whose result X = hi + lo31 is canonicalised by "+1 if X >= 2^31".  The states at that threshold --
1 (X = 2^31, the lowest value that must carry) and m - 1 (X = 2^31 - 2, the highest that must not) -- occur once in 2 GiB
of stream, so tests have to put them where they look: `key_for` makes the key, `full_period_keystream` the whole period.

Nothing here calls the library under test: the C oracle (oracle/cycle_oracle.c), Python integers and numpy only.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

M = 0x7FFFFFFF
A = 16807
P = M - 1
WORD = 16
THRESHOLD_STATES = (1, 2, M - 2, M - 1)
BYTE_POW = [pow(A, j, M) for j in range(WORD)]  # a^J: lcg::kBytePow of modulate_amd/csrc/lcg.h, recomputed


CHUNK = 65536
DIRECTED_N = 2 * CHUNK + 16 + 5  # two whole chunks, one more word, a ragged tail
# head bytes and first word; the chunk edge; last word and ragged tail
DIRECTED_POSITIONS = tuple(range(16)) + tuple(range(CHUNK - 8, CHUNK + 9)) + tuple(range(DIRECTED_N - 16, DIRECTED_N))
DIRECTED_OFFS = (0, P - 3, (1 << 32) + 5, (1 << 64) - DIRECTED_N - 1)
DIRECTED_PHASES = (0, 5)  # bytes past a 64 KiB boundary at which a destination starts


def directed_cases(positions=DIRECTED_POSITIONS, offs=DIRECTED_OFFS, states=THRESHOLD_STATES):
    """(state, position, off, key): `key` puts `state` at byte `position` of a buffer whose byte 0 has stream index `off`.
    Every fourth key is returned in its negative-int32 form."""
    out = []
    for state in states:
        for off in offs:
            for pos in positions:
                out.append((state, pos, off, key_for(state, off + pos, negative=len(out) % 4 == 3)))
    return out


def is_folded(pos, word0):
    """True if byte `pos` of a buffer whose byte 0 sits at word position word0 is one of bytes 1..15 of a 16-byte word as
    model_keystream lays them out: the bytes computed with the fold (a word's byte 0 and the head bytes in front of the first word
    are states kept canonical by the jump arithmetic)"""
    head = (WORD - word0) % WORD
    return pos >= head and (pos - head) % WORD != 0


def pool_size():
    return max(1, min(16, os.cpu_count() or 1))


def _slices(n, parts):
    """`parts` contiguous (lo, hi) slices of range(n), cut at multiples of 64 bytes"""
    step = max(64, -(-n // parts) + 63 & ~63)
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def full_period_keystream(oracle, key, extra, length=None):
    """ks[0 : P + extra] of `key` as one uint8 array (`length` replaces P for a reduced run): oracle.cycle_at over zero bytes, in
    contiguous slices on a thread pool (ctypes releases the GIL; each slice jumps to its own stream offset)."""
    n = (P if length is None else length) + extra
    try:
        ks = np.zeros(n, dtype=np.uint8)
    except MemoryError as e:
        raise AssertionError(f"the host lacks the memory for {n} bytes of keystream") from e
    with ThreadPoolExecutor(pool_size()) as pool:
        list(pool.map(lambda s: oracle.cycle_at(ks[s[0]:s[1]], key, s[0]), _slices(n, 4 * pool_size())))
    return ks


def key_for(state, index, negative=False):
    """An int32 key whose stream has canonical state `state` at stream index `index`: the residue state * a^-(index+1) mod m --
    the exponent is (index mod P) + 1, so an index = -1 (mod P) makes it P and the power 1 -- or, with `negative`, that residue
    minus m: a negative int32 of the same residue.  Callers assert oracle.state_at(key, index) == state."""
    assert 0 < state < M
    res = state * pow(A, -((index % P) + 1), M) % M
    return res - M if negative else res


def first_mismatch(got, want):
    """index of the first byte at which two equally long uint8 arrays differ, or None; slices compared on the thread pool"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    n = got.size
    if n < (1 << 22):
        bad = np.flatnonzero(got != want)
        return int(bad[0]) if bad.size else None

    def one(s):
        lo, hi = s
        if np.array_equal(got[lo:hi], want[lo:hi]):
            return None
        for at in range(lo, hi, 1 << 20):  # (keeps the boolean temporaries small)
            bad = np.flatnonzero(got[at:min(at + (1 << 20), hi)] != want[at:min(at + (1 << 20), hi)])
            if bad.size:
                return at + int(bad[0])

    with ThreadPoolExecutor(pool_size()) as pool:
        hits = [h for h in pool.map(one, _slices(n, 4 * pool_size())) if h is not None]
    return min(hits) if hits else None


def all_zero(a):
    """True if a uint8 array holds only zero bytes; slices on the thread pool"""
    if a.size < (1 << 22):
        return not a.any()
    with ThreadPoolExecutor(pool_size()) as pool:
        return not any(pool.map(lambda s: bool(a[s[0]:s[1]].any()), _slices(a.size, 4 * pool_size())))


def report_mismatch(oracle, got, want, key, index0, word0=None):
    """None if got == want, else a line that names the first bad byte: its index, its stream index index0 + j, the oracle's state
    there, its position in the 16-byte word (word0 is the word position of byte 0; default: index0 mod 16) and both bytes."""
    j = first_mismatch(got, want)
    if j is None:
        return None
    word0 = index0 % WORD if word0 is None else word0
    return (f"first bad byte {j} of {got.size}: stream index {index0 + j}, state {oracle.state_at(key, index0 + j):#010x}, "
            f"word position {(word0 + j) % WORD}, got {int(got[j]):#04x}, want {int(want[j]):#04x}")


def fold(s, j):
    """X = hi + lo31 of the product s * a^j: the non-canonical state of byte j of the word whose first state is s (mul_fold of
    modulate_amd/csrc/cycle_kernel_impl.h: s*y == hi * 2^31 + lo31 == hi + lo31 (mod m))"""
    p = s * BYTE_POW[j]
    return (p >> 31) + (p & M)


def model_keystream(key, index0, n, word0, carry_from=1 << 31):
    """A Python model of the kernels' keystream over n bytes from stream index index0, byte 0 at word position word0: the first byte
    of every 16-byte word (and every byte in front of the first whole word) is the canonical state itself, bytes 1..15 of a word come
    from the fold of the word's first state, +1 if X >= carry_from.  carry_from = 2^31 is what the kernels do; 2^31 + 1 is the
    deliberately wrong "carry when X > 2^31".  The keystream byte is ~state.  uint8 array."""
    res = key % M
    assert res != 0
    head = min(n, (WORD - word0) % WORD)
    out = np.empty(n, dtype=np.uint8)
    s = res * pow(A, (index0 % P) + 1, M) % M
    for j in range(head):
        out[j] = s & 0xFF
        s = s * A % M
    words = -(-(n - head) // WORD)
    if words:
        # states of the words' first bytes by doubling: w[k] = s * a^(16 k)
        w = np.array([s], dtype=np.uint64)
        while w.size < words:
            w = np.concatenate([w, w * np.uint64(pow(A, WORD * w.size, M)) % np.uint64(M)])
        w = w[:words]
        cols = np.empty((words, WORD), dtype=np.uint8)
        cols[:, 0] = (w & np.uint64(0xFF)).astype(np.uint8)
        for j in range(1, WORD):
            p = w * np.uint64(BYTE_POW[j])  # < 2^62
            x = (p >> np.uint64(31)) + (p & np.uint64(M))
            cols[:, j] = ((x + (x >= np.uint64(carry_from))) & np.uint64(0xFF)).astype(np.uint8)
        out[head:] = cols.reshape(-1)[:n - head]
    return ~out
