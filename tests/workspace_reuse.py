"""What tests/test_gpu_workspace_reuse.py and tests/test_workspace_reuse_cpu.py share: one adapter per kind of call that runs on a
caller's device workspace, the models of what each may change, the comparer, and the case lists.

The ten KINDS are the five table calls, the two fused ones, the two moving ones and the single move call.  A Case is a kind, an entry
count, a side (the fused kinds), optionally one refused entry and a variant (one entry rewritten).  `model(case)` gives everything the
call may change -- from outside the library: the bytes from oracle.cycle_at's keystreams through the move tests' model (want[dst:dst+n]
= img[src:src+n] ^ ks_from ^ ks_to), the records from zlib.adler32, the mismatch counts and first_mismatch from a numpy compare.
`Rig.run(case, ws_off)` lays the case into the move tests' arena (0xA5 guards around the window), gives the call EXACTLY what its own
*_workspace_bytes function returns at an address inside one shared buffer W, and returns (got, want): the model plus the bytes of W
outside the workspace the call was given, which must be what they were.  `compare` names the first output that differs.

The arena, the guards, the key pairs, the keystream base and the model are tests/test_gpu_rekey_move_table.py's."""
import contextlib
import ctypes
import functools
import zlib

import numpy as np

from test_gpu_rekey_move_table import BASE, CAP, CHUNK, G, KEY_PAIRS, PS3, PS4, SPAN, Arena, layout

KINDS = ("cycle_table", "rekey_table", "verify_table", "verify_rekey_table", "digest_table", "cycle_digest_table", "rekey_digest_table",
         "rekey_move_table", "rekey_relayout_table", "rekey_move")
FILLS = ("zero", "leftover", "ones", "random")
NS = (1, 16, 17, 256, 257, 1025, 4097)  # where top, the level sizes and the number of 1024-entry blk records change
BIG_N, SMALL_N, ALIGN_N = 4097, 17, 257
EDGE_SIZES = (0, 1, 15, 17, 4101, 65535, 65537, 131073)
PHASES = (0, 1, 7)
BAD = 123         # the entry a refused case has nonzero flags in
REFUSED_N = 257   # ... and its entry count
GW = 4096         # guard bytes at either end of W
NONE64 = (1 << 64) - 1
OUTPUT, INPUT, PLAIN = 0, 1, 2  # modgpu.DIGEST_OUTPUT / _INPUT / _PLAIN
# single-keystream pairs in the shape of KEY_PAIRS (key_to = 0: the model's second keystream is zero); the last key is the identity
CYCLE_PAIRS = [("ps4", PS4, 0, 3, 3), ("ps3", PS3, 0, 1000, 1000), ("identity", 0x7FFFFFFF, 0, 5, 5)]

# per kind: rekey entries (56 bytes) or table entries (40), its records, its sides, the header family of its workspace, its launches
# (None: they depend on the route), the hook that forces its stream / move grid
SPEC = {
    "cycle_table": dict(rekey=False, rec=None, sides=(None,), family="cycle", launches=3, grid="debug_set_table_grid"),
    "rekey_table": dict(rekey=True, rec=None, sides=(None,), family="cycle", launches=3, grid="debug_set_rekey_table_grid"),
    "verify_table": dict(rekey=False, rec="verify", sides=(None,), family="cycle", launches=3, grid="debug_set_verify_table_grid"),
    "verify_rekey_table": dict(rekey=True, rec="verify", sides=(None,), family="cycle", launches=3, grid="debug_set_rekey_verify_table_grid"),
    "digest_table": dict(rekey=False, rec="digest", sides=(None,), family="cycle", launches=3, grid="debug_set_digest_table_grid"),
    "cycle_digest_table": dict(rekey=False, rec="digest", sides=(OUTPUT, INPUT), family="cycle", launches=3, grid="debug_set_cycle_digest_table_grid"),
    "rekey_digest_table": dict(rekey=True, rec="digest", sides=(PLAIN, OUTPUT, INPUT), family="cycle", launches=3,
                               grid="debug_set_rekey_digest_table_grid"),
    "rekey_move_table": dict(rekey=True, rec=None, sides=(None,), family="move", launches=5, grid="debug_set_move_table_grid"),
    "rekey_relayout_table": dict(rekey=True, rec=None, sides=(None,), family="move", launches=10, grid="debug_set_move_table_grid"),
    "rekey_move": dict(rekey=True, rec=None, sides=(None,), family="single", launches=None, grid="debug_set_move_grid"),
}
assert tuple(SPEC) == KINDS and len(KINDS) == 10
VERIFYING = tuple(k for k in KINDS if SPEC[k]["rec"] == "verify")
DIGESTING = tuple(k for k in KINDS if SPEC[k]["rec"] == "digest")
MOVING = tuple(k for k in KINDS if SPEC[k]["family"] == "move")
REFUSABLE = tuple(k for k in KINDS if SPEC[k]["family"] != "single")  # the single move call has no device tier


def other(kind):
    """the kind whose leavings the leftover fill is: another one, of the other header family for the kinds that have one"""
    return KINDS[(KINDS.index(kind) + 7) % len(KINDS)]


class Case:
    """a kind, n entries, a side (None: the kind's first), `bad` = the entry with nonzero flags (None: a clean call), `variant` = 1
    rewrites one entry (its key pair)"""

    def __init__(self, kind, n, side=None, bad=None, variant=0):
        side = SPEC[kind]["sides"][0] if side is None else side
        assert side in SPEC[kind]["sides"] and (bad is None or (bad < n and kind in REFUSABLE))
        self.kind, self.n, self.side, self.bad, self.variant = kind, n, side, bad, variant
        self.key = (kind, n, side, bad, variant)

    def __repr__(self):
        return "Case" + repr(self.key)


# ---- the layouts, counted from the arena's base (a 64 KiB boundary): [(dst, src, n, pair)] as the move tests have them ---------------
def sizes(n):
    """n entry sizes: the edge set once, largest first (n = 1 is the 131073-byte entry), then small ones, some empty, some of 4101"""
    small = (17, 1, 0, 15, 33, 16, 48)
    return [EDGE_SIZES[7 - i] if i < 8 else 4101 if i % 97 == 5 else small[i % len(small)] for i in range(n)]


def _pairs(kind, n, variant):
    pairs = KEY_PAIRS if SPEC[kind]["rekey"] else CYCLE_PAIRS
    picked = [pairs[i % len(pairs)] for i in range(n)]
    if variant:
        at = min(5, n - 1)
        picked[at] = pairs[(at + 1) % len(pairs)]
    return picked


def _apart(szs, pairs):
    """sources rising from just below a chunk boundary, destinations rising from just below a later one, nothing overlapping; sources
    and destinations at phases 0, 1 and 7 of a 16-byte word, every combination"""
    at, srcs = CHUNK - 40, []
    for i, n in enumerate(szs):
        at = -(-at // 16) * 16 + PHASES[(i // 3) % 3]
        srcs.append(at)
        at += n
    at, segs = -(-(at + 512) // CHUNK) * CHUNK - 33, []
    for i, n in enumerate(szs):
        at = -(-at // 16) * 16 + PHASES[i % 3]
        segs.append((at, srcs[i], n, pairs[i]))
        at += n
    return segs


def _one_way(szs, pairs, down):
    """the move table tests' layout: one side packed, the other spread by gaps that add up, so a destination lies over the sources of
    entries before it; the first entries (gap 0) stay where they are"""
    gaps = (0, 0, 1, 3, 16, 17, 0, 7)
    segs = layout(szs, [gaps[i % len(gaps)] for i in range(len(szs))], down, CHUNK + 7, [None])
    return [(d, s, n, pairs[i]) for i, (d, s, n, _) in enumerate(segs)]


def _both_ways(szs, pairs):
    """entries that slide down, up and stay, sources and destinations rising and disjoint each: a downward entry's destination lies
    over the tail of the source before it, an upward one's over the head of the source behind it (the relayout tests' pattern, with
    shifts that keep 4097 entries inside the arena)"""
    ways = "DUSDDUUDSU"
    segs, src, dst_end = [], 2 * CHUNK + 7, 0
    for i, n in enumerate(szs):
        way = ways[i % len(ways)]
        far = (4099, 65541, 65536)[i % 3] if n > 4096 else (1, 7, 17, 5)[i % 4]
        shift = 0 if way == "S" else far if way == "U" else -far
        src += (0, 1, 3, 16)[i % 4]
        if src + shift < dst_end:
            src = dst_end - shift
        segs.append((src + shift, src, n, pairs[i]))
        dst_end = src + shift + n
        src += n
    return segs


def _single(n, pairs):
    """one entry of n * 255 + 17 bytes whose ranges overlap: the single move call's "table" """
    shift = {1: 1, 16: -17, 17: 4099, 256: -65541, 257: 7, 1025: -65536, 4097: 65541}.get(n, 7)
    src = 2 * CHUNK + 7
    return [(src + shift, src, n * 255 + 17, pairs[n % len(pairs)])]


@functools.lru_cache(maxsize=None)
def _segs(kind, n, variant):
    pairs = _pairs(kind, n, variant)
    if kind == "rekey_move":
        segs = _single(n, KEY_PAIRS)
    elif kind == "rekey_move_table":
        segs = _one_way(sizes(n), pairs, n % 2 == 0)
    elif kind == "rekey_relayout_table":
        segs = _both_ways(sizes(n), pairs)
    else:
        segs = _apart(sizes(n), pairs)
    assert all(d >= G and s >= G and max(d, s) + k <= CAP for d, s, k, _ in segs), (kind, n)
    return segs


def segs_of(case):
    return _segs(case.kind, case.n, case.variant)


def total_bytes(case):
    return sum(n for _, _, n, _ in segs_of(case))


def planted(case):
    """the (entry, byte) pairs whose comparand byte a verifying case has flipped: in every fifth non-empty entry its first byte, its
    middle one and its last"""
    if SPEC[case.kind]["rec"] != "verify":
        return []
    full = [i for i, (_, _, n, _) in enumerate(segs_of(case)) if n]
    return [(i, j) for i in full[::5] for j in sorted({0, segs_of(case)[i][2] // 2, segs_of(case)[i][2] - 1})]


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class Keystreams:
    """the keystream bytes of both keys from BASE on, computed once (read-only); a key that is 0 mod 2^31-1 has zeros"""

    def __init__(self, oracle):
        self.payload = oracle.splitmix_bytes(CAP, 51)
        self.payload.setflags(write=False)
        self.ks = {}
        for key in (PS3, PS4):
            z = np.zeros(SPAN, np.uint8)
            oracle.cycle_at(z, key, BASE)
            z.setflags(write=False)
            self.ks[key] = z
        self.zero = np.zeros(SPAN, np.uint8)
        self.zero.setflags(write=False)
        self.models = {}

    def __call__(self, key):
        return self.ks.get(key, self.zero)


def window(case, K):
    """(lo, img): the arena's bytes [lo - G, hi + G) as the call finds them -- the payload inside 0xA5 guards; a verifying case has what
    the cipher makes of every source at its comparand, with the planted bytes flipped"""
    segs = segs_of(case)
    lo, img = Arena.window(None, segs, K.payload)
    if SPEC[case.kind]["rec"] == "verify":
        img = Arena.model(segs, lo, img, K)
        for i, j in planted(case):
            img[G + segs[i][0] - lo + j] ^= 0x40
    return lo, img


def model(case, K):
    """everything the call may change, as a dict (cached: the arrays are read-only)"""
    if case.key in K.models:
        return K.models[case.key]
    spec, segs = SPEC[case.kind], segs_of(case)
    lo, img = window(case, K)
    refused = case.bad is not None
    want = {}
    ciphered = Arena.model(segs, lo, Arena.window(None, segs, K.payload)[1], K)  # every destination holds its source under the cipher
    writes = spec["rec"] != "verify" and case.kind != "digest_table"
    want["arena"] = ciphered if writes and not refused else img
    if spec["family"] != "single":
        want["table_status"] = case.bad
    if spec["family"] == "move":
        want["move_table_status"] = (case.bad, None)
    if spec["family"] == "single":
        want["move_status"] = None
    if spec["launches"]:
        want["launches"] = spec["launches"]
    if spec["rec"]:
        want["record_guards"] = np.full(2 * G, 0xA5, np.uint8)
    if spec["rec"] and refused:
        want["records_raw"] = np.full(32 * case.n, 0x5A, np.uint8)
    if spec["rec"] == "verify":
        want["summary"] = "refused" if refused else None
    if spec["rec"] == "verify" and not refused:
        rec = np.zeros((case.n, 3), np.uint64)
        for i, (d, _, n, _) in enumerate(segs):
            diff = np.flatnonzero(img[G + d - lo:G + d - lo + n] != ciphered[G + d - lo:G + d - lo + n])
            rec[i] = (diff.size, diff[0] if diff.size else NONE64, n)
        dirty = np.flatnonzero(rec[:, 0])
        want["records"] = rec
        want["summary"] = {"mismatches": int(rec[:, 0].sum()), "first_bad_entry": int(dirty[0]) if dirty.size else None, "entries": case.n}
    if spec["rec"] == "digest" and not refused:
        rec = np.zeros((case.n, 2), np.uint64)
        for i, (d, s, n, (_, kf, _, of, _)) in enumerate(segs):
            read = img[G + s - lo:G + s - lo + n]
            summed = read if case.side == INPUT else read ^ K(kf)[of + s:of + s + n] if case.side == PLAIN else ciphered[G + d - lo:G + d - lo + n]
            rec[i] = (zlib.adler32(summed.tobytes()), n)
        want["records"] = rec
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    K.models[case.key] = want
    return want


# ---- the comparer --------------------------------------------------------------------------------------------------------------------
def compare(got, want, what=""):
    """every output the model has, in turn; AssertionError names the first that differs"""
    missing = set(want) - set(got)
    assert not missing, (what, "the adapter did not return", sorted(missing))
    for name, w in want.items():
        g = got[name]
        if isinstance(w, np.ndarray):
            g = np.asarray(g)
            if g.shape != w.shape or not np.array_equal(g, w):
                bad = np.flatnonzero((g != w).reshape(-1)) if g.shape == w.shape else np.zeros(0, int)
                raise AssertionError((what, name, "differs: shapes, then first / last / count of differing elements", g.shape, w.shape,
                                      int(bad[0]) if bad.size else None, int(bad[-1]) if bad.size else None, int(bad.size)))
        elif g != w:
            raise AssertionError((what, name, "is", g, "expected", w))


# ---- the adapters --------------------------------------------------------------------------------------------------------------------
def need(M, case):
    """what the kind's own *_workspace_bytes function returns for the case"""
    k, n = case.kind, case.n
    if k == "rekey_move":
        return M.move_workspace_bytes(total_bytes(case))
    if k in MOVING:
        return M.rekey_move_table_workspace_bytes(n, total_bytes(case))
    return getattr(M, {"cycle_table": "table", "rekey_table": "rekey_table", "verify_table": "verify_table", "verify_rekey_table": "verify_rekey_table",
                       "digest_table": "digest_table", "cycle_digest_table": "cycle_digest_table", "rekey_digest_table": "rekey_digest_table"}[k]
                   + "_workspace_bytes")(n)


def entries(M, case, base):
    """the table as the device reads it, its addresses counted from `base`"""
    segs = segs_of(case)
    if SPEC[case.kind]["rekey"]:
        t = M.rekey_table(len(segs))
        for i, (dst, src, n, (_, kf, kt, of, ot)) in enumerate(segs):
            t[i]["dst"], t[i]["src"], t[i]["n"] = base + dst, base + src, n
            t[i]["off_from"], t[i]["off_to"] = BASE + of + src, BASE + (of + dst if ot is None else ot + src)
            t[i]["key_from"], t[i]["key_to"] = M.as_int32(kf), M.as_int32(kt)
    else:
        t = M.table(len(segs))
        for i, (dst, src, n, (_, key, _, of, _)) in enumerate(segs):
            t[i]["dst"], t[i]["src"], t[i]["n"], t[i]["stream_off"], t[i]["key"] = base + dst, base + src, n, BASE + of + src, M.as_int32(key)
    if case.bad is not None:
        t[case.bad]["flags"] = 1
    return t


class Site:
    """where a case is laid: the move tests' arena, a table, and the records between 0xA5 guards of their own"""

    def __init__(self, M, max_n):
        self.arena = Arena(M, entries=max_n)
        self.table = self.arena.table
        self.res = M.DeviceBuffer(2 * G + 32 * max_n)

    def free(self):
        self.arena.free()
        self.res.free()


class Rig:
    """One workspace buffer W for everything -- `room` bytes between two guard bands of GW -- and the sites the cases are laid into.  M is
    the package, or a stand-in for it whose DeviceBuffer is the stand-in runtime's device memory."""

    def __init__(self, M, K, room, max_n=BIG_N, sites=1):
        self.M, self.K, self.room = M, K, room
        self.sites = [Site(M, max_n) for _ in range(sites)]
        self.W = M.DeviceBuffer(room + 2 * GW + 64)
        self.inner = GW + (-(self.W.ptr + GW)) % 64  # offset of the 64-byte aligned address the workspaces start at
        self.mirror = np.full(self.W.nbytes, 0xA5, np.uint8)
        self.W.upload(self.mirror)
        self.small = M.DeviceBuffer(4 * G + 32 + 4 * max_n + 8 * ((max_n + 63) // 64) + 8)  # a check's summary, manifest and bitmap, guards between

    def free(self):
        for s in self.sites:
            s.free()
        self.W.free()
        self.small.free()

    def sync(self, stream=None):
        self.W.sync(stream)

    def fill(self, how, seed=0):
        """W's room, every byte: 0x00, 0xFF or seeded random bytes"""
        body = {"zero": lambda: np.zeros(self.room, np.uint8), "ones": lambda: np.full(self.room, 0xFF, np.uint8),
                "random": lambda: np.random.default_rng(seed).integers(0, 256, self.room, dtype=np.uint8)}[how]()
        self.mirror = self.mirror.copy()
        self.mirror[self.inner:self.inner + self.room] = body
        self.W.upload(body, offset=self.inner)

    def lay(self, case, site=0):
        """the window, the table and the records' buffer as the call finds them"""
        S = self.sites[site]
        lo, img = window(case, self.K)
        S.arena.buf.upload(img, offset=S.arena.at + lo - G)
        S.table.upload(entries(self.M, case, S.arena.base).view(np.uint8))
        if SPEC[case.kind]["rec"]:
            pre = np.full(2 * G + 32 * case.n, 0xA5, np.uint8)
            pre[G:G + 32 * case.n] = 0x5A
            S.res.upload(pre)

    def call(self, case, ws_off=0, site=0, stream=None):
        """queues the call: the workspace at W's aligned start + ws_off, exactly need(case) bytes of it"""
        M, S, k, n = self.M, self.sites[site], case.kind, case.n
        ws = self.W.ptr + self.inner + ws_off
        assert ws_off >= 0 and ws_off + need(M, case) <= self.room
        tab, res = S.table.ptr, S.res.ptr + G
        if k == "rekey_move":
            t = entries(M, case, S.arena.base)[0]
            _, kf, kt, _, _ = segs_of(case)[0][3]
            M.rekey_move_device(int(t["dst"]), int(t["src"]), int(t["n"]), kf, kt, int(t["off_from"]), int(t["off_to"]), ws, stream=stream)
        elif k in MOVING:
            getattr(M, k + "_device")(tab, total_bytes(case), ws, n=n, stream=stream)
        elif k in ("cycle_table", "rekey_table"):
            getattr(M, k + "_device")(tab, ws, n=n, stream=stream)
        elif k in ("cycle_digest_table", "rekey_digest_table"):
            getattr(M, k + "_device")(tab, res, case.side, ws, n=n, stream=stream)
        else:
            getattr(M, k + "_device")(tab, res, ws, n=n, stream=stream)

    def gather(self, case, ws_off=0, site=0, status=True):
        """what the call left, once its stream has been waited for; status=False leaves out what is read from the workspace (another
        call has run on it since)"""
        M, S, spec, n = self.M, self.sites[site], SPEC[case.kind], case.n
        ws = self.W.ptr + self.inner + ws_off
        lo, img = window(case, self.K)
        got = {"arena": S.arena.buf.download(img.size, offset=S.arena.at + lo - G)}
        if spec["rec"]:
            raw = S.res.download(2 * G + 32 * n)
            got["record_guards"] = np.concatenate([raw[:G], raw[G + 32 * n:]])
            got["records_raw"] = raw[G:G + 32 * n]
            if spec["rec"] == "verify":
                r = M.verify_results(S.res.ptr + G, n)
                got["records"] = np.stack([r["mismatches"], r["first_mismatch"], r["n"]], axis=1).astype(np.uint64)
            else:
                r, adler = M.digest_results(S.res.ptr + G, n)
                got["records"] = np.stack([adler.astype(np.uint64), r["n"]], axis=1).astype(np.uint64)
        if not status:
            return got
        if spec["family"] != "single":
            got["table_status"] = M.table_status(ws)
        if spec["family"] == "move":
            got["move_table_status"] = M.rekey_move_table_status(ws)
        if spec["family"] == "single":
            got["move_status"] = M.move_status(ws)
        if spec["rec"] == "verify":
            try:
                got["summary"] = M.verify_table_summary(ws)
            except M.ModGpuError:
                got["summary"] = "refused"
        return got

    def run(self, case, ws_off=0, site=0):
        """lay, call, wait, gather: (got, want), both with the bytes of W outside the workspace the call was given"""
        self.lay(case, site)
        before = self.M.path_stats()["gpu_launches"]
        self.call(case, ws_off, site)
        self.sync()
        got = self.gather(case, ws_off, site)
        got["launches"] = self.M.path_stats()["gpu_launches"] - before
        a, b = self.inner + ws_off, self.inner + ws_off + need(self.M, case)
        after = self.W.download()
        got["w_outside"] = np.concatenate([after[:a], after[b:]])
        want = dict(model(case, self.K), w_outside=np.concatenate([self.mirror[:a], self.mirror[b:]]))
        self.mirror = after
        return got, want

    def check(self, case, manifest, ws_off=0, site=0):
        """modgpu_digest_check_device on the records the case's call left, `manifest` the expected Adler-32 values, the producer's
        workspace given: the summary as a dict, the bitmap's words, and the guards around the three small buffers"""
        M, S, n = self.M, self.sites[site], case.n
        words = (n + 63) // 64
        pre = np.full(self.small.nbytes, 0xA5, np.uint8)
        at_sum, at_exp = G, 2 * G + 32
        at_bits = at_exp + 4 * n + (-(4 * n)) % 8 + G
        pre[at_exp:at_exp + 4 * n] = np.asarray(manifest, dtype="<u4").view(np.uint8)
        self.small.upload(pre)
        M.digest_check_device(S.res.ptr + G, self.small.ptr + at_exp, n, table_workspace=self.W.ptr + self.inner + ws_off,
                              summary=self.small.ptr + at_sum, bad_bits=self.small.ptr + at_bits)
        self.sync()
        after = self.small.download()
        s = after[at_sum:at_sum + 32].view("<u8")
        bits = after[at_bits:at_bits + 8 * words]
        rest = np.ones(after.size, bool)
        for a, k in ((at_sum, 32), (at_exp, 4 * n), (at_bits, 8 * words)):
            rest[a:a + k] = False
        return {"bad_entries": int(s[0]), "first_bad_entry": None if int(s[1]) == NONE64 else int(s[1]), "entries": int(s[2]), "refused": int(s[3]),
                "bits": bits.copy(), "guards_intact": bool((after[rest] == 0xA5).all()),
                "bits_untouched": bool((bits == 0xA5).all())}


@contextlib.contextmanager
def rig(M, K, cases, sites=1):
    """a Rig sized for `cases` in the testing flavour, every stream and move grid forced to 4 so that each workgroup draws many tickets
    and waits across entries"""
    with M.testing_flavour():
        hooks = sorted({SPEC[k]["grid"] for k in KINDS})
        for h in hooks:
            getattr(M, h)(4)
        r = Rig(M, K, max(need(M, c) for c in cases) + 64, max(c.n for c in cases), sites)
        try:
            yield r
        finally:
            for h in hooks:
                getattr(M, h)(0)
            r.free()


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def sided(kind, n, **kw):
    """the case of `kind` at n entries on each of its sides"""
    return [Case(kind, n, side, **kw) for side in SPEC[kind]["sides"]]


FILL_CASES = [(fill, kind) for fill in FILLS for kind in KINDS]
PAIR_CASES = [(prev, nxt, a, b) for prev in KINDS for nxt in KINDS for a, b in ((BIG_N, SMALL_N), (SMALL_N, BIG_N))]
ALIGN_CASES = list(KINDS)
REFUSAL_PREVIOUS = ("cycle_digest_table", "rekey_relayout_table")  # one per header family: CycleTableHdr, MoveTableHdr
assert len(FILL_CASES) == 40 and len(PAIR_CASES) == 200 and len({(p, q) for p, q, _, _ in PAIR_CASES}) == 100 and len(ALIGN_CASES) == 10


def all_cases():
    """every Case the lists above can run: what a Rig must have room for"""
    out = []
    for kind in KINDS:
        for n in NS + (ALIGN_N,):
            out += sided(kind, n)
        if kind in REFUSABLE:
            out += sided(kind, REFUSED_N, bad=BAD)
        out += sided(kind, REFUSED_N)
    return out


PASSED = set()  # (fill, kind) of every fill case that passed in this session


def fill_blocked(fill, kind):
    """why the 0xFF or random fill must not run for the kind (a plan record read from such bytes is a wild pointer), or None"""
    missing = [f for f in ("zero", "leftover") if (f, kind) not in PASSED] if fill in ("ones", "random") else []
    return f"{kind} is not run on a workspace of {fill} bytes: it did not pass the {' and the '.join(missing)} fill in this session" if missing else None


def run_fill(r, fill, kind, ns=NS):
    """case a: the kind at every n of `ns`, on every side, W filled beforehand"""
    assert not fill_blocked(fill, kind), fill_blocked(fill, kind)
    for n in ns:
        for case in sided(kind, n):
            if fill == "leftover":
                r.fill("zero")
                got, want = r.run(Case(other(kind), BIG_N))
                assert got.get("table_status") is None and got.get("move_status") is None, (other(kind), "left behind a refused call")
            else:
                r.fill(fill, seed=n)
            compare(*r.run(case), (fill, case))
    PASSED.add((fill, kind))


def run_pairs(r, prev, nexts=KINDS, orders=((BIG_N, SMALL_N), (SMALL_N, BIG_N))):
    """case b: `prev` then every next kind, both size orders, W untouched in between; next's outputs are compared"""
    for nxt in nexts:
        for a, b in orders:
            for case in sided(nxt, b):
                r.run(Case(prev, a))
                compare(*r.run(case), ("after", prev, a, case))


def run_refusals(r, prev, nexts=KINDS):
    """case c: a refused `prev` then a clean next of another kind; a clean `prev` then a refused next"""
    for nxt in nexts:
        if nxt == prev:
            continue
        for case in sided(nxt, REFUSED_N):
            got, _ = r.run(Case(prev, REFUSED_N, bad=BAD))
            assert got["table_status"] == BAD, (prev, "was not refused", got["table_status"])
            compare(*r.run(case), ("after a refused", prev, case))
        if nxt in REFUSABLE:
            for case in sided(nxt, REFUSED_N, bad=BAD):
                got, _ = r.run(Case(prev, REFUSED_N))
                assert got["table_status"] is None, (prev, got["table_status"])
                compare(*r.run(case), ("refused after a clean", prev, case))


def run_verify_summaries(r):
    """case d: the summary of a verifying call at 17 entries behind one at 4097 with planted mismatches is the small call's"""
    for big in VERIFYING:
        for small in VERIFYING:
            got, want = r.run(Case(big, BIG_N))
            assert want["summary"]["mismatches"] > 100 and got["summary"] == want["summary"], (big, got["summary"], want["summary"])
            got, want = r.run(Case(small, SMALL_N))
            assert want["summary"]["entries"] == SMALL_N and 0 < want["summary"]["mismatches"] < 100
            compare(got, want, (small, "after", big))


def run_move_statuses(r):
    """case d: rekey_move_table_status after a clean moving call on each fill is (None, None)"""
    for kind in MOVING:
        for fill in FILLS:
            if fill == "leftover":
                r.fill("zero")
                r.run(Case(other(kind), BIG_N))
            else:
                r.fill(fill, seed=3)
            got, want = r.run(Case(kind, ALIGN_N))
            assert got["move_table_status"] == (None, None), (kind, fill, got["move_table_status"])
            compare(got, want, (kind, fill))


def run_checks(r):
    """case d: modgpu_digest_check_device reads the producing call's header in W -- behind a refused call of another kind the check of
    a clean producer compares (refused clear, the bad count right); behind a refused producer it says so and compares nothing"""
    for kind in DIGESTING:
        refused_other = Case(other(kind) if other(kind) in REFUSABLE else "rekey_relayout_table", REFUSED_N, bad=BAD)
        for case in sided(kind, REFUSED_N):
            got, _ = r.run(refused_other)
            assert got["table_status"] == BAD
            got, want = r.run(case)
            compare(got, want, case)
            manifest = want["records"][:, 0].astype(np.uint32)
            wrong = [3, 64, 65, REFUSED_N - 1]
            manifest[wrong] ^= 1
            c = r.check(case, manifest)
            assert (c["refused"], c["bad_entries"], c["first_bad_entry"], c["entries"], c["guards_intact"]) == (0, len(wrong), 3, REFUSED_N, True), (case, c)
            assert np.flatnonzero(np.unpackbits(c["bits"], bitorder="little")[:REFUSED_N]).tolist() == wrong, case
        for case in sided(kind, REFUSED_N, bad=BAD):
            got, want = r.run(case)
            compare(got, want, case)
            c = r.check(case, np.zeros(REFUSED_N, np.uint32))
            assert (c["refused"], c["bad_entries"], c["first_bad_entry"], c["entries"], c["guards_intact"], c["bits_untouched"]) == \
                (1, 0, None, REFUSED_N, True, True), (case, c)


def run_aligned(r, kind):
    """case e: the workspace at an address that is 8 modulo 64, on the leftover fill"""
    for case in sided(kind, ALIGN_N):
        r.fill("zero")
        r.run(Case(other(kind), BIG_N))
        assert (r.W.ptr + r.inner + 8) % 64 == 8
        compare(*r.run(case, ws_off=8), ("8 modulo 64", case))


# ---- the package on the CPU stand-in of the HIP runtime ----------------------------------------------------------------------------
class StandinBuffer:
    """DeviceBuffer's surface over what the stand-in runtime knows as device memory"""

    def __init__(self, M, nbytes):
        self.M, self.L, self.nbytes = M, M.lib(), nbytes  # (each flavour is a CDLL of its own: the prototypes are set on the one in use)
        self.L.modgpu_shim_xfer_alloc.restype = ctypes.c_void_p
        self.L.modgpu_shim_xfer_alloc.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
        self.L.modgpu_shim_xfer_free.argtypes = [ctypes.c_void_p]
        self.ptr = self.L.modgpu_shim_xfer_alloc(max(nbytes, 1), 0)
        assert self.ptr

    def upload(self, host, offset=0):
        host = np.ascontiguousarray(host, dtype=np.uint8)
        assert offset + host.size <= self.nbytes
        ctypes.memmove(self.ptr + offset, host.ctypes.data, host.size)

    def download(self, n=None, offset=0):
        n = self.nbytes - offset if n is None else n
        out = np.empty(n, np.uint8)
        ctypes.memmove(out.ctypes.data, self.ptr + offset, n)
        return out

    def sync(self, stream=None):
        rc = self.L.modgpu_sync(-1, ctypes.c_void_p(stream or 0))
        assert rc == 0, rc

    def free(self):
        if self.ptr:
            self.L.modgpu_shim_xfer_free(ctypes.c_void_p(self.ptr))
            self.ptr = None


class Standin:
    """modulate_amd with DeviceBuffer replaced: for a process whose MODGPU_LIB is the stand-in build of the library"""

    def __init__(self, M):
        self._M = M
        assert M.testing_hooks() and hasattr(M.lib(), "modgpu_shim_xfer_alloc"), "MODGPU_LIB must name the stand-in build"

    def __getattr__(self, name):
        return getattr(self._M, name)

    def DeviceBuffer(self, nbytes):
        return StandinBuffer(self._M, nbytes)
