"""Characterisation of the Python wrappers of modulate_amd/capi.py, with neither library nor GPU: a recording stand-in takes the
place of capi.lib, and for every case the sequence of C calls (names and normalised arguments), the return value and the exception
are compared with tests/capi_wrapper_calls.json.  That file is recorded, not written by hand:

    python tests/test_capi_wrappers_cpu.py --record

Record it on the commit whose behaviour is the yardstick, BEFORE changing the wrappers; afterwards the test must pass against the
unchanged file.  Normalisation: c_void_p and integers are their value (NULL is 0), byref(...) is "byref", ctypes arrays are lists,
an address the stand-in did not hand out and the case did not choose is "host"; what modgpu_h2d uploads is named by a hash of its
bytes, so the tables the DeviceBuffer methods build are compared too."""
import ctypes
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from modulate_amd import capi  # noqa: E402

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "capi_wrapper_calls.json")
# addresses the cases choose (all below 2^40: above that an address is host memory)
TB, RES, WS, EXP, SRC, DST, STREAM = 0x70000000, 0x71000000, 0x72000000, 0x73000000, 0x74000000, 0x75000000, 0x5151
KEY, KEY2 = capi.KEY_PS4, capi.KEY_PS3
NONE64 = (1 << 64) - 1


def norm(a):
    if isinstance(a, ctypes.Array):
        return [norm(x) for x in a]
    if type(a).__name__ == "CArgObject":
        return "byref"
    if isinstance(a, ctypes._Pointer):
        a = ctypes.cast(a, ctypes.c_void_p)
    if isinstance(a, ctypes._SimpleCData):
        a = a.value
        if isinstance(a, bytes):
            return a.decode()
    if a is None:
        return 0
    if isinstance(a, (int, np.integer)):
        return int(a) if int(a) < (1 << 40) or int(a) == NONE64 else "host"
    if isinstance(a, bytes):
        return a.decode()
    return a


class FakeLib:
    """every attribute is a function that records (name, normalised arguments) and returns 0, but for the few that have to answer"""

    def __init__(self):
        self.calls, self.next, self.rc = [], 0x10000, {}
        self.refused, self.stalled = NONE64, NONE64
        self.kept, self.closed = [], False

    def buf(self, nbytes, device=-1):
        """a DeviceBuffer of the case's own: kept alive, so that no modgpu_free of its __del__ lands among the wrapper's calls"""
        self.kept.append(capi.DeviceBuffer(nbytes, device))
        return self.kept[-1]

    def __getattr__(self, name):
        def fn(*args):
            if self.closed:
                return 0
            rec = [name, [norm(a) for a in args]]
            self.calls.append(rec)
            if name == "modgpu_alloc":
                args[0]._obj.value = self.next
                rec[1][0] = self.next
                self.next += (int(args[1]) + 0xFFF) // 0x1000 * 0x1000 + 0x1000
            elif name == "modgpu_h2d":
                rec.append(hashlib.sha256(ctypes.string_at(args[1].value, int(args[2]))).hexdigest()[:16])
            elif name.endswith("_workspace_bytes"):
                return 4096 + 64 * int(args[0]) + (int(args[1]) >> 8 if len(args) > 1 else 0)
            elif name in ("modgpu_table_status", "modgpu_move_status"):
                args[2]._obj.value = self.refused if name == "modgpu_table_status" else self.stalled
                return 1 if self.refused != NONE64 else 3 if self.stalled != NONE64 else 0
            elif name == "modgpu_rekey_move_table_status":
                args[2]._obj.value, args[3]._obj.value = self.refused, self.stalled
                return 1 if self.refused != NONE64 else 3 if self.stalled != NONE64 else 0
            elif name == "modgpu_last_error":
                return b"boom"
            elif name in ("modgpu_verify_results", "modgpu_digest_results") and args[1]:
                ctypes.memset(args[3], 1, 32 * int(args[1]))
                if name == "modgpu_digest_results":
                    ctypes.memset(args[4], 2, 4 * int(args[1]))
            elif name.startswith("modgpu_time_"):
                args[-1]._obj.value = 1.5
            return self.rc.get(name, 0)
        return fn


def host_table(dtype, count=3):
    t = np.zeros(count, dtype=dtype)
    for i in range(count):
        t[i]["dst"], t[i]["src"], t[i]["n"] = DST + 0x1000 * i, SRC + 0x1000 * i, (100, 0, 300)[i % 3]
    return t


# the seven table wrappers: (entry dtype, keyword of the results buffer or None, has check=, name of the main C call)
TABLE_CALLS = {
    "cycle_table_device": (capi.TABLE_DTYPE, None, True),
    "rekey_table_device": (capi.REKEY_TABLE_DTYPE, None, True),
    "rekey_move_table_device": (capi.REKEY_TABLE_DTYPE, None, True),
    "verify_table_device": (capi.TABLE_DTYPE, "results", False),
    "verify_rekey_table_device": (capi.REKEY_TABLE_DTYPE, "results", False),
    "digest_table_device": (capi.TABLE_DTYPE, "results", False),
    "cycle_digest_table_device": (capi.TABLE_DTYPE, "records", False),
}
CASES = {}


def case(name):
    def deco(f):
        assert name not in CASES
        CASES[name] = f
        return f
    return deco


def _table_cases(w, dtype, res_kw, has_check):
    fn = lambda *a, **k: getattr(capi, w)(*a, **k)  # noqa: E731  (looked up at call time)
    move = w == "rekey_move_table_device"
    resident = dict({res_kw: RES} if res_kw else {}, stream=STREAM, n=3, **({"total_bytes": 400} if move else {}))
    CASES[w + "/host3"] = lambda fake: fn(host_table(dtype))
    CASES[w + "/host3_stream_device"] = lambda fake: fn(host_table(dtype), device=1, stream=STREAM)
    CASES[w + "/empty"] = lambda fake: fn(host_table(dtype, 0))
    CASES[w + "/resident_ws_addr"] = lambda fake: fn(TB, workspace=WS, **resident)
    CASES[w + "/resident_ws_buffer"] = lambda fake: fn(fake.buf(120), workspace=fake.buf(8192), **resident)
    CASES[w + "/resident_own_ws"] = lambda fake: fn(TB, **resident)
    CASES[w + "/resident_n0"] = lambda fake: fn(TB, **dict(resident, n=0))
    CASES[w + "/resident_without_n"] = lambda fake: fn(TB, workspace=WS, **dict(resident, n=None))
    if move:
        CASES[w + "/resident_without_total_bytes"] = lambda fake: fn(TB, workspace=WS, stream=STREAM, n=3)
        CASES[w + "/host3_total_bytes_given"] = lambda fake: fn(host_table(dtype), 1 << 20)

        def stalled(fake):
            fake.stalled = 7
            return fn(host_table(dtype))
        CASES[w + "/stalled"] = stalled
    if res_kw:
        CASES[w + "/host3_own_ws_given_results"] = lambda fake: fn(host_table(dtype), **{res_kw: RES})

    def refused(fake):
        fake.refused = 2
        return fn(host_table(dtype))
    CASES[w + "/refused"] = refused

    def failed(fake):
        fake.rc["modgpu_" + w] = 5
        return fn(host_table(dtype))
    CASES[w + "/call_fails"] = failed
    if has_check:
        CASES[w + "/check_false"] = lambda fake: fn(host_table(dtype), check=False)

        def invalid(fake):
            fake.rc["modgpu_" + {"cycle_table_device": "table", "rekey_table_device": "rekey_table",
                                 "rekey_move_table_device": "rekey_move_table"}[w] + "_validate"] = 2
            return fn(host_table(dtype))
        CASES[w + "/validate_fails"] = invalid
    if w == "cycle_digest_table_device":
        for side in (capi.DIGEST_OUTPUT, capi.DIGEST_INPUT):
            CASES[w + f"/resident_side{side}"] = lambda fake, side=side: fn(TB, RES, side, WS, -1, STREAM, n=3)
            CASES[w + f"/host3_side{side}"] = lambda fake, side=side: fn(host_table(dtype), side=side)


for _w, _spec in TABLE_CALLS.items():
    _table_cases(_w, *_spec)


# the own-result single-entry calls: name -> the arguments between (expect, src) and result
for _w, _mid in (("verify_device", (KEY, 7)), ("verify_rekey_device", (KEY, KEY2, 7, 9))):
    def _single(w=_w, mid=_mid):
        fn = lambda *a, **k: getattr(capi, w)(*a, **k)  # noqa: E731
        CASES[w + "/own_result"] = lambda fake: fn(EXP, SRC, *mid, n=100)
        CASES[w + "/given_result"] = lambda fake: fn(EXP, SRC, *mid, RES, 1, STREAM, n=100)
        CASES[w + "/given_result_buffer"] = lambda fake: fn(EXP, SRC, *mid, fake.buf(32), n=100)
        CASES[w + "/n_from_buffers"] = lambda fake: fn(fake.buf(500), fake.buf(300), *mid)
        CASES[w + "/n_missing"] = lambda fake: fn(EXP, fake.buf(300), *mid)
        CASES[w + "/n_missing_given_result"] = lambda fake: fn(fake.buf(300), SRC, *mid, RES)

        def failed(fake):
            fake.rc["modgpu_" + w] = 5
            return fn(EXP, SRC, *mid, n=100)
        CASES[w + "/call_fails"] = failed
    _single()


def _digest_cases():
    fn = lambda *a, **k: capi.digest_device(*a, **k)  # noqa: E731
    CASES["digest_device/own_result"] = lambda fake: fn(SRC, KEY, 7, n=100)
    CASES["digest_device/own_result_dst"] = lambda fake: fn(SRC, KEY, 7, DST, n=100)
    CASES["digest_device/given_result"] = lambda fake: fn(SRC, KEY, 7, None, RES, 1, STREAM, n=100)
    CASES["digest_device/given_result_dst"] = lambda fake: fn(SRC, KEY, 7, DST, fake.buf(32), 1, STREAM, n=100)
    CASES["digest_device/n_from_src"] = lambda fake: fn(fake.buf(500), KEY)
    CASES["digest_device/n_from_src_and_dst"] = lambda fake: fn(fake.buf(500), KEY, dst=fake.buf(300))
    CASES["digest_device/n_missing"] = lambda fake: fn(SRC, KEY)
    CASES["digest_device/n_missing_dst_address"] = lambda fake: fn(fake.buf(500), KEY, dst=DST)

    def failed(fake):
        fake.rc["modgpu_digest_device"] = 5
        return fn(SRC, KEY, 7, n=100)
    CASES["digest_device/call_fails"] = failed


_digest_cases()

P3, Q3, Z3, O3, O3B = [DST, DST + 0x100, DST + 0x200], [SRC, SRC + 0x100, SRC + 0x200], [10, 0, 30], [1, 2, 3], [4, 5, 6]


@case("cycle_batch_device/offsets")
def _(fake):
    return capi.cycle_batch_device(P3, Z3, KEY, O3, 1, STREAM)


@case("cycle_batch_device/no_offsets")
def _(fake):
    return capi.cycle_batch_device(P3, Z3, KEY)


@case("cycle_batch_device_to/offsets")
def _(fake):
    return capi.cycle_batch_device_to(P3, Q3, Z3, KEY, O3, 1, STREAM)


@case("cycle_batch_device_to/no_offsets")
def _(fake):
    return capi.cycle_batch_device_to(P3, Q3, Z3, KEY)


@case("rekey_batch_device_to/offsets")
def _(fake):
    return capi.rekey_batch_device_to(P3, Q3, Z3, KEY, KEY2, O3, O3B, 1, STREAM)


@case("rekey_batch_device_to/no_offsets_buffers")
def _(fake):
    return capi.rekey_batch_device_to([fake.buf(64), DST, DST + 64], [SRC, fake.buf(64), SRC + 64], Z3, KEY, KEY2)


@case("rekey_batch_device_to/one_offset_list")
def _(fake):
    return capi.rekey_batch_device_to(P3, Q3, Z3, KEY, KEY2, offs_to=O3B)


@case("verify_batch_device/offsets")
def _(fake):
    return capi.verify_batch_device(P3, Q3, Z3, KEY, RES, O3, 1, STREAM)


@case("verify_batch_device/no_offsets_buffers")
def _(fake):
    return capi.verify_batch_device([fake.buf(64), EXP, EXP + 64], Q3, Z3, KEY, fake.buf(96))


@case("verify_rekey_batch_device/offsets")
def _(fake):
    return capi.verify_rekey_batch_device(P3, Q3, Z3, KEY, KEY2, RES, O3, O3B, 1, STREAM)


@case("verify_rekey_batch_device/no_offsets")
def _(fake):
    return capi.verify_rekey_batch_device(P3, Q3, Z3, KEY, KEY2, fake.buf(96))


@case("verify_rekey_batch_device/one_offset_list")
def _(fake):
    return capi.verify_rekey_batch_device(P3, Q3, Z3, KEY, KEY2, RES, offs_from=O3)


@case("digest_batch_device/digest_only")
def _(fake):
    return capi.digest_batch_device(Q3, Z3, KEY, RES)


@case("digest_batch_device/some_dst")
def _(fake):
    return capi.digest_batch_device(Q3, Z3, KEY, RES, [DST, None, 0], O3, 1, STREAM)


@case("digest_batch_device/buffers")
def _(fake):
    return capi.digest_batch_device([fake.buf(64), SRC, SRC + 64], Z3, KEY, fake.buf(96), [fake.buf(64), None, DST])


@case("digest_batch_device/empty")
def _(fake):
    return capi.digest_batch_device([], [], KEY, RES, [])


# every time_* wrapper, each argument of its signature given positionally with a value of its own; the workspace once as an address
# (its size is then asked of the library) and once as a DeviceBuffer
TIMED = {
    "time_cycle_device": lambda ws: (SRC, 100, KEY, 7),
    "time_cycle_device_to": lambda ws: (DST, SRC, 100, KEY, 7),
    "time_rekey_device_to": lambda ws: (DST, SRC, 100, KEY, KEY2, 7, 9),
    "time_cycle_table_device": lambda ws: (TB, 3, ws),
    "time_rekey_table_device": lambda ws: (TB, 3, ws),
    "time_verify_device": lambda ws: (EXP, SRC, 100, KEY, RES, 7),
    "time_digest_device": lambda ws: (SRC, 100, KEY, RES, DST, 7),
    "time_verify_rekey_device": lambda ws: (EXP, SRC, 100, KEY, KEY2, RES, 7, 9),
    "time_verify_table_device": lambda ws: (TB, 3, RES, ws),
    "time_digest_table_device": lambda ws: (TB, 3, RES, ws),
    "time_cycle_digest_table_device": lambda ws: (TB, 3, RES, ws, capi.DIGEST_INPUT),
    "time_verify_rekey_table_device": lambda ws: (TB, 3, RES, ws),
}
for _w, _args in TIMED.items():
    CASES[_w + "/address"] = lambda fake, w=_w, args=_args: getattr(capi, w)(*args(WS), 1, STREAM, 5)
    CASES[_w + "/buffers_defaults"] = lambda fake, w=_w, args=_args: getattr(capi, w)(
        *[fake.buf(64) if isinstance(x, int) and x >= TB else x for x in args(fake.buf(8192))])
CASES["time_digest_device/digest_only"] = lambda fake: capi.time_digest_device(SRC, 100, KEY, RES)

RANGES = [(0, 100), (4096, 0), (8192, 333)]


@case("DeviceBuffer.digests")
def _(fake):
    return fake.buf(1 << 16, 1).digests(RANGES, KEY, 1000, None, STREAM)


@case("DeviceBuffer.digests/workspace")
def _(fake):
    return fake.buf(1 << 16).digests(RANGES, KEY, workspace=WS)


@case("DeviceBuffer.extract")
def _(fake):
    return fake.buf(1 << 16, 1).extract(RANGES, KEY, fake.buf(1 << 12, 1), 1000, capi.DIGEST_INPUT, None, STREAM)


@case("DeviceBuffer.extract/in_place")
def _(fake):
    b = fake.buf(1 << 16)
    return b.extract(RANGES, KEY, b, workspace=fake.buf(8192))


@case("DeviceBuffer.compact")
def _(fake):
    return fake.buf(1 << 16, 1).compact([(256, 100), (4096, 50), (8192, 333)], KEY, 1000, None, STREAM)


@case("DeviceBuffer.compact/workspace_nothing_kept")
def _(fake):
    b = fake.buf(1 << 16)
    return [b.compact([(256, 100), (4096, 50)], KEY, workspace=WS), b.compact([], KEY)]


@case("DeviceBuffer.compact/falling_ranges")
def _(fake):
    return fake.buf(1 << 16).compact([(4096, 50), (256, 100)], KEY)


@case("DeviceBuffer.move")
def _(fake):
    return fake.buf(1 << 16, 1).move(0, 100, 5000, KEY, KEY2, 7, 9, None, STREAM)


@case("DeviceBuffer.move/workspace_defaults")
def _(fake):
    b = fake.buf(1 << 16)
    return [b.move(0, 100, 5000, workspace=WS), b.move(0, 100, 5000, workspace=fake.buf(8192)), b.move(0, 100, 0)]


@case("DeviceBuffer.move/stalled")
def _(fake):
    fake.stalled = 4
    return fake.buf(1 << 16).move(0, 100, 5000)


@case("DeviceBuffer.digest")
def _(fake):
    return fake.buf(1 << 16, 1).digest(KEY, 100, 64, 7, STREAM)


def plain(v):
    """a return value as JSON"""
    if isinstance(v, np.ndarray):
        return {"dtype": str(v.dtype), "data": plain(v.tolist())}
    if isinstance(v, (tuple, list)):
        return [plain(x) for x in v]
    if isinstance(v, np.generic):
        return {"dtype": str(v.dtype), "data": plain(v.tolist())}
    return v


def run(name, monkeypatch=None):
    fake = FakeLib()
    if monkeypatch is not None:
        monkeypatch.setattr(capi, "lib", lambda: fake)
        out = _outcome(name, fake)
    else:
        real, capi.lib = capi.lib, lambda: fake
        try:
            out = _outcome(name, fake)
        finally:
            capi.lib = real
    fake.closed = True
    allocs = [c[1][0] for c in fake.calls if c[0] == "modgpu_alloc"]
    frees = [c[1][0] for c in fake.calls if c[0] == "modgpu_free"]
    out["calls"] = fake.calls
    out["not_freed"] = sorted(set(allocs) - set(frees) - {b.ptr for b in fake.kept})  # of the buffers the WRAPPER made
    return json.loads(json.dumps(out))


def _outcome(name, fake):
    try:
        return {"returns": plain(CASES[name](fake)), "raises": None}
    except Exception as e:  # noqa: BLE001  (the exception is what is recorded)
        return {"returns": None, "raises": [type(e).__name__, getattr(e, "code", None), str(e)]}


def signatures():
    names = sorted({n.split("/")[0] for n in CASES if not n.startswith("DeviceBuffer")})
    sig = {n: str(inspect.signature(getattr(capi, n))) for n in names}
    for m in ("digest", "digests", "extract", "compact", "move"):
        sig["DeviceBuffer." + m] = str(inspect.signature(getattr(capi.DeviceBuffer, m)))
    return sig


def expected():
    with open(EXPECTED) as f:
        return json.load(f)


def test_every_case_is_recorded():
    assert sorted(expected()["cases"]) == sorted(CASES)


def test_signatures():
    assert signatures() == expected()["signatures"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_wrapper(name, monkeypatch):
    got, want = run(name, monkeypatch), expected()["cases"][name]
    assert got["raises"] == want["raises"]
    assert got["calls"] == want["calls"]
    assert got["returns"] == want["returns"]
    assert got["not_freed"] == want["not_freed"] == [], "a wrapper frees every buffer it made, whatever happened"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    doc = {"signatures": signatures(), "cases": {n: run(n) for n in sorted(CASES)}}
    with open(EXPECTED, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("recorded", len(CASES), "cases,", os.path.getsize(EXPECTED), "bytes")
