"""CPU checks of the digest check (modgpu_digest_check_device & co., include/modgpu.h): the symbols are declared, exported and listed,
the summary is 32 bytes, the bitmap's size, tier 1 comes before any device work, the verify table TU's code-generation guard still
passes the finish kernel with its extra branch and still rejects both broken builds, the host code runs under ASan + UBSan against the
CPU stand-in of the HIP runtime as a stand-alone program (its own main, run directly, the sanitizer runtimes linked statically), and
the Python wrappers make the C calls they promise, on the recording stand-in of tests/test_capi_wrappers_cpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _csrc_build as B
import test_capi_wrappers_cpu as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
MAX_ENTRIES = 1 << 22  # MODGPU_TABLE_MAX_ENTRIES
PUBLIC = {"modgpu_digest_check_bits_bytes", "modgpu_digest_check_device", "modgpu_digest_check_summary"}
TESTING = {"modgpu_time_digest_check_device"}


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_symbols_declared_exported_and_listed(modgpu):
    pub = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    tst = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    for s in PUBLIC:
        assert re.search(r"\b%s\(" % s, pub) and s in modgpu.EXPORTS, s
    for s in TESTING:
        assert re.search(r"\b%s\(" % s, tst) and s in modgpu.TESTING_EXPORTS, s
    assert "19 = the check launch of modgpu_digest_check_device" in tst and "modgpu_verify_table_kernel_source_hash() for variant 19" in tst
    assert "} modgpu_digest_check_summary_t;" in pub
    shipped, hooks = exported(modgpu.lib_path("shipped")), exported(modgpu.lib_path("testing"))
    assert PUBLIC | TESTING <= shipped and PUBLIC | TESTING <= hooks
    assert modgpu.lib().modgpu_abi_version() == 8
    for f in ("digest_check_device", "digest_check_result", "digest_check_bits_bytes", "time_digest_check_device"):
        assert callable(getattr(modgpu, f)), f
    assert callable(modgpu.DeviceBuffer.check) and callable(modgpu.DeviceBuffer.extract_checked)


def test_summary_is_32_bytes(modgpu):
    class Summary(ctypes.Structure):  # the four fields of include/modgpu.h, in its order
        _fields_ = [(k, ctypes.c_uint64) for k in ("bad_entries", "first_bad_entry", "entries", "refused")]
    assert ctypes.sizeof(Summary) == 32 == modgpu.DIGEST_CHECK_SUMMARY_DTYPE.itemsize
    assert [Summary.bad_entries.offset, Summary.first_bad_entry.offset, Summary.entries.offset, Summary.refused.offset] == [0, 8, 16, 24]
    assert list(modgpu.DIGEST_CHECK_SUMMARY_DTYPE.names) == [k for k, _ in Summary._fields_]
    pub = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    body = pub[pub.index("typedef struct modgpu_digest_check_summary {"):pub.index("} modgpu_digest_check_summary_t;")]
    assert re.findall(r"uint64_t (\w+);", body) == [k for k, _ in Summary._fields_]
    capi = open(os.path.join(CSRC, "modgpu_capi.cpp")).read()
    assert "static_assert(sizeof(modgpu_digest_check_summary_t) == 32 && sizeof(CycleVerifyResult) == 32" in capi


def test_bits_bytes(modgpu):
    want = {0: 0, 1: 8, 64: 8, 65: 16, MAX_ENTRIES: MAX_ENTRIES // 8, MAX_ENTRIES + 1: 0}
    assert {n: modgpu.digest_check_bits_bytes(n) for n in want} == want


def test_without_a_gpu_the_call_fails_with_no_device(modgpu):
    """Tier 1 comes first (MODGPU_ERR_INVALID, nothing queued); a well-formed call gets as far as the device and fails there."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    L = modgpu.lib()
    rec, exp, out = np.zeros(4 * 70, np.uint64), np.zeros(70, np.uint32), np.zeros(16, np.uint64)
    r, e, s, b = rec.ctypes.data, exp.ctypes.data, out.ctypes.data, out.ctypes.data + 64
    before = modgpu.path_stats()
    texts = []

    def refused(*args):
        assert L.modgpu_digest_check_device(*args, -1, None) == 1, args
        texts.append(L.modgpu_last_error().decode())
    refused(None, e, 70, None, s, b)
    refused(r, None, 70, None, s, b)
    refused(r, e, 70, None, None, b)
    refused(r + 4, e, 69, None, s, b)
    refused(r, e, 70, None, s + 4, b)
    refused(r, e, 70, None, s, b + 4)
    refused(r, e + 2, 69, None, s, b)
    refused(r, e, 70, s + 4, s, b)
    refused(r, e, MAX_ENTRIES + 1, None, s, b)
    refused(r, e, 70, None, r + 32, b)
    refused(r, e, 70, None, s, e)
    refused(r, e, 70, None, s, s + 24)
    assert [t.split(": ")[-1] for t in texts] == ["null records, manifest or summary"] * 3 + ["records, summary or bits not 8-byte aligned"] * 3 + [
        "manifest not 4-byte aligned", "table workspace not 8-byte aligned", "more entries than a table call takes (4194304)"] + [
        "the summary or the bits overlap the records, the manifest or each other"] * 3, texts
    assert L.modgpu_digest_check_device(None, None, 0, None, None, None, -1, None) == 0
    assert L.modgpu_digest_check_device(r, e, 70, None, s, b, -1, None) == 2  # MODGPU_ERR_NO_DEVICE
    assert L.modgpu_digest_check_device(r, e, 70, None, s, None, -1, None) == 2
    assert L.modgpu_digest_check_summary(None, -1, s) == 1 and L.modgpu_digest_check_summary(s, -1, None) == 1
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] and st["scalar_calls"] == before["scalar_calls"]
    assert not rec.any() and not exp.any() and not out.any()


def test_codegen_guard_still_passes_and_still_rejects():
    """`make isa-check-verify-table` passes the tree (still 3 kernels: the check is a mode of the finish kernel); both broken builds of
    the TU are still made -- their sed anchors still match -- and still rejected; the stand-in is wired, and is no row of TABLE."""
    B.isa_check_target("isa-check-verify-table", 3)
    for target, words in (("isa-check-broken-verify-table", "a verify kernel stores through a buffer descriptor"), ("isa-check-broken-verify-table-digest", "a store in the kernel of the digest loop")):
        broken = subprocess.run(["make", "-s", "-C", CSRC, target], capture_output=True, text=True, timeout=900)
        assert broken.returncode != 0, f"the guard accepted {target}"
        assert words in broken.stdout, broken.stdout[-3000:] + broken.stderr[-2000:]
    B.standin_is_wired("standin_launch_digest_check.cpp")
    assert "digest_check" not in B.make_var("TUS").split()
    hip = open(os.path.join(CSRC, "cycle_verify_table_kernel.hip")).read()
    assert hip.count("__global__") == 3 and "VERIFY_TABLE_CHECK" in hip


def test_the_check_in_the_finish_kernels_assembly():
    """The finish kernel's own atomics: the refusal's min, the compare mode's pair and the check's pair -- none returns its value; the
    check takes the wave's word from one 64-bit ballot (s_bcnt1 / s_ff1 of it), with no LDS traffic of its own."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_verify_table_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_verify_table_kernel.s")).read()
    assert ci.check(asm) == []
    finish = next(body for name, body in ci.kernel_bodies(asm).items() if "modgpu_cycle_verify_table_finish" in name)
    atomics = re.findall(r"^\s+(global_atomic_\w+) .*$", finish, re.M)
    assert sorted(atomics) == ["global_atomic_add_x2"] * 2 + ["global_atomic_umin_x2"] * 3, atomics
    assert not [ln for ln in re.findall(r"^\s+global_atomic_.*$", finish, re.M) if " sc0" in ln]
    assert "s_bcnt1_i32_b64" in finish and "s_ff1_i32_b64" in finish


def test_digest_check_on_the_standin_under_asan_ubsan():
    """tests/digest_check_main.cpp: synthetic records at the lane, wave and workgroup edges with nothing, the first, the last and every
    entry bad; the digest table stand-in's records end to end; a refused producer; every host refusal with its text; the summary, every
    word of the bitmap and the guard bytes against a model."""
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "digest-check-main"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", MODGPU_REQUIRE_GPU="0")
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "digest_check_main")], env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1] == f"{len(lines) - 1} passed, 0 failed" and len(lines) - 1 == 60, lines[-1]
    for n in (1, 63, 64, 65, 1023, 1024, 1025):
        for plant in ("clean", "first bad", "last bad", "all bad"):
            assert f"ok   digest check: synthetic n={n} {plant}" in lines, (n, plant)
    for what in ("digest table records: clean", "digest table records: a source byte of entry 0 flipped", "digest table records: a source byte of entry 69 flipped",
                 "refused producer", "refusal: too many entries", "refusal: null records", "refusal: null manifest", "refusal: null summary",
                 "refusal: misaligned records", "refusal: misaligned summary", "refusal: misaligned bits", "refusal: misaligned manifest",
                 "refusal: misaligned table workspace", "refusal: summary inside the records", "refusal: summary inside the manifest",
                 "refusal: bits inside the records", "refusal: bits inside the manifest", "refusal: bits over the summary",
                 "refusal: records that are not device memory", "refusal: manifest that is not device memory", "refusal: summary that is not device memory",
                 "refusal: bits that are not device memory", "refusal: table workspace that is not device memory", "refusal: summary read from host memory",
                 "refusal: timing without iterations", "refusals queued nothing"):
        assert any(ln.startswith(f"ok   digest check: {what}") for ln in lines), what
    assert "ok   bitmap sizes" in lines and lines[-2].startswith("ok   launches: ") and lines[-2].endswith(", 0 plan errors")


# ---- the wrappers' C calls, on the recording stand-in ------------------------------------------------------------------------------
REC, EXP, SUM, BITS, WS, STREAM = W.RES, W.EXP, 0x76000000, 0x77000000, W.WS, W.STREAM
ADLERS = np.array([11, 22, 33], dtype=np.uint32)


class Fake(W.FakeLib):
    """FakeLib, answering the two calls that report a check: a summary of `bad` (a set of entries), and their bitmap"""

    def __init__(self, bad=(), refused_check=False):
        super().__init__()
        self.bad, self.refused_check = sorted(bad), refused_check

    def __getattr__(self, name):
        fn = super().__getattr__(name)

        def answer(*args):
            rc = fn(*args)
            if self.closed:
                return rc
            if name == "modgpu_digest_check_summary":
                out = np.array([(len(self.bad), self.bad[0] if self.bad else W.NONE64, 3, int(self.refused_check))], dtype=W.capi.DIGEST_CHECK_SUMMARY_DTYPE)
                ctypes.memmove(args[2], out.ctypes.data, 32)
                return 1 if self.refused_check else rc
            if name == "modgpu_d2h":
                words = np.zeros(int(args[2]) // 8, dtype="<u8")
                for i in self.bad:
                    words[i // 64] |= np.uint64(1 << (i % 64))
                ctypes.memmove(args[0], words.ctypes.data, words.nbytes)
            return rc
        return answer


def calls_of(fake, f):
    real, W.capi.lib = W.capi.lib, lambda: fake
    try:
        out = f(fake)
    finally:
        W.capi.lib = real
        fake.closed = True
    allocs = {c[1][0] for c in fake.calls if c[0] == "modgpu_alloc"}
    frees = {c[1][0] for c in fake.calls if c[0] == "modgpu_free"}
    assert allocs - frees - {b.ptr for b in fake.kept} == set(), "a wrapper frees every buffer it made"
    return out, [c[0].replace("modgpu_", "") for c in fake.calls], fake.calls


def triple(t):
    return t[0], t[1], None if t[2] is None else t[2].tolist()


def test_wrapper_digest_check_device_own_summary():
    out, names, calls = calls_of(Fake({1, 2}), lambda fake: W.capi.digest_check_device(REC, ADLERS, 3, WS, device=1, stream=STREAM))
    assert triple(out) == (2, 1, [1, 2])
    assert names == ["alloc", "alloc", "h2d", "digest_check_bits_bytes", "alloc", "digest_check_device", "sync", "digest_check_summary", "d2h", "free", "free", "free"]
    summary, manifest, bits = (c[1][0] for c in calls if c[0] == "modgpu_alloc")
    assert [c[1][1] for c in calls if c[0] == "modgpu_alloc"] == [32, 12, 8]
    assert calls[5][1] == [REC, manifest, 3, WS, summary, bits, 1, STREAM] and calls[6][1] == [1, STREAM]
    assert calls[7][1] == [summary, 1, "host"] and calls[8][1] == ["host", bits, 8, 1]
    # clean: 32 bytes come back and no bitmap; a manifest and a bitmap in device memory are used as they are
    out, names, calls = calls_of(Fake(), lambda fake: W.capi.digest_check_device(REC, EXP, 3, bad_bits=BITS))
    assert triple(out) == (0, None, [])
    assert names == ["alloc", "digest_check_device", "sync", "digest_check_summary", "free"]
    assert calls[1][1] == [REC, EXP, 3, 0, calls[0][1][0], BITS, -1, 0]
    # no entries: no call at all
    out, names, _ = calls_of(Fake(), lambda fake: W.capi.digest_check_device(REC, EXP, 0))
    assert triple(out) == (0, None, []) and names == []


def test_wrapper_digest_check_device_asynchronous_and_refused():
    out, names, calls = calls_of(Fake(), lambda fake: W.capi.digest_check_device(REC, EXP, 3, WS, SUM, None, 1, STREAM))
    assert out is None and names == ["digest_check_device"] and calls[0][1] == [REC, EXP, 3, WS, SUM, 0, 1, STREAM]
    out, names, calls = calls_of(Fake({0}), lambda fake: W.capi.digest_check_result(SUM, 3, BITS, 1))
    assert triple(out) == (1, 0, [0]) and names == ["digest_check_summary", "d2h"] and calls[1][1] == ["host", BITS, 8, 1]
    out, names, _ = calls_of(Fake({2}), lambda fake: W.capi.digest_check_result(SUM, 3))
    assert triple(out) == (1, 2, None) and names == ["digest_check_summary"]
    with pytest.raises(W.capi.ModGpuError, match="boom"):
        calls_of(Fake(refused_check=True), lambda fake: W.capi.digest_check_device(REC, EXP, 3, WS))
    with pytest.raises(TypeError, match="manifest in device memory"):
        calls_of(Fake(), lambda fake: W.capi.digest_check_device(REC, ADLERS, 3, WS, SUM))
    assert calls_of(Fake(), lambda fake: W.capi.time_digest_check_device(REC, EXP, 3, SUM, BITS, WS, 1, STREAM, 5))[2] == [
        ["modgpu_time_digest_check_device", [REC, EXP, 3, WS, SUM, BITS, 1, STREAM, 5, "byref"]]]


def test_wrapper_device_buffer_check():
    """one digest table call and one check on the same stream, ONE synchronise, and no modgpu_digest_results: the records stay"""
    out, names, calls = calls_of(Fake({2}), lambda fake: fake.buf(1 << 16, 1).check(W.RANGES, W.KEY, ADLERS, 1000, None, STREAM))
    assert triple(out) == (1, 2, [2])
    assert names == ["alloc", "alloc", "h2d", "alloc", "digest_table_workspace_bytes", "alloc", "digest_table_device", "alloc", "alloc", "h2d",
                     "digest_check_bits_bytes", "alloc", "digest_check_device", "sync", "table_status", "digest_check_summary", "d2h"] + ["free"] * 6
    by = {c[0]: c[1] for c in calls}
    _, table, records, ws, summary, manifest, bits = (c[1][0] for c in calls if c[0] == "modgpu_alloc")
    assert by["modgpu_digest_table_device"] == [table, 3, records, ws, by["modgpu_digest_table_device"][4], 1, STREAM]
    assert by["modgpu_digest_check_device"] == [records, manifest, 3, ws, summary, bits, 1, STREAM] and by["modgpu_sync"] == [1, STREAM]
    # the table is DeviceBuffer.digests' table, byte for byte
    _, _, want = calls_of(W.FakeLib(), lambda fake: fake.buf(1 << 16, 1).digests(W.RANGES, W.KEY, 1000, None, STREAM))
    assert [c[2] for c in calls if c[0] == "modgpu_h2d"][0] == [c[2] for c in want if c[0] == "modgpu_h2d"][0]
    # the producer refused: the table call's own refusal is raised, and everything is freed
    fake = Fake()
    fake.refused = 1
    with pytest.raises(W.capi.ModGpuError, match="the device refused digest table entry 1"):
        calls_of(fake, lambda fake: fake.buf(1 << 16).check(W.RANGES, W.KEY, ADLERS))
    out, names, _ = calls_of(Fake(), lambda fake: fake.buf(1 << 16).check([], W.KEY, []))
    assert triple(out) == (0, None, []) and names == ["alloc"]


def test_wrapper_extract_checked_and_extract_as_it_was():
    f = lambda fake: fake.buf(1 << 16, 1).extract_checked(W.RANGES, W.KEY, fake.buf(1 << 12, 1), ADLERS, 1000, W.capi.DIGEST_INPUT, None, STREAM)  # noqa: E731
    (adlers, outcome), names, calls = calls_of(Fake({0, 2}), f)
    assert adlers.tolist() == [33686018] * 3 and triple(outcome) == (2, 0, [0, 2])
    assert names == ["alloc", "alloc", "alloc", "h2d", "alloc", "cycle_digest_table_workspace_bytes", "alloc", "cycle_digest_table_device", "alloc", "alloc", "h2d",
                     "digest_check_bits_bytes", "alloc", "digest_check_device", "sync", "table_status", "digest_results", "digest_check_summary", "d2h"] + ["free"] * 6
    by = {c[0]: c[1] for c in calls}
    assert by["modgpu_digest_check_device"][0] == by["modgpu_cycle_digest_table_device"][2] and by["modgpu_digest_check_device"][3] == by["modgpu_cycle_digest_table_device"][4]
    # without the check the sequence is the recorded one
    for name in ("DeviceBuffer.extract", "DeviceBuffer.extract/in_place"):
        got, want = W.run(name), W.expected()["cases"][name]
        assert got["calls"] == want["calls"] and got["returns"] == want["returns"] and got["raises"] is None
