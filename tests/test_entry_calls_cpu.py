"""CPU checks of what the five entry-list calls share on the host (modulate_amd/csrc/modgpu_capi.cpp: one planner, one run loop, one
results preamble, one copy of each check) and in the stand-ins (tests/cpu_runtime_standin/standin_entry.h): the out-of-place, rekey,
verify and rekey verify calls driven on the CPU stand-in of the HIP runtime by a stand-alone program under ASan + UBSan (its own main,
run directly, the sanitizer runtimes linked statically: the environment's preloads are left alone).  The digest calls have
tests/digest_main.cpp (tests/test_digest_cpu.py)."""
import os
import subprocess

import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
CALLS = ("cycle to", "rekey", "verify", "verify rekey")


def test_shared_pieces_exist_once():
    capi = open(os.path.join(CSRC, "modgpu_capi.cpp")).read()
    assert capi.count("a.start[k] = (uint32_t)p.total;") == 2  # plan_entries: an entry's own start, and the padding loop
    assert capi.count("for (int k = r.n; k <= kCycleBatchMax; ++k) a.start[k] = (uint32_t)p.total;") == 1
    assert capi.count('"an entry that spans 2^24 chunks') == 1
    assert capi.count('"result not 8-byte aligned"') == 1
    assert capi.count('"modgpu_cycle_verify_init"') == 1
    # (the host table validator has a copy of its own, reported per entry)
    assert capi.count('fail(MODGPU_ERR_INVALID, "destination partly overlaps its source') == 1 and capi.count('"a destination meets another entry') == 1
    assert capi.count("entry_geom(r.role[k]") == 1 and capi.count("template <class Keep, class Fn>") == 1
    standin = os.path.join(ROOT, "tests", "cpu_runtime_standin")
    texts = {f: open(os.path.join(standin, f)).read() for f in os.listdir(standin) if f.endswith((".cpp", ".h"))}
    six = ("standin_launch_to.cpp", "standin_launch_rekey.cpp", "standin_launch_verify.cpp", "standin_launch_rekey_verify.cpp",
           "standin_launch_to_digest.cpp", "standin_launch_rekey_move.cpp")
    assert texts["standin_entry.h"].count("(kChunk - 1)) != P.lead") == 1 and not [f for f in six if "!= P.lead" in texts[f]]
    assert [f for f in six if "b.start[p] != total" in texts[f]] == ["standin_launch_rekey_move.cpp"]  # (its one part's own rule: no edges, no lead)
    assert sorted(f for f, t in texts.items() if '#include "standin_entry.h"' in t) == [
        "standin_launch_rekey.cpp", "standin_launch_rekey_move.cpp", "standin_launch_rekey_verify.cpp", "standin_launch_to.cpp",
        "standin_launch_to_digest.cpp", "standin_launch_verify.cpp"]
    # the stand-ins stay a second implementation: the shared header is written from the record types and lcg.h, not from the device code
    assert "_impl.h" not in texts["standin_entry.h"].split("#pragma once")[1]
    assert "standin_entry.h" in B.make_var("SHIM_DEPS")


def test_entry_calls_on_the_standin_under_asan_ubsan():
    """tests/entry_calls_main.cpp: every size at every phase of the role pointer and the source, batches across the run boundary with
    empty entries, the degenerate keys, null offsets, the routes without a ticket pair, planted mismatches and every host refusal with
    its text, every byte of the arena and every result against a model; no plan error in any stand-in."""
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "entry-calls-main"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", MODGPU_REQUIRE_GPU="0")
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "entry_calls_main")], env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1].endswith(", 0 failed") and int(lines[-1].split()[0]) == len(lines) - 1 == 501, lines[-1]
    sizes = (0, 1, 15, 16, 17, 65535, 65536, 65536 + 17, 3 * 65536 + 77)
    for call in CALLS:
        whats = [f"size {n} at role phase {rp} src phase {sp} " for n in sizes for rp in (0, 1, 65535) for sp in (0, 3, 4)]
        whats += [f"batch of {n} entries=" for n in (1, 16, 17, 33)] + [f"batch of {n} with null offsets" for n in (1, 16, 17, 33)]
        whats += ["empty entries only", "no entries", "key_from == 0 mod m (0)", "key_from == 0 mod m (2147483647)", "ring exhausted, single",
                  "ring exhausted, batch of 17", "refusal: negative count", "refusal: null role list", "refusal: null source list", "refusal: null sizes",
                  "refusal: null role pointer in a batch", "refusal: null source in a batch", "refusal: a device that does not exist",
                  "refusals queued nothing and wrote nothing"]
        if call in ("rekey", "verify rekey"):
            whats += ["key_to == 0 mod m (0)", "both keys == 0 mod m (0)", "equal keys at equal and unequal offsets",
                      "keys equal mod m at equal and unequal offsets", "equal keys with null offsets", "equal keys a period apart, single"]
        if call in ("cycle to", "rekey"):
            whats += ["dst == src", "ring exhausted, in place", "refusal: partial overlap, dst above", "refusal: partial overlap, dst below",
                      "refusal: partial overlap by one byte", "refusal: two destinations meet", "refusal: a destination meets another entry's source",
                      "refusal: partial overlap before a later null", "refusal: null before a later partial overlap",
                      "refusal: partial overlap before a meeting", "refusal: partial overlap before the device"]
        else:
            whats += ["planted in the head", "planted in the body", "planted in the tail", "planted at the edges",
                      "planted across a batch of both kinds of entry", "planted across a batch under one identity key", "refusal: null result ",
                      "refusal: null results of a batch", "refusal: misaligned result ", "refusal: result in host memory ",
                      "refusal: result in host memory under an identity key", "refusal: 2^24 chunks ", "refusal: 2^24 chunks by the phase of expect",
                      "refusal: 2^41 bytes", "refusal: bad list before null result", "refusal: null result before a null buffer",
                      "refusal: misaligned result before a null buffer", "refusal: null buffer before a later oversized entry",
                      "refusal: oversized entry before a later null buffer", "refusal: misaligned result before the device"]
        for what in whats:
            assert any(ln.startswith(f"ok   {call}: {what}") for ln in lines), (call, what)
    # what every plan led to is on the case's line; in all of them no stand-in counted a plan error or a collision of ticket pairs
    assert all(" planerr=0 " in ln + " " and " coll=0 " in ln for ln in lines if " | " in ln)
    assert lines[-2].startswith("ok   launches: ")
