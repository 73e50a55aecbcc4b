"""The single host-buffer calls and the single transfers on the CPU stand-in of the HIP runtime, as a stand-alone program
(tests/host_calls_main.cpp: its own main, run directly, the sanitizer runtimes linked statically: the environment's preloads are left
alone): every shape of call and every route of modulate_amd/csrc/host_stream.cpp at the smallest size that still takes it, injected
failures at every stage, refused launches, the staging set of another NUMA node and a list call cut into two windows run clean under
ASan + UBSan and under TSan, every byte against a model.  Each line also prints what the call's plan led to and nothing that depends
on the run, so that the output of two commits can be compared byte for byte when host_stream.cpp is reshaped."""
import os
import subprocess

import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
CASES = 120


def _whats():
    whats = ["the chunk size from the host trace", "page-locked in place", "one slot, at the limit", "one slot, one below the limit",
             "one slot, page-locked source is cycled in place all the same", "feed, one piece", "feed, 2 x pipes x chunk + 17",
             "slot_kernel, one piece", "slot_kernel, five chunks behind a ramp", "dma, pageable on both sides",
             "dma, page-locked source to a file", "dma, a file to a page-locked destination", "dma, page-locked in place on the ring",
             "file to pageable", "file to page-locked, through the slots", "file to page-locked, in_dst", "file to pageable, a launch per chunk",
             "pageable to file", "file to file", "identity key in place: nothing to do", "identity key out of place, file to pageable",
             "identity key out of place, page-locked to file", "stream_off at 2^64 - 3", "stream_off at 2^64 - 3, page-locked", "n = 0",
             "a device pointer that is host memory, up", "a device pointer that is host memory, down",
             "all pipeline slots but two held", "the held slots given back",
             "a refused launch, one pipeline: the error stands", "a refused launch, one pipeline, the host loop behind it",
             "a refused launch with several pipelines: the launch's text wins over a pipeline's",
             "a refused launch with several pipelines, the host loop behind it",
             "no worker threads to be had: not the feed route", "no worker threads to be had: a transfer of one pipeline",
             "injected failure before anything is touched, host buffer", "injected failure before anything is touched, transfer",
             "injected failure before anything is touched, list", "a good call after the failures",
             "the staging set of another node, host buffer", "the staging set of another node, transfer",
             "the staging set of another node, list of two windows, up", "the GPU's own set again"]
    for d in ("up", "down"):
        whats += [f"transfer {d}, {w}" for w in ("pageable, one piece", "page-locked, one piece", "page-locked, 2 x pipes x chunk + 17",
                                                  "a file on the host side", "identity key", "identity key, page-locked", "DMA form, pageable",
                                                  "DMA form, page-locked")]
        whats += [f"transfer {d}, pageable, 2 x pipes x chunk + 17, device phase {p}" for p in (0, 1, 15)]
        whats += [f"a refused transfer launch, one pipeline, {d}", f"a refused transfer launch with several pipelines, {d}",
                  f"a refused transfer launch on page-locked memory, {d}"]
        whats += [f"list of three entries in two windows, the second clipped, {d}", f"list digest of three entries in two windows, the second clipped, {d}"]
    for piece in ("0", "middle", "last"):
        for stage in ("fill", "launch", "sync", "drain", "after-drain"):
            whats.append(f"injected failure on feed, piece {piece} stage {stage}")
            whats.append(f"injected failure on xfer down, piece {piece} stage {stage}")
            if stage != "drain":  # (an upload has nothing to drain)
                whats.append(f"injected failure on xfer up, piece {piece} stage {stage}")
    return whats


def _run_main(flavour, env_extra):
    env = dict(os.environ, MODGPU_REQUIRE_GPU="0", **env_extra)
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW", "MODGPU_HOST_PIPES", "MODGPU_HOST_CHUNK_MB"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "host_calls_main_" + flavour)], env=env, capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1].endswith(", 0 failed") and int(lines[-1].split()[0]) == len(lines) - 1 == CASES, lines[-1]
    whats = _whats()
    assert len(whats) + 3 == CASES  # (+ the three "... and its text" lines behind the refused launches with several pipelines)
    for what in whats:
        assert any(ln == f"ok   {what}" or ln.startswith(f"ok   {what} | ") for ln in lines), what
    assert sum(ln == "ok   ... and its text" for ln in lines) == 3


def test_host_calls_on_the_standin_under_asan_ubsan():
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "../_san/host_calls_main_asan"])
    _run_main("asan", {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})


def test_host_calls_on_the_standin_under_tsan():
    if not B.sanitizer_runtime("libtsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "../_san/host_calls_main_tsan"])
    _run_main("tsan", {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1 suppressions=" + os.path.join(ROOT, "tests", "tsan.supp")})
