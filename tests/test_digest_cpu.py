"""CPU checks of the digest entry points (modgpu_digest_device / modgpu_digest_batch_device / modgpu_digest_results /
modgpu_digest_adler32, include/modgpu.h): the symbols are in both library flavours, the host's closing arithmetic is zlib's Adler-32,
argument validation happens before any device work, the out-of-place TU's code-generation guard passes the tree with the digest loop in
it and rejects a broken build and hand-made faults, and the host code runs clean under ASan + UBSan against the CPU stand-in of the HIP
runtime -- in a stand-alone program with its own main, run directly, the sanitizer runtimes linked statically."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import _csrc_build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")
PUBLIC = ("modgpu_digest_device", "modgpu_digest_batch_device", "modgpu_digest_results", "modgpu_digest_adler32")
P = 65521


def test_new_symbols_in_both_flavours_and_the_header(modgpu):
    for flavour in ("shipped", "testing"):
        out = subprocess.run(["nm", "-D", "--defined-only", modgpu.lib_path(flavour)], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(PUBLIC) | {"modgpu_time_digest_device"} <= names, (flavour, set(PUBLIC) - names)
        assert ("modgpu_debug_set_digest_grid" in names) == (flavour == "testing")
    assert set(PUBLIC) <= set(modgpu.EXPORTS) and "modgpu_time_digest_device" in modgpu.TESTING_EXPORTS
    assert "modgpu_debug_set_digest_grid" in modgpu.DEBUG_EXPORTS
    header = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    testing = open(os.path.join(ROOT, "include", "modgpu_testing.h")).read()
    assert all(name + "(" in header for name in PUBLIC) and "} modgpu_digest_result_t;" in header
    assert "modgpu_time_digest_device(" in testing and "modgpu_debug_set_digest_grid(" in testing and "16 = the digest loop" in testing
    assert modgpu.lib().modgpu_abi_version() == 8
    assert modgpu.DIGEST_RESULT_DTYPE.itemsize == 32 and modgpu.DIGEST_RESULT_DTYPE.names == ("s1", "s2", "n", "reserved")


@pytest.mark.parametrize("n", [0, 1, 65521, 100003])
def test_adler32_from_a_record_is_zlibs(modgpu, n):
    """Records built with numpy from random bytes -- S1 = sum of bytes, S2 = sum of j * byte_j -- reduced, and with multiples of 65521
    added to either word (only the residues are specified): modgpu_digest_adler32 gives zlib.adler32 of the bytes."""
    data = np.random.default_rng(n).integers(0, 256, size=n, dtype=np.uint8)
    want = zlib.adler32(data.tobytes()) & 0xFFFFFFFF
    s1 = int(data.sum(dtype=np.uint64))
    s2 = int((np.arange(n, dtype=np.uint64) * data).sum(dtype=np.uint64))  # < 100003^2 * 255: exact in 64 bits
    assert modgpu.digest_adler32((s1, s2, n)) == want                    # unreduced sums
    assert modgpu.digest_adler32((s1 % P, s2 % P, n)) == want            # reduced
    assert modgpu.digest_adler32((s1 % P + 3 * P, s2 % P + (1 << 44) * P, n)) == want
    assert modgpu.digest_adler32((s1 % P + ((1 << 64) - 1 - s1 % P) // P * P, s2 % P, n)) == want  # the largest word with that residue
    rec = np.zeros(1, modgpu.DIGEST_RESULT_DTYPE)
    rec["s1"], rec["s2"], rec["n"] = s1 % P, s2 % P, n
    assert modgpu.digest_adler32(rec[0]) == want
    if n == 0:
        assert want == 1 and modgpu.lib().modgpu_digest_adler32(None) == 1


def test_validation_comes_before_the_device(modgpu):
    """Without a GPU: a null source with bytes to read, a null or misaligned record, a partial overlap of dst and src and a batch whose
    destinations meet are MODGPU_ERR_INVALID (checked before any device work); every valid call is MODGPU_ERR_NO_DEVICE -- nothing is
    computed on the host."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    b = np.arange(256, dtype=np.uint8)
    keep = b.copy()
    res = np.full(8 * 4, 0xEE, np.uint64)
    before = modgpu.path_stats()
    p, r = b.ctypes.data, res.ctypes.data

    def code(fn, *args, **kw):
        with pytest.raises(modgpu.ModGpuError) as e:
            fn(*args, **kw)
        return e.value.code

    assert code(modgpu.digest_device, 0, 1, result=r, n=10) == 1                      # null source
    assert code(modgpu.digest_device, 0, 1, dst=p, result=r, n=10) == 1
    assert code(modgpu.digest_device, p, 1, result=0, n=10) == 1                      # null record
    assert code(modgpu.digest_device, p, 1, result=r + 4, n=10) == 1                  # misaligned record
    assert code(modgpu.digest_device, p, 1, result=r + 1, n=0) == 1                   # ... whatever n is
    for d, s in ((p + 1, p), (p, p + 1), (p + 9, p), (p, p + 9)):                     # partial overlaps, down to one byte
        assert code(modgpu.digest_device, s, 1, dst=d, result=r, n=10) == 1
    assert code(modgpu.digest_batch_device, [p + 100, p + 25], [10, 10], 1, r, dst_ptrs=[p, p + 20]) == 1   # entry 1 partly overlaps its own source
    assert code(modgpu.digest_batch_device, [p + 100, p + 120], [10, 10], 1, r, dst_ptrs=[p, p + 5]) == 1   # two destinations meet
    assert code(modgpu.digest_batch_device, [p + 20, p + 40], [10, 10], 1, r, dst_ptrs=[p, p + 20]) == 1    # dst 1 is src 0
    assert code(modgpu.digest_batch_device, [p + 20, p + 40], [10, 10], 1, r, dst_ptrs=[None, p + 25]) == 1  # ... of a digest-only entry
    assert code(modgpu.digest_batch_device, [p, 0], [10, 10], 1, r) == 1
    assert code(modgpu.digest_batch_device, [p, p + 20], [10, 10], 1, 0) == 1
    assert code(modgpu.digest_results, 0, 1) == 1 and code(modgpu.digest_results, r + 4, 1) == 1
    # valid: digest only, fused, exact alias, n == 0, null with n == 0, overlapping sources without a destination, empty entries,
    # identity keys
    assert code(modgpu.digest_device, p, 1, result=r, n=10) == 2
    assert code(modgpu.digest_device, p, 1, dst=p + 100, result=r, n=10) == 2
    assert code(modgpu.digest_device, p, 1, dst=p, result=r, n=10) == 2
    assert code(modgpu.digest_device, p, 1, result=r, n=0) == 2
    assert code(modgpu.digest_device, 0, 1, result=r, n=0) == 2
    assert code(modgpu.digest_device, p, 0x7FFFFFFF, dst=p + 100, result=r, n=10) == 2
    assert code(modgpu.digest_batch_device, [p, p + 5, p + 5], [10, 10, 0], 1, r, stream_offs=[0, 5, 7]) == 2
    assert code(modgpu.digest_batch_device, [p, p + 5, 0], [10, 10, 0], 1, r, dst_ptrs=[p + 100, None, None]) == 2
    assert code(modgpu.time_digest_device, p, 10, 1, r) == 2
    assert code(modgpu.digest_results, r, 1) == 2
    assert np.array_equal(b, keep) and (res == 0xEE).all()
    st = modgpu.path_stats()
    assert st["gpu_launches"] == before["gpu_launches"] == 0 and st["scalar_calls"] == before["scalar_calls"]


def test_codegen_guard_with_the_digest_loop():
    """`make isa-check-to` passes the tree (still 2 kernels, inside the register budget, nothing spilled); the same TU with a store
    through the source descriptor put into the digest loop is rejected by name."""
    B.isa_check_target("isa-check-to", 2)
    broken = subprocess.run(["make", "-s", "-C", CSRC, "isa-check-broken-to-digest"], capture_output=True, text=True, timeout=900)
    assert broken.returncode != 0, "the guard accepted a digest loop that stores through its source's descriptor"
    assert "nothing through its source's" in broken.stdout and "20 buffer stores, expected 18" in broken.stdout, broken.stdout[-3000:]


def test_codegen_guard_rules_of_the_digest_loop_on_altered_assembly():
    """The digest loop's rules of check_isa.check() on the tree's own assembly with one fault put in by hand each."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "cycle_to_kernel.s"])
    ci = B.load_check_isa()
    asm = open(os.path.join(CSRC, "cycle_to_kernel.s")).read()
    assert ci.check(asm) == []
    bodies = ci.kernel_bodies(asm)
    assert len(bodies) == 2
    for fn in bodies.values():  # both loops are inside what the rules read, and inside the budget
        assert fn.count("v_dot4_u32_u8") >= 8 and fn.count("global_atomic_add_x2") >= 3 and len(ci.code_lines(fn, "buffer_store_dwordx4")) == 18
    for name in bodies:
        md = ci.metadata(asm, name)
        assert md["vgpr_count"] <= 128 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    first = next(iter(bodies))
    at = asm.index(first + ":")
    end = asm.index(".Lfunc_end", at)

    def in_first(old, new, count=1):
        head, body, tail = asm[:at], asm[at:end], asm[end:]
        assert old in body
        return head + body.replace(old, new, count) + tail

    one_store = next(ln for ln in asm[at:end].splitlines() if ln.startswith("\tbuffer_store_dwordx4 "))
    cases = {
        "64-bit atomics ['global_atomic_add_x2', 'global_atomic_umin_x2']": in_first("\tglobal_atomic_add_x2 ", "\tglobal_atomic_umin_x2 "),
        "expected non-returning global_atomic_add_x2 only": in_first("\tglobal_atomic_add_x2 ", "\tglobal_atomic_umin_x2 ", -1),
        "no v_dot4_u32_u8": in_first("\tv_dot4_u32_u8 ", "\tv_dot4_removed ", -1),
        "19 buffer stores, expected 18": in_first(one_store + "\n", one_store + "\n" + one_store + "\n"),
        "17 buffer stores, expected 18": in_first(one_store + "\n", ""),
    }
    for want, text in cases.items():
        got = ci.check(text)
        assert any(want in f for f in got), (want, got[:5])
    returning = in_first("\tglobal_atomic_add_x2 ", "\tglobal_atomic_add_x2 v[90:91], ")
    i = returning.index("\tglobal_atomic_add_x2 v[90:91], ", at)
    j = returning.index("\n", i)
    got = ci.check(returning[:j] + " sc0" + returning[j:])
    assert any("expected non-returning global_atomic_add_x2 only" in f for f in got), got[:5]


def test_digest_calls_on_the_standin_under_asan_ubsan():
    """tests/digest_main.cpp: every edge size at source phases 0, 1, 15 and 65520 + 15, digest only and fused, identity keys, batches
    of 1, 16 and 17 with empty entries, every host refusal with its text, every byte of the arena and every record against a model
    written from lcg.h and the closed form."""
    if not B.sanitizer_runtime("libasan.a") or not B.sanitizer_runtime("libubsan.a"):
        pytest.skip("gcc sanitizer runtimes not installed")
    subprocess.check_call(["make", "-s", "-C", CSRC, "digest-main"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", MODGPU_REQUIRE_GPU="0")
    for k in ("MODGPU_SHIM_DEVICES", "MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "modulate_amd", "_san", "digest_main")], env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not r.stderr.strip(), "\n".join(ln for ln in lines if not ln.startswith("ok  "))[-3000:] + r.stderr[-3000:]
    assert lines[-1].endswith(", 0 failed") and int(lines[-1].split()[0]) == len(lines) - 1 == 195, lines[-1]
    for what in ("closed form n=100003", "digest-only entries=1 n0=196613 src0=131071", "fused       entries=1 n0=65537", "fused alias entries=1 n0=17",
                 "identity    entries=1 n0=65535", "identity fu entries=1 n0=1 ", "batch       entries=3", "batch       entries=18", "batch       entries=19",
                 "batch empty entries=2", "timed digest", "refusal: null source", "refusal: null result", "refusal: misaligned result",
                 "refusal: result in host memory", "refusal: partial overlap by one byte", "refusal: 2^24 chunks by the source's phase",
                 "refusal: two destinations meet", "refusal: a destination meets a digest-only entry's source", "refusal: results: host memory",
                 "refusal: timed: partial overlap", "refusals queued nothing"):
        assert any(ln.startswith("ok   " + what) for ln in lines), what
    assert lines[-2].startswith("ok   launch plans: 0 plan errors")
    B.standin_is_wired("standin_launch_to_digest.cpp")
