"""CPU checks of the workspace reuse harness (tests/workspace_reuse.py) before it meets a GPU: the case lists are whole and every table
in them passes the library's host validators; the comparer fails a model that is wrong in ONE thing -- one arena byte, one guard byte,
one record, one status, one summary field, the launch count, one byte of W past workspace_bytes --; the gate of the 0xFF and random
fills holds; and the same adapters, models and case lists run, every case of them, on the CPU stand-in of the HIP runtime -- a build
of the library's host code and the stand-in kernels with no sanitizer in it (`make standin-lib`), loaded by a child process."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import workspace_reuse as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")


@pytest.fixture(scope="module")
def K(oracle):
    return R.Keystreams(oracle)


def test_the_case_lists_are_whole():
    assert len(R.KINDS) == 10 and len(R.FILLS) == 4 and R.NS == (1, 16, 17, 256, 257, 1025, 4097)
    assert sorted(R.FILL_CASES) == sorted((f, k) for f in R.FILLS for k in R.KINDS)
    assert [f for f, _ in R.FILL_CASES] == sorted((f for f, _ in R.FILL_CASES), key=R.FILLS.index), "0x00 first, then the leftover, 0xFF, random"
    assert len(R.PAIR_CASES) == 200 and {(a, b) for _, _, a, b in R.PAIR_CASES} == {(4097, 17), (17, 4097)}
    assert sorted(R.ALIGN_CASES) == sorted(R.KINDS)
    assert all(R.other(k) != k for k in R.KINDS) and {R.SPEC[k]["family"] for k in R.REFUSAL_PREVIOUS} == {"cycle", "move"}
    assert R.SPEC["cycle_digest_table"]["sides"] == (R.OUTPUT, R.INPUT) and R.SPEC["rekey_digest_table"]["sides"] == (R.PLAIN, R.OUTPUT, R.INPUT)
    # the layouts: every edge size, sources and destinations at phases 0, 1 and 7, both ways and stationary in the moving kinds
    for n in (16, 4097):
        assert set(R.EDGE_SIZES) <= set(R.sizes(n))
        segs = R.segs_of(R.Case("rekey_table", n))
        assert {(d % 16, s % 16) for d, s, _, _ in segs} == {(a, b) for a in R.PHASES for b in R.PHASES}
        for kind, ways in (("rekey_move_table", {-1, 0} if n % 2 == 0 else {0, 1}), ("rekey_relayout_table", {-1, 0, 1})):
            segs = R.segs_of(R.Case(kind, n))
            assert {int(np.sign(d - s)) for d, s, k, _ in segs if k} == ways, kind
            # a destination lies over ANOTHER entry's source: a stale "loaded" flag would release a store early
            assert any(d < s2 + k2 and s2 < d + k for i, (d, _, k, _) in enumerate(segs[:64]) for j, (_, s2, k2, _) in enumerate(segs[:64]) if i != j and k and k2), kind
    d, s, k, _ = R.segs_of(R.Case("rekey_move", 4097))[0]
    assert abs(d - s) < k, "the single move's ranges overlap"


def test_every_table_passes_the_host_validators(modgpu):
    base = 1 << 32
    for kind, validate in (("cycle_table", modgpu.table_validate), ("cycle_digest_table", modgpu.table_validate), ("rekey_table", modgpu.rekey_table_validate),
                           ("rekey_digest_table", modgpu.rekey_table_validate), ("rekey_move_table", modgpu.rekey_move_table_validate),
                           ("rekey_relayout_table", modgpu.rekey_relayout_table_validate)):
        for n in R.NS + (R.ALIGN_N,):
            for variant in (0, 1):
                validate(R.entries(modgpu, R.Case(kind, n, variant=variant), base))
        with pytest.raises(modgpu.ModGpuError, match=f"entry {R.BAD}:"):
            validate(R.entries(modgpu, R.Case(kind, R.REFUSED_N, bad=R.BAD), base))
    # what each kind is given is what its own size function returns, and the shared buffer has room for the largest
    sizes = {c.key: R.need(modgpu, c) for c in R.all_cases()}
    assert all(v > 0 and v % 64 == 0 for v in sizes.values())
    assert max(sizes, key=sizes.get)[:2] == ("rekey_relayout_table", 4097) or max(sizes, key=sizes.get)[:2] == ("rekey_move_table", 4097)


def _outputs(K, case, room=4096):
    """what a faultless adapter would return for the case, and what Rig.run would expect"""
    want = dict(R.model(case, K), w_outside=np.full(room, 0xA5, np.uint8))
    got = {k: copy.deepcopy(v) for k, v in want.items()}
    for v in got.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=True)
    return got, want


def _flip(name, at):
    def change(got):
        a = got[name].reshape(-1)
        a[at] ^= 1
    return change


def _set(name, value):
    def change(got):
        got[name] = value
    return change


def _summary(field, value):
    def change(got):
        got["summary"] = dict(got["summary"], **{field: value})
    return change


WRONG = [  # (case, the ONE thing that is wrong, the output the comparer must name)
    (("cycle_table", 17), _flip("arena", R.G + 5), "arena"),
    (("cycle_table", 17), _flip("arena", 3), "arena"),                      # a byte of the window's guard
    (("cycle_table", 17), _flip("arena", -1), "arena"),
    (("cycle_table", 17), _set("table_status", 0), "table_status"),
    (("cycle_table", 17), _set("launches", 4), "launches"),
    (("cycle_table", 17), _flip("w_outside", 0), "w_outside"),              # one byte of W in front of the workspace
    (("cycle_table", 17), _flip("w_outside", -1), "w_outside"),             # ... and one past workspace_bytes
    (("verify_table", 17), _flip("records", 0), "records"),                 # a mismatch count
    (("verify_table", 17), _flip("records", 1), "records"),                 # a first_mismatch
    (("verify_table", 17), _flip("records", 3 * 16 + 2), "records"),        # the last entry's n
    (("verify_table", 17), _flip("record_guards", R.G), "record_guards"),   # the byte behind the last record
    (("verify_table", 17), _summary("mismatches", 0), "summary"),
    (("verify_table", 17), _summary("first_bad_entry", 5), "summary"),
    (("verify_table", 17), _summary("entries", 4097), "summary"),
    (("verify_rekey_table", 17), _flip("arena", R.G + 70000), "arena"),     # a verifying call that wrote
    (("cycle_digest_table", 17), _flip("records", 0), "records"),           # an Adler-32
    (("cycle_digest_table", 17), _flip("records", 2 * 9 + 1), "records"),   # a record's n
    (("rekey_digest_table", 17), _flip("arena", R.G + 100), "arena"),
    (("rekey_relayout_table", 17), _set("move_table_status", (None, 3)), "move_table_status"),
    (("rekey_relayout_table", 17), _set("table_status", 2), "table_status"),
    (("rekey_relayout_table", 17), _set("launches", 5), "launches"),
    (("rekey_move_table", 17), _flip("arena", R.G + 131073), "arena"),
    (("rekey_move", 17), _set("move_status", 0), "move_status"),
    (("rekey_move", 17), _flip("arena", R.G + 4000), "arena"),
    (("rekey_digest_table", R.REFUSED_N, None, R.BAD), _flip("records_raw", 32 * 7), "records_raw"),  # a refused call that stored a record
    (("rekey_digest_table", R.REFUSED_N, None, R.BAD), _flip("arena", R.G + 9), "arena"),
    (("rekey_digest_table", R.REFUSED_N, None, R.BAD), _set("table_status", None), "table_status"),
    (("rekey_digest_table", R.REFUSED_N, None, R.BAD), _set("table_status", R.BAD + 1), "table_status"),
    (("verify_table", R.REFUSED_N, None, R.BAD), _set("summary", {"mismatches": 0, "first_bad_entry": None, "entries": R.REFUSED_N}), "summary"),
    (("rekey_move_table", R.REFUSED_N, None, R.BAD), _set("move_table_status", (None, None)), "move_table_status"),
]


@pytest.mark.parametrize("key,change,named", WRONG, ids=[f"{k[0]}-{k[1]}-{named}-{i}" for i, (k, _, named) in enumerate(WRONG)])
def test_the_comparer_fails_a_model_wrong_in_one_thing(K, key, change, named):
    case = R.Case(*key)
    got, want = _outputs(K, case)
    R.compare(got, want, case)  # faultless outputs pass
    change(got)
    with pytest.raises(AssertionError) as e:
        R.compare(got, want, case)
    assert e.value.args[0][1] == named, e.value.args
    # ... and an adapter that leaves an output out does not pass either
    got, want = _outputs(K, case)
    del got[named]
    with pytest.raises(AssertionError, match="did not return"):
        R.compare(got, want, case)


def test_the_models_are_the_oracles(K, oracle):
    """the model against the oracle applied entry by entry, and the records against zlib on those bytes: one case, by hand"""
    import zlib
    case = R.Case("cycle_digest_table", 17, R.OUTPUT)
    lo, img = R.window(case, K)
    want = R.model(case, K)
    for i, (d, s, n, (_, key, _, of, _)) in enumerate(R.segs_of(case)):
        seg = img[R.G + s - lo:R.G + s - lo + n].copy()
        oracle.cycle_at(seg, key, R.BASE + of + s)
        assert np.array_equal(want["arena"][R.G + d - lo:R.G + d - lo + n], seg), i
        assert tuple(want["records"][i]) == (zlib.adler32(seg.tobytes()), n), i
    assert (want["arena"][:R.G] == 0xA5).all() and (want["arena"][-R.G:] == 0xA5).all()
    # a verifying case counts exactly the planted bytes, the first of each entry where it was planted
    case = R.Case("verify_rekey_table", 257)
    want, plants = R.model(case, K), R.planted(case)
    assert want["summary"] == {"mismatches": len(plants), "first_bad_entry": plants[0][0], "entries": 257} and len(plants) > 50
    for i in {i for i, _ in plants}:
        assert tuple(want["records"][i][:2]) == (sum(1 for e, _ in plants if e == i), min(j for e, j in plants if e == i)), i
    assert R.model(R.Case("verify_rekey_table", 257, bad=R.BAD), K)["summary"] == "refused"


def test_the_gate_of_the_0xff_and_random_fills():
    saved = set(R.PASSED)
    try:
        R.PASSED.clear()
        assert R.fill_blocked("zero", "cycle_table") is None and R.fill_blocked("leftover", "cycle_table") is None
        assert "did not pass the zero and the leftover fill" in R.fill_blocked("ones", "cycle_table")
        R.PASSED.add(("zero", "cycle_table"))
        assert "did not pass the leftover fill" in R.fill_blocked("random", "cycle_table")
        with pytest.raises(AssertionError, match="is not run on a workspace of ones bytes"):
            R.run_fill(None, "ones", "cycle_table")
        R.PASSED.add(("leftover", "cycle_table"))
        assert R.fill_blocked("ones", "cycle_table") is None and R.fill_blocked("random", "cycle_table") is None
        assert R.fill_blocked("ones", "rekey_table")
    finally:
        R.PASSED.clear()
        R.PASSED.update(saved)


def test_every_case_on_the_standin(oracle):
    """tests/_workspace_reuse_child.py: all forty fills, all two hundred ordered pairs, the refusals across kinds, the readers and the
    odd alignment, through the adapters and models the GPU module uses, on the stand-in kernels -- a second implementation of every
    call, so a case that passes here has its layout, its model and its adapter right"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "standin-lib"])
    env = dict(os.environ, MODGPU_LIB=os.path.join(ROOT, "modulate_amd", "_san", "libmodgpu_standin.so"), MODGPU_REQUIRE_GPU="0", MODGPU_SHIM_DEVICES="1")
    for k in ("MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_workspace_reuse_child.py")], env=env, capture_output=True, text=True, cwd=ROOT, timeout=900)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "workspace reuse on the stand-in: ok", r.stdout[-2000:] + r.stderr[-4000:]
    assert lines[0].startswith("fills: 40 ") and lines[1].startswith("pairs: 200 "), lines
