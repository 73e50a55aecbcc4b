"""CPU-only checks of the C++ host mirror (libmodulate_host.so): it loads, the CArk header writer
and part-split bookkeeping agree with the independent Python restatement (oracle/ark_header.py;
both are held to the compiled reference itself in tests/test_ref_host_parity.py), CEncryptionCycler::Cycle keeps
the reference's "cannot fail" contract on a GPU-less host (BASELINE config 1) unless
MODGPU_REQUIRE_GPU forbids it, and the reference's deterministic quirks are the default with their
fixes behind one switch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ark_header as AH


@pytest.fixture(scope="module")
def host():
    from modulate_amd import host as H
    H.lib()
    H.set_flags(overwrite=True, ignore_new=True, pack_all=False, verbose=False)
    H.set_fix_quirks(False)
    return H


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "modulate_amd", "bin", "modulate")
needs_host_loop = pytest.mark.skipif(os.environ.get("MODGPU_REQUIRE_GPU", "0") not in ("", "0"),
                                     reason="MODGPU_REQUIRE_GPU forbids the host loop in this process")


def synth_table(n, seed=1):
    rng = np.random.default_rng(seed)
    names = [f"dir{k % 97}/sub{k % 13}/f{k}.bin" for k in range(n)]  # SURVEY 8d config-4 naming
    names[: min(n, 3)] = ["readme.txt", "Dir5/UPPER.bin", "dir5/lower.bin"][: min(n, 3)]
    sizes = [int(x) for x in rng.integers(0, 3000, size=n)]
    if n > 10:
        sizes[4] = sizes[9] = 0  # empty files keep offset 0 (CArk.cpp:787-791)
    return names, sizes


def test_hooks_exported(host):
    L = host.lib()
    for name in host.HOOKS:
        assert getattr(L, name) is not None


@pytest.mark.parametrize("ps4", [True, False])
@pytest.mark.parametrize("n,n_arks", [(1, 1), (2, 1), (57, 3), (1000, 4), (5000, 8)])
def test_header_writer_matches_restatement(host, ps4, n, n_arks):
    host.select_platform(ps4)
    names, sizes = synth_table(n, seed=n)
    a = host.Ark()
    a.construct_from_table(names, sizes, n_arks, "main_ps4" if ps4 else "main_ps3")
    data = np.random.default_rng(n).integers(0, 256, size=sum(sizes), dtype=np.uint8)
    a.build_from_memory(data)
    offs, parts = AH.split_into_arks(sizes, AH.even_plan(sum(sizes), n_arks))
    assert a.ark_sizes() == parts and sum(parts) == sum(sizes)
    assert [f["offset"] for f in a.files()] == offs
    assert np.array_equal(a.data(), data)
    img = a.serialise_header(encrypt=False).tobytes()
    assert img == AH.serialise(names, sizes, offs, parts, a.ark_paths(), ps4)
    p = AH.parse(img)
    assert p["end"] == len(img) and p["magic"] == AH.MAGIC[ps4] and p["version"] == 9
    assert p["ark_sizes"] == parts and [f["name"] for f in p["files"]] != []
    # the header's own lookup structure finds every name, and only those
    for nm in names:
        i = AH.lookup(p, nm)
        assert i >= 0 and p["files"][i]["name"] == nm
    assert AH.lookup(p, "no/such/file") == -1
    by_name = {f["name"]: f for f in p["files"]}
    for nm, s, o in zip(names, sizes, offs):
        assert by_name[nm]["size"] == s and by_name[nm]["offset"] == o
        assert by_name[nm]["hash"] == (AH.HASH_FIELD[ps4] if s else 0)
    a.close()


def test_files_never_straddle_parts(host):
    host.select_platform(True)
    names, sizes = synth_table(3000, seed=5)
    a = host.Ark()
    a.construct_from_table(names, sizes, 6, "p")
    a.build_from_memory(np.zeros(sum(sizes), np.uint8))
    bounds = np.cumsum([0] + a.ark_sizes())
    for f in a.files():
        if f["size"]:
            k = np.searchsorted(bounds, f["offset"], side="right") - 1
            assert f["offset"] + f["size"] <= bounds[k + 1]
    a.close()


def test_bad_arguments(host):
    a = host.Ark()
    with pytest.raises(host.HostError) as e:
        a.construct_from_table(["a", "b"], [1], 1)
    assert e.value.code == 11  # eError_InvalidParameter
    a.construct_from_table(["a", "b"], [1, 2], 1)
    with pytest.raises(host.HostError) as e:
        a.build_from_memory(np.zeros(2, np.uint8))  # 3 bytes expected
    assert e.value.code == 11
    with pytest.raises(host.HostError) as e:
        host.Ark().load("/nonexistent/main_ps4.hdr")
    assert e.value.code == 1  # eError_FailedToOpenFile
    with pytest.raises(host.HostError) as e:
        host.Ark().parse_header(np.zeros(64, np.uint8))
    assert e.value.code == 3  # eError_UnknownVersionNumber: magic is checked before any cipher work
    a.close()


@needs_host_loop
def test_config1_cycle_cannot_fail_without_gpu(host, modgpu, oracle, tmp_path):
    """BASELINE config 1 as worded ("single 4 KiB .dta decrypt on reference CPU path, no GPU"): the
    reference's Cycle returns void and cannot fail (CEncryptionCycler.cpp:4-14), so on a GPU-less host
    the class, the three framed call sites and `modulate -decode` all work, bit-exact."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    from oracle import dta_tree as DT
    before = modgpu.path_stats()
    for key in (0x90CFC0AB, 0xC64EED30, 1, 0xFFFFFFFF, 0x80000000, 0, 0x7FFFFFFF):
        for n in (0, 1, 15, 4092, 100_001):
            whole = oracle.splitmix_bytes(n + 4, n + 1)
            got = whole.copy()
            host.cycle_via_class(got[4:], key)  # CEncryptionCycler().Cycle(buf+4, size-4, key)
            want = whole.copy()
            oracle.cycle(want[4:], key)
            assert np.array_equal(got, want), (hex(key), n)
    after = modgpu.path_stats()
    if not os.environ.get("MODULATE_HOST_LIB"):  # (the sanitizer build binds to a stub, not to the library that counts)
        # n = 100 001 is header-sized (< MODGPU_MIN_GPU_BYTES): every one of these calls is the size dispatch's, none a GPU attempt
        assert after["auto_small"] > before["auto_small"] and after["gpu_launches"] == 0
    # a 4 KiB DTA blob framed like a header, on disk as main_ps4.hdr: -decode writes magic + plaintext
    tree = DT.synth_tree(np.random.default_rng(4096), target_bytes=4092)
    body = np.frombuffer(DT.serialise(tree), dtype=np.uint8)
    for ps4, plat in ((True, "ps4"), (False, "ps3")):
        framed = np.concatenate([np.zeros(4, np.uint8), body])
        assert oracle.hdr_encrypt(framed, ps4) == 0
        d = tmp_path / plat
        d.mkdir()
        framed.tofile(d / f"main_{plat}.hdr")
        r = subprocess.run([EXE] + ([] if ps4 else ["-ps3"]) + ["-decode", str(d)], capture_output=True, text=True)
        assert r.returncode == 0 and "Complete!" in r.stdout, r.stdout + r.stderr
        dec = np.fromfile(d / f"main_{plat}.hdr.dec", dtype=np.uint8)
        assert np.array_equal(dec[4:], body) and np.array_equal(dec[:4], framed[:4])
        out, dump = host.dta_roundtrip(dec[4:].tobytes())
        assert out == body.tobytes() and dump == DT.dump(tree)


@needs_host_loop
def test_part_cipher_on_a_host_without_gpu(host, modgpu, oracle, header_cwd, tmp_path):
    """BASELINE config 5 says "byte-diff vs the build's CPU path": the part cipher (north_star: Cycle over part-sized
    buffers beside LoadArkData / lSaveArk, CArk.cpp:723-758, 845-899) is defined on a GPU-less host too -- the parts go
    through the library's own host loop, as Cycle itself does there.  Encrypted parts == oracle Cycle of the raw slices,
    `-cryptparts -unpack` restores every file, `-cryptparts -pack` writes parts that oracle-decrypt to the files at their
    offsets, and MODGPU_REQUIRE_GPU=1 refuses instead of computing."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    host.select_platform(True)
    rng = np.random.default_rng(55)
    n = 300
    names = [f"dir{k % 7}/sub{k % 3}/f{k}.bin" for k in range(n)]
    sizes = [int(x) for x in rng.integers(0, 300_000, size=n)]
    data = rng.integers(0, 256, size=sum(sizes), dtype=np.uint8)
    offs = np.cumsum([0] + sizes)
    first = str(tmp_path / "first") + "/"
    os.makedirs(first)
    a = host.Ark()
    a.construct_from_table(names, sizes, 3, "main_ps4")
    a.build_from_memory(data)
    a.enable_part_cipher(True, 8)
    a.save(first, "main_ps4.hdr")
    assert np.array_equal(a.data(), data)  # SaveArk leaves the in-memory slices as they were
    off = 0
    for path, size in zip(a.ark_paths(), a.ark_sizes()):
        assert np.array_equal(np.fromfile(first + path, dtype=np.uint8), oracle.cycle(data[off:off + size].copy(), oracle.KEY_PS4)), path
        off += size
    b = host.Ark().load(first + "main_ps4.hdr")
    b.enable_part_cipher(True, 8)
    b.load_data()
    assert np.array_equal(b.data(), data)
    b.cycle_parts(oracle.KEY_PS4, 8)  # the in-memory form (CycleArkData): every part its own stream from offset 0
    off = 0
    for size in b.ark_sizes():
        assert np.array_equal(b.data()[off:off + size], oracle.cycle(data[off:off + size].copy(), oracle.KEY_PS4))
        off += size
    a.close(), b.close()
    unpacked, packed = str(tmp_path / "u"), str(tmp_path / "p")
    os.makedirs(packed)
    env = {k: v for k, v in os.environ.items() if k != "MODGPU_REQUIRE_GPU"}
    r = subprocess.run([EXE, "-cryptparts", "-gpus", "8", "-unpack", first, unpacked], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "Complete!" in r.stdout, r.stdout[-2000:] + r.stderr
    for nm, s_, o in zip(names, sizes, offs):
        assert np.array_equal(np.fromfile(os.path.join(unpacked, nm), dtype=np.uint8), data[o:o + s_]), nm
    r = subprocess.run([EXE, "-cryptparts", "-gpus", "8", "-pack", first, unpacked, packed], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "Complete!" in r.stdout, r.stdout[-2000:] + r.stderr
    c = host.Ark().load(packed + "/main_ps4.hdr")
    raw = np.concatenate([oracle.cycle(np.fromfile(os.path.join(packed, p), dtype=np.uint8), oracle.KEY_PS4) for p in c.ark_paths()])
    by_name = dict(zip(names, zip(offs, sizes)))
    assert sorted(f["name"] for f in c.files()) == sorted(names)
    for f in c.files():
        o, s_ = by_name[f["name"]]
        assert f["size"] == s_ and np.array_equal(raw[f["offset"]:f["offset"] + s_], data[o:o + s_]), f["name"]
    c.close()
    strict = subprocess.run([EXE, "-cryptparts", "-unpack", first, str(tmp_path / "never")], capture_output=True, text=True,
                            env=dict(env, MODGPU_REQUIRE_GPU="1"))
    assert strict.returncode != 0 and "no HIP device visible" in strict.stdout, strict.stdout[-1000:]


@needs_host_loop
def test_header_save_load_framing_without_gpu(host, modgpu, oracle, header_cwd, tmp_path):
    """SaveArk / Load framing (CArk.cpp:914-915, 1135-1136, 328-339) on a GPU-less host: header on disk ==
    oracle ciphertext of the plain image; Load decrypts it back; parts are raw slices."""
    if modgpu.device_count() > 0:
        pytest.skip("GPU present")
    for ps4 in (True, False):
        host.select_platform(ps4)
        plat = "ps4" if ps4 else "ps3"
        names, sizes = synth_table(300, seed=8)
        data = np.random.default_rng(8).integers(0, 256, size=sum(sizes), dtype=np.uint8)
        a = host.Ark()
        a.construct_from_table(names, sizes, 3, f"main_{plat}")
        a.build_from_memory(data)
        assert not a.data_pinned
        out = str(tmp_path / plat) + "/"
        os.makedirs(out)
        a.save(out, f"main_{plat}.hdr")
        plain = a.serialise_header(encrypt=False)
        want = plain.copy()
        assert oracle.hdr_encrypt(want, ps4) == 0
        assert np.array_equal(np.fromfile(out + f"main_{plat}.hdr", dtype=np.uint8), want)
        b = host.Ark().load(out + f"main_{plat}.hdr")
        assert b.ark_sizes() == a.ark_sizes() and [f["name"] for f in b.files()] == [f["name"] for f in AH.parse(plain.tobytes())["files"]]
        b.load_data()
        assert np.array_equal(b.data(), data)
        a.close(), b.close()
    host.select_platform(True)


def test_require_gpu_makes_cycle_throw_without_gpu(host):
    """The opt-in strict mode: MODGPU_REQUIRE_GPU=1 and no GPU -> Cycle throws, buffer untouched."""
    code = ("import numpy as np\n"
            "from modulate_amd import host as H\n"
            "b = np.arange(100, dtype=np.uint8); k = b.copy()\n"
            "try:\n"
            "    H.cycle_via_class(b, 0x90CFC0AB); raise SystemExit('computed')\n"
            "except H.HostError as e:\n"
            "    assert e.code == -1 and 'GPU path failed' in str(e), str(e)\n"
            "assert (b == k).all()\n"
            "print('THROWS_OK')\n")
    env = dict(os.environ, MODGPU_REQUIRE_GPU="1", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and "THROWS_OK" in r.stdout, r.stdout + r.stderr


# ---- the reference's deterministic quirks are the default; -fixquirks / mbFixReferenceQuirks corrects them
def _small_ark(host, n_arks=3, n=60, seed=21):
    names, sizes = synth_table(n, seed=seed)
    data = np.random.default_rng(seed).integers(0, 256, size=sum(sizes), dtype=np.uint8)
    a = host.Ark()
    a.construct_from_table(names, sizes, n_arks, "main_ps4")
    a.build_from_memory(data)
    return a, names, sizes, data


@needs_host_loop
def test_quirk_savearc_needs_header_in_cwd(host, tmp_path, monkeypatch):
    """CArk.cpp:904-909: SaveArk opens lpHeaderFilename (bare name, working directory) before anything else."""
    host.select_platform(True)
    a, *_ = _small_ark(host)
    empty = tmp_path / "empty"
    empty.mkdir()
    monkeypatch.chdir(empty)
    out = str(tmp_path / "out") + "/"
    os.makedirs(out)
    with pytest.raises(host.HostError) as e:
        a.save(out, "main_ps4.hdr")
    assert e.value.code == 1 and not os.path.exists(out + "main_ps4.hdr")  # eError_FailedToOpenFile, nothing written
    host.set_fix_quirks(True)
    try:
        a.save(out, "main_ps4.hdr")
        assert os.path.getsize(out + "main_ps4.hdr") > 0
    finally:
        host.set_fix_quirks(False)
    (empty / "main_ps4.hdr").write_bytes(b"x")
    a.save(out, "main_ps4.hdr")  # reference mode, header present: fine
    a.close()


@needs_host_loop
def test_pack_does_not_change_the_working_directory(host, header_cwd, tmp_path):
    """-pack used to chdir() the whole process into the header directory so that SaveArk's bare-name open
    (CArk.cpp:904-909) worked.  Now the header directory is the CArk object's working directory: the CLI, started
    somewhere else with relative paths, resolves them against ITS directory, finds the header in the directory it was
    given, and the round trip reaches its fixed point."""
    import subprocess
    if os.environ.get("MODULATE_HOST_LIB"):
        pytest.skip("CLI binary binds to the product library")
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "modulate_amd", "bin", "modulate")
    host.select_platform(True)
    a, names, sizes, data = _small_ark(host)
    work = tmp_path / "elsewhere"
    (work / "first").mkdir(parents=True)
    a.save(str(work / "first") + "/", "main_ps4.hdr")
    a.close()
    for cmd in (["-unpack", "first", "unpacked"], ["-pack", "first", "unpacked", "second"], ["-unpack", "second", "again"], ["-pack", "second", "again", "third"]):
        if cmd[0] == "-pack":
            (work / cmd[-1]).mkdir()
        r = subprocess.run([exe] + cmd, capture_output=True, text=True, cwd=work)  # no main_ps4.hdr in `work` itself
        assert r.returncode == 0 and "ERROR" not in r.stdout, (cmd, r.stdout + r.stderr)
    assert not (work / "main_ps4.hdr").exists()
    produced = sorted(f.name for f in (work / "second").iterdir())
    assert "main_ps4.hdr" in produced and len(produced) >= 2
    for fn in produced:
        assert (work / "second" / fn).read_bytes() == (work / "third" / fn).read_bytes(), fn
    offs = np.cumsum([0] + sizes)
    for nm, sz, o in zip(names, sizes, offs):
        assert np.array_equal(np.fromfile(work / "again" / nm, dtype=np.uint8), data[o:o + sz]), nm


@needs_host_loop
def test_quirk_skipped_part_keeps_slice_pointer(host, header_cwd, tmp_path):
    """CArk.cpp:853-869, 883-891: with overwriting off, an existing non-empty part is skipped and lpArkPtr is
    NOT advanced, so every later part is written from the slice of the part before it."""
    host.select_platform(True)
    a, names, sizes, data = _small_ark(host, n_arks=4)
    parts, paths = a.ark_sizes(), a.ark_paths()
    bounds = np.cumsum([0] + parts)
    for fix in (False, True):
        out = str(tmp_path / f"fix{int(fix)}") + "/"
        os.makedirs(out)
        with open(out + paths[1], "wb") as f:
            f.write(b"keep me")
        host.set_flags(overwrite=False, ignore_new=True, pack_all=False, verbose=False)
        host.set_fix_quirks(fix)
        try:
            a.save(out, "main_ps4.hdr")
        finally:
            host.set_flags(overwrite=True, ignore_new=True, pack_all=False, verbose=False)
            host.set_fix_quirks(False)
        assert open(out + paths[1], "rb").read() == b"keep me"
        assert np.array_equal(np.fromfile(out + paths[0], dtype=np.uint8), data[bounds[0]:bounds[1]])
        for i in (2, 3):
            start = bounds[i] if fix else bounds[i] - parts[1]  # reference: one part's worth behind
            assert np.array_equal(np.fromfile(out + paths[i], dtype=np.uint8), data[start:start + parts[i]]), (fix, i)
    a.close()


@needs_host_loop
def test_quirk_extract_ignores_range(host, header_cwd, tmp_path):
    """CArk.cpp:435: ExtractFiles walks all miNumFiles entries whatever (first, count) it was given."""
    host.select_platform(True)
    a, names, sizes, data = _small_ark(host)
    out = str(tmp_path / "packed") + "/"
    os.makedirs(out)
    a.save(out, "main_ps4.hdr")
    for fix in (False, True):
        b = host.Ark().load(out + "main_ps4.hdr")
        target = str(tmp_path / f"x{int(fix)}") + "/"
        host.set_fix_quirks(fix)
        try:
            b.extract(target, first=5, count=7)
        finally:
            host.set_fix_quirks(False)
        written = sorted(os.path.relpath(os.path.join(r, f), target) for r, _, fs in os.walk(target) for f in fs)
        listed = [f["name"] for f in b.files()]
        assert written == (sorted(listed[5:12]) if fix else sorted(listed))
        b.close()
    a.close()


def test_quirk_dta_top_level_trees_back_to_back(host):
    """CDtaFile.cpp:371-374: Save writes the root's children back to back, no type/1 separator between
    them -- so several top-level trees do not survive the reference's own Load.  Default here too."""
    from oracle import dta_tree as DT
    multi = [("tree", 16, 1, [("int", 0, 5)]), ("tree", 17, 9, [("int", 0, 6)]), ("tree", 16, 3, [("str", 5, "x")])]
    blob = DT.serialise(multi)  # the loadable form: separators present
    out, _ = host.dta_roundtrip(blob)
    assert out == DT.serialise(multi, separators=False) and out != blob
    host.set_fix_quirks(True)
    try:
        out2, dump2 = host.dta_roundtrip(blob)
        assert out2 == blob and dump2 == DT.dump(multi)
    finally:
        host.set_fix_quirks(False)


def test_cli_usage_and_unknown_flag():
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "modulate_amd", "bin", "modulate")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "usage" in r.stdout
    r = subprocess.run([exe, "-bogus"], capture_output=True, text=True)
    assert r.returncode != 0 and "Unkown parameter" in r.stdout  # the reference's own spelling (Modulate.cpp:962)
    r = subprocess.run([exe, "-decode", "/nonexistent"], capture_output=True, text=True)
    assert r.returncode != 0 and "ERROR: Failed to open file" in r.stdout


# ---- binary DTA tree (parity: test_ref_host_parity.py) -------------------------------------
def test_dta_roundtrip_matches_restatement(host):
    from oracle import dta_tree as DT
    rng = np.random.default_rng(12)
    tree = DT.synth_tree(rng, target_bytes=4000)
    blob = DT.serialise(tree)
    assert DT.parse(blob) == tree
    out, dump = host.dta_roundtrip(blob)
    assert out == blob                      # C++ writer == Python writer on the C++ parse of the Python image
    assert dump == DT.dump(tree)            # node for node
    # several top-level trees round-trip only with the quirk fix on (see test_quirk_dta_top_level_trees_back_to_back)
    multi = [tree[0], ("tree", 17, 9, [("int", 0, 5)]), ("tree", 16, 3, [("str", 5, "x"), ("float", 1, 0x40490FDB)])]
    blob2 = DT.serialise(multi)
    host.set_fix_quirks(True)
    try:
        out2, dump2 = host.dta_roundtrip(blob2)
    finally:
        host.set_fix_quirks(False)
    assert out2 == blob2 and dump2 == DT.dump(multi)


def test_dta_rejects_bad_images(host):
    from oracle import dta_tree as DT
    tree = DT.synth_tree(np.random.default_rng(1), target_bytes=600)
    blob = DT.serialise(tree)
    for cut in (0, 4, 6, 9, 40, len(blob) - 1):
        with pytest.raises(host.HostError) as e:
            host.dta_roundtrip(blob[:cut])
        assert e.value.code == 6  # eError_InvalidData
    bad = bytearray(blob)
    bad[9:13] = (77).to_bytes(4, "little")  # unknown child type (CDtaFile.cpp:503-504)
    with pytest.raises(host.HostError):
        host.dta_roundtrip(bytes(bad))
    zero = bytearray(blob)
    zero[5:7] = (0).to_bytes(2, "little")  # a tree with no children is invalid (CDtaFile.cpp:398-401)
    with pytest.raises(host.HostError):
        host.dta_roundtrip(bytes(zero))


def test_integration_binding_compiles_against_the_class_header(tmp_path):
    """INTEGRATION.md's binding, literally: the class declaration upstream's callers compile against (this repo's drop-in
    modulate_amd/csrc/host/CEncryptionCycler.h: the reference's class and signature; an empty pch.h stands in for upstream's
    precompiled header) + the binding's body for Cycle + libmodgpu.so = a working class with the reference's signature."""
    (tmp_path / "pch.h").write_text("")
    exe = str(tmp_path / "upstream_binding")
    lib = os.path.join(ROOT, "modulate_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + str(tmp_path), "-I" + os.path.join(lib, "csrc", "host"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "upstream_binding.cpp"), "-o", exe,
                           "-L" + lib, "-lmodgpu", "-Wl,-rpath," + lib])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    strict = os.environ.get("MODGPU_REQUIRE_GPU", "0") not in ("", "0")
    assert (r.returncode == 0 and "UPSTREAM_BINDING_OK" in r.stdout) or strict, r.stdout + r.stderr


def test_parsers_survive_mutated_images(host):
    """Header and DTA images with random byte flips and truncations: the C++ readers either accept the image or return
    an error -- never read out of bounds (this test is part of the ASan + UBSan job, tests/test_sanitizers.py)."""
    from oracle import dta_tree as DT
    rng = np.random.default_rng(20261004)
    names = [f"dir{k % 5}/f{k}.bin" for k in range(40)]
    sizes = [int(x) for x in rng.integers(0, 3000, size=40)]
    a = host.Ark()
    a.construct_from_table(names, sizes, 3, "main_ps4")
    a.build_from_memory(np.zeros(sum(sizes), np.uint8))
    plain = a.serialise_header(encrypt=False).copy()
    a.close()
    dta = bytearray(DT.serialise(DT.synth_tree(rng, 1500) + [("tree", 17, 9, [("int", 0, 5), ("str", 5, "abc")])]))
    verdicts = {"hdr_ok": 0, "hdr_rejected": 0, "dta_ok": 0, "dta_rejected": 0}
    try:
        for it in range(1500):
            m = plain.copy()
            for _ in range(int(rng.integers(1, 6))):
                m[int(rng.integers(4, m.size))] = rng.integers(0, 256)
            if rng.random() < 0.2:
                m = m[:int(rng.integers(4, m.size))].copy()
            body = m[4:]
            if body.size:
                host.cycle_via_class(body, 0x90CFC0AB)  # encrypt the mutated plaintext through the product (what Load will undo)
            b = host.Ark()
            try:
                b.parse_header(m)
                b.files(), b.ark_sizes(), b.ark_paths()
                verdicts["hdr_ok"] += 1
            except host.HostError:
                verdicts["hdr_rejected"] += 1
            b.close()
            d = bytearray(dta)
            for _ in range(int(rng.integers(1, 5))):
                d[int(rng.integers(0, len(d)))] = int(rng.integers(0, 256))
            if rng.random() < 0.2:
                d = d[:int(rng.integers(0, len(d)))]
            host.set_fix_quirks(bool(it & 1))
            try:
                host.dta_roundtrip(bytes(d))
                verdicts["dta_ok"] += 1
            except host.HostError:
                verdicts["dta_rejected"] += 1
    finally:
        host.set_fix_quirks(False)
    assert verdicts["hdr_ok"] > 100 and verdicts["hdr_rejected"] > 100 and verdicts["dta_ok"] > 50 and verdicts["dta_rejected"] > 100, verdicts
