"""CPU-only: the code AROUND the cipher -- header wire format, lookup chains, entry order, part split, extract, pack,
the DTA tree reader and writer -- held to what the REFERENCE's own host classes did.

tests/golden/host_golden.json was recorded by oracle/make_host_golden.py from oracle/_ref/ref_host: the reference's
CArk.cpp, CDtaFile.cpp, Utils.cpp and Settings.cpp compiled for Linux against oracle/win32_standin, one action per
child process.  Every case is rebuilt here from its recipe and goes three ways:

  mirror vs golden        modulate_amd.host (the C++ mirror, default settings: the reference's quirks ON) must write the
                          reference's bytes: saved header, every part, every extracted file, the re-saved DTA image, and
                          field for field the parsed table; where the reference refused an input, the mirror must refuse it
  restatement vs golden   oracle/ark_header.py and oracle/dta_tree.py must give the same
  golden vs _ref          where oracle/_ref/ref_host is present, running the reference again gives the stored record

Not compared, because the reference does not decide them (see oracle/make_host_golden.py): the 16 uninitialised
mChecksumData bytes of a saved header (zeroed on both sides), the enumeration order of a directory (the stand-in's NTFS
order; pack inputs hold no names that differ only in case), and exact ties of the PS4 entry order.
"""
import json
import os
import struct

import numpy as np
import pytest

from oracle import ark_header as AH
from oracle import dta_tree as DT
from oracle import make_host_golden as MG

PLATFORM_CASES = [
    "n1_parts1", "n2_parts1", "n57_parts3", "n1000_parts3", "n5000_parts8", "n2_parts8_more_parts_than_files",
    "names_differ_only_in_case", "names_no_dir_no_ext_many_dots", "name_length_255", "name_length_256_one_over",
    "names_with_high_bytes", "many_names_in_one_bucket", "duplicate_names", "zero_sizes_first_last_adjacent",
    "flags_and_hash_fields_carried",
]
CASES = [f"{c}_{p}" for c in PLATFORM_CASES for p in ("ps3", "ps4")] + [
    "pack_57_parts3_ps4", "pack_57_parts3_ps3",
    "pack_file_ends_exactly_on_planned_part_size", "pack_file_ends_one_byte_past_planned_part_size",
    "pack_total_so_small_trailing_part_is_empty", "pack_duplicate_names_in_reference_header",
    "pack_unknown_files_ignore_new_on_pack_all_off", "pack_unknown_files_ignore_new_on_pack_all_on",
    "pack_unknown_files_ignore_new_off_pack_all_off", "pack_unknown_files_ignore_new_off_pack_all_on",
    "dta_every_node_type", "dta_empty_top_level_tree", "dta_empty_subtree", "dta_nested_eight_levels",
    "dta_three_top_level_trees_with_separators", "dta_three_top_level_trees_back_to_back", "dta_strings_empty_and_long",
    "dta_negative_integers", "dta_floats_negative_zero_nan_inf_denormal",
]
# the inputs the reference REFUSES (exit status = its eError ordinal): pinned here so that a re-recorded golden cannot
# quietly turn a refusal into a pass or the other way round
REFUSED = {"name_length_256_one_over_ps3": 6, "name_length_256_one_over_ps4": 6, "dta_empty_top_level_tree": 6,
           "dta_empty_subtree": 6, "dta_three_top_level_trees_back_to_back": 6}


@pytest.fixture(scope="module")
def host_golden():
    with open(MG.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def host(oracle):
    from modulate_amd import host as H
    H.lib()
    return H


@pytest.fixture()
def mirror(host):
    """The mirror at its defaults (CSettings as the reference initialises it, quirks on); restored afterwards."""
    def reset():
        host.set_flags(overwrite=True, ignore_new=True, pack_all=False, verbose=False)
        host.set_fix_quirks(False)
        host.select_platform(True)
    reset()
    yield host
    reset()


def test_the_matrix_is_whole(host_golden):
    """No case may go missing from the golden file, and the reference's refusals are the ones written down here."""
    assert list(host_golden["cases"]) == CASES == list(MG.cases())
    for name, case in host_golden["cases"].items():
        assert case["recipe"] == json.loads(json.dumps(MG.cases()[name])), name
        statuses = {rec["status"] for rec in case["ref"].values()}
        assert statuses == {REFUSED.get(name, 0)}, (name, statuses)


# ------------------------------------------------------------------------------------------------ mirror vs golden
def _status(host, call):
    """0, or the eError ordinal the mirror refused with -- and then modhost_last_error() must say so."""
    try:
        call()
        return 0
    except host.HostError as e:
        assert e.code != 0 and host.lib().modhost_last_error() != b"", "a refusal must leave its reason behind"
        return e.code


def _mirror_table(host, header):
    rec = {}

    def load():
        a = host.Ark().load(header)
        files = [(f["name"].encode("latin-1"), f["size"], f["offset"], f["flags1"], f["flags2"], f["hash"]) for f in a.files()]
        rec.update(MG.table_record(zip(a.ark_sizes(), [p.encode("latin-1") for p in a.ark_paths()]), files))
        a.close()
    return {"status": _status(host, load), **rec}


def run_mirror(host, recipe, work):
    """The same actions as MG.run_reference, through modulate_amd.host, into the same record."""
    T = MG.materialise(recipe, work)
    if recipe["kind"] == "dta":
        rec = {}

        def resave():
            with open(os.path.join(work, "in.dta"), "rb") as f:
                rec["image"] = MG.blob_record(host.dta_roundtrip(f.read())[0])
        return {"dta-resave": {"status": _status(host, resave), **rec}}
    sw = recipe.get("switches", [])
    host.select_platform(recipe["ps4"])
    host.set_flags(overwrite=True, ignore_new="--allow-new" not in sw, pack_all="--pack-all" in sw, verbose=False)
    hdr = T["header_name"]
    os.mkdir(os.path.join(work, "out"))
    if recipe["kind"] == "pack":
        def pack():
            ref = host.Ark().load(hdr)
            a = host.Ark()
            a.construct_from_directory("in/", ref)
            a.build("in/")
            a.save("out/", hdr)
            a.close(), ref.close()
        rec = {"status": _status(host, pack)}
        if rec["status"] == 0:
            rec.update(MG.saved_record(os.path.join(work, "out"), hdr))
            rec["table"] = _mirror_table(host, "out/" + hdr)
        return {"pack": rec}
    out = {"dump": _mirror_table(host, hdr)}

    def resave():
        a = host.Ark().load(hdr)
        a.load_data()
        a.save("out/", hdr)
        a.close()
    out["resave"] = {"status": _status(host, resave)}
    if out["resave"]["status"] == 0:
        out["resave"].update(MG.saved_record(os.path.join(work, "out"), hdr))
        out["resave"]["table"] = _mirror_table(host, "out/" + hdr)
    os.mkdir(os.path.join(work, "ex"))

    def extract():
        a = host.Ark().load(hdr)
        a.extract("ex/")
        a.close()
    out["extract"] = {"status": _status(host, extract)}
    if out["extract"]["status"] == 0:
        out["extract"].update(MG.tree_record(os.path.join(work, "ex")))
    return out


def _assert_same(got, want, name):
    """Record against record, leaf by leaf, so that a failure names the action and the field."""
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    for action in want:
        for field in sorted(set(want[action]) | set(got[action])):
            assert got[action].get(field) == want[action].get(field), f"{name}: {action}.{field} differs from the reference"


@pytest.mark.parametrize("name", CASES)
def test_mirror_matches_reference(mirror, host_golden, tmp_path, monkeypatch, name):
    """Pins, with the quirks the mirror keeps at its defaults: SaveArk's demand for the header in the working directory
    (the cases run where it lies), Save writing top-level DTA trees back to back (dta_three_top_level_trees_*),
    ExtractFiles walking every entry, and the entry-name reader stopping inside a name of more than 255 bytes
    (name_length_256_one_over_*: refused, as the reference refuses it)."""
    case = host_golden["cases"][name]
    monkeypatch.chdir(tmp_path)  # the reference resolves part files and the header name against the working directory
    _assert_same(run_mirror(mirror, case["recipe"], str(tmp_path)), case["ref"], name)


# ------------------------------------------------------------------------------------------- restatement vs golden
def _encrypted(oracle, plain, ps4):
    img = np.frombuffer(plain, dtype=np.uint8).copy()
    assert oracle.hdr_encrypt(img, ps4) == 0
    return img.tobytes()


def _parsed_record(p):
    return MG.table_record(zip(p["ark_sizes"], [s.encode("latin-1") for s in p["ark_paths"]]),
                           [(f["name"].encode("latin-1"), f["size"], f["offset"], f["flags1"], f["flags2"], f["hash"]) for f in p["files"]])


def _saved_by_restatement(oracle, p, ark_sizes, ps4):
    """What SaveArk makes of a parsed table, by oracle/ark_header.py: (header record, table record of that header)."""
    f = p["files"]
    plain = AH.serialise([x["name"] for x in f], [x["size"] for x in f], [x["offset"] for x in f], ark_sizes, p["ark_paths"], ps4,
                         flags1=[x["flags1"] for x in f], flags2=[x["flags2"] for x in f])
    again = AH.parse(plain)
    assert again["end"] == len(plain)
    for x in f:  # the header's own lookup structure finds every name (name_bucket, chain links, bucket table) ...
        i = AH.lookup(again, x["name"])
        if AH.name_bucket(x["name"], len(f)) < 0:  # ... but those whose signed-char hash is negative: no slot for them (CArk.cpp:1117-1131)
            assert i == -1 and max(x["name"].encode("latin-1")) >= 0x80
            continue
        assert i >= 0 and again["files"][i]["name"] == x["name"], x["name"]
    assert AH.lookup(again, "no/such/file") == -1
    return MG.blob_record(_encrypted(oracle, plain, ps4)), {"status": 0, **_parsed_record(again)}


def _parts_record(T, ark_sizes, data):
    rows, at = [], 0
    for path, size in zip(T["ark_paths"], ark_sizes):
        rows.append([path, size, MG.fnv(data[at:at + size])])
        at += size
    return sorted(rows)


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference(oracle, host_golden, name):
    case = host_golden["cases"][name]
    recipe, ref = case["recipe"], case["ref"]
    if recipe["kind"] == "dta":
        blob, want = MG.dta_image(recipe), ref["dta-resave"]
        if want["status"] != 0:
            with pytest.raises(ValueError):
                DT.parse(blob)
            return
        # the reference's Save writes the top-level trees back to back (CDtaFile.cpp:371-374)
        assert MG.blob_record(DT.serialise(DT.parse(blob), separators=False)) == want["image"]
        return
    T = MG.expand(recipe)
    ps4 = T["ps4"]
    seed = MG.seed_header(T)[0]
    if ref[next(iter(ref))]["status"] != 0:
        with pytest.raises((ValueError, AssertionError, struct.error)):
            AH.parse(seed)
        return
    p = AH.parse(seed)
    assert p["end"] == len(seed)
    if recipe["kind"] == "ark":
        assert {"status": 0, **_parsed_record(p)} == ref["dump"]
        header, table = _saved_by_restatement(oracle, p, p["ark_sizes"], ps4)
        assert header == ref["resave"]["header"] and table == ref["resave"]["table"]
        assert _parts_record(T, p["ark_sizes"], T["data"]) == ref["resave"]["parts"]
        files = {}
        for f in p["files"]:  # a later duplicate overwrites an earlier one (CArk.cpp:439-457, overwriting on)
            files[f["name"]] = T["data"][f["offset"]:f["offset"] + f["size"]].tobytes()
        rows = sorted([nm.encode("latin-1").hex(), len(b), MG.fnv(b)] for nm, b in files.items())
        assert MG.rows_record(rows) == ref["extract"]["files"]
        return
    # pack: which files, in which order (ConstructFromDirectory), where they lie (BuildArk), what is written (SaveArk)
    inputs = MG.pack_inputs(recipe, T)
    sw = recipe["switches"]
    first = {}
    for f in p["files"]:
        first.setdefault(f["name"], f)
    names = AH.construct_from_directory(inputs, first, ignore_new="--allow-new" not in sw, pack_all="--pack-all" in sw)
    sizes = [len(inputs[nm]) for nm in names]
    offsets, ark_sizes = AH.split_into_arks(sizes, AH.even_plan(sum(sizes), recipe["n_arks"]))
    table = {"ark_paths": p["ark_paths"], "files": [
        {"name": nm, "size": s, "offset": o, "flags1": first[nm]["flags1"] if nm in first else -1,
         "flags2": first[nm]["flags2"] if nm in first else -1} for nm, s, o in zip(names, sizes, offsets)]}
    header, saved = _saved_by_restatement(oracle, table, ark_sizes, ps4)
    assert saved["arks"] == ref["pack"]["table"]["arks"], "part layout"
    assert header == ref["pack"]["header"] and saved == ref["pack"]["table"]
    data = b"".join(inputs[nm] for nm in names)
    assert _parts_record(T, ark_sizes, np.frombuffer(data, dtype=np.uint8)) == ref["pack"]["parts"]


# --------------------------------------------------------------------------------------------------- golden vs _ref
@pytest.mark.parametrize("name", CASES)
def test_golden_matches_compiled_reference(oracle, host_golden, tmp_path, name):
    """Where oracle/_ref/ref_host is present (it is built from the reference's sources, which do not travel with a
    checkout), running the reference again gives the stored record."""
    if oracle.have_ref_host():
        case = host_golden["cases"][name]
        _assert_same(MG.run_reference(case["recipe"], str(tmp_path)), case["ref"], name)
