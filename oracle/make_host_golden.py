#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- records tests/golden/host_golden.json from the COMPILED REFERENCE's host classes
(oracle/_ref/ref_host: the reference's CArk / CDtaFile / CUtils / CSettings behind oracle/ref_host_main.cpp).

    python oracle/make_host_golden.py            # rewrite the golden file (needs oracle/_ref/ref_host)
    python oracle/make_host_golden.py --check    # regenerate and compare with the committed file

Every input is built from the case's recipe alone: names and sizes from the generators below, file bytes from
oracle.splitmix_bytes, seed headers from oracle/ark_header.py (`serialise_raw`: the table verbatim, in the order
and with the link words the recipe gives) + oracle.hdr_encrypt, DTA images from oracle/dta_tree.py.  The same
functions rebuild the inputs in tests/test_ref_host_parity.py, which puts them through the C++ mirror and the
Python restatement and holds both to what is recorded here.

What is recorded per case: the recipe, and per action the reference's exit status and its outputs -- header and
DTA images of up to WHOLE_IMAGE_MAX bytes whole (hex), everything else as size + FNV-1a-64; parsed tables of up
to WHOLE_TABLE_MAX entries whole, longer ones as count + digest of their canonical text.

Two things are NOT the reference's to decide and are kept out of what is compared:
  * bytes 12..27 of a saved header's plaintext (mChecksumData) are uninitialised stack in the reference
    (CArk.cpp:912-921 never writes them): every recorded header has them set to zero (`canonical_header`);
  * the order in which a directory is enumerated belongs to the file system (oracle/win32_standin): the
    directories that `pack` cases enumerate hold no two names that differ only in case and none of [ \\ ] ^ _ `.
Exact ties in the PS4 entry order (same name ignoring case AND same two link words) are kept out as well: the
reference's comparator (CArk.cpp:977-1048) answers "true" for them, which std::sort does not allow, so their
order belongs to the standard library.  Where names tie, the recipes give them different link words.
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ark_header as AH  # noqa: E402
from oracle import dta_tree as DT  # noqa: E402
from oracle import oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "host_golden.json")
WHOLE_IMAGE_MAX = 8192
WHOLE_TABLE_MAX = 64


# ------------------------------------------------------------------------------------------ digests / records
def fnv(data):
    return f"{O.fnv1a64(np.frombuffer(bytes(data), dtype=np.uint8)):016x}"


def blob_record(data):
    data = bytes(data)
    return {"hex": data.hex()} if len(data) <= WHOLE_IMAGE_MAX else {"size": len(data), "fnv": fnv(data)}


def rows_record(rows):
    """A table as a list of rows, whole or as count + digest of its canonical text."""
    if len(rows) <= WHOLE_TABLE_MAX:
        return {"rows": rows}
    return {"n": len(rows), "fnv": fnv(json.dumps(rows, separators=(",", ":")).encode())}


def canonical_header(image):
    """A saved header with the 16 undefined mChecksumData bytes (plaintext offsets 12..27) set to zero."""
    a = np.frombuffer(bytes(image), dtype=np.uint8).copy()
    if a.size < 28 or O.hdr_decrypt(a) != 0:
        return bytes(image)
    ps4 = int.from_bytes(a[:4].tobytes(), "little") == O.MAGIC_PS4
    a[12:28] = 0
    assert O.hdr_encrypt(a, ps4) == 0
    return a.tobytes()


def table_record(arks, files):
    """arks: [(size, path bytes)], files: [(name bytes, size, offset, flags1, flags2, hash)] -> the `dump` record."""
    return {"arks": [[int(s), bytes(p).hex()] for s, p in arks],
            "files": rows_record([[bytes(f[0]).hex()] + [int(x) for x in f[1:]] for f in files])}


def saved_record(out_dir, header_name):
    """What SaveArk left in out_dir: the header (canonical) and every other file as [name, size, fnv]."""
    rec = {"header": None, "parts": []}
    for fn in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, fn), "rb") as f:
            data = f.read()
        if fn == header_name:
            rec["header"] = blob_record(canonical_header(data))
        else:
            rec["parts"].append([fn, len(data), fnv(data)])
    return rec


def tree_record(top):
    """Every file under `top` (bytes paths: names may hold any byte) as [relative name hex, size, fnv], sorted."""
    rows = []
    top = os.fsencode(top)
    for r, _, files in os.walk(top):
        for fn in files:
            p = os.path.join(r, fn)
            with open(p, "rb") as f:
                data = f.read()
            rows.append([os.path.relpath(p, top).hex(), len(data), fnv(data)])
    return {"files": rows_record(sorted(rows))}


# ------------------------------------------------------------------------------------------ generators
def synth_names(n):
    names = [f"dir{k % 97}/sub{k % 13}/f{k}.bin" for k in range(n)]
    names[: min(n, 3)] = ["readme.txt", "Dir5/UPPER.bin", "dir5/lower.bin"][: min(n, 3)]
    return names


def synth_sizes(n, seed, max_size):
    return [int(x) % max_size for x in O.splitmix_bytes(4 * n, seed).view("<u4")]


def one_bucket_names(n, crowded, bucket):
    """n names of which `crowded` fall into one bucket of the n-entry lookup table (CArk.cpp:832-843)."""
    hit = [nm for nm in (f"b/x{k}.bin" for k in range(100 * n)) if AH.name_bucket(nm, n) == bucket][:crowded]
    assert len(hit) == crowded
    rest = [f"r/y{k}.bin" for k in range(n - crowded)]
    out = []
    for k in range(max(len(hit), len(rest))):  # interleaved, so that the chain is not one run of the table
        out += hit[k:k + 1] + rest[k:k + 1]
    return out


def expand(recipe):
    """recipe -> the table it describes: names (latin-1 str, as WRITTEN), sizes, offsets, links, parts, bytes."""
    t = recipe["table"]
    if "gen" in t:
        names = synth_names(t["n"])
        sizes = synth_sizes(t["n"], t["seed"], t["max_size"])
        for k in t.get("zero_at", []):
            sizes[k] = 0
    else:
        names, sizes = list(t["names"]), list(t["sizes"])
    n = len(names)
    ps4 = recipe["ps4"]
    plat = "ps4" if ps4 else "ps3"
    offsets, ark_sizes = AH.split_into_arks(sizes, AH.even_plan(sum(sizes), recipe["n_arks"]))
    return {
        "ps4": ps4, "header_name": f"main_{plat}.hdr", "names": names, "sizes": sizes, "offsets": offsets,
        "flags1": list(t.get("flags1") or [-1] * n), "flags2": list(t.get("flags2") or [-1] * n),
        "hashes": list(t.get("hashes") or [AH.HASH_FIELD[ps4] if s else 0 for s in sizes]),
        "ark_sizes": ark_sizes, "ark_paths": [f"main_{plat}_{i}.ark" for i in range(recipe["n_arks"])],
        "data": O.splitmix_bytes(sum(sizes), recipe["data_seed"]),
    }


def seed_header(T):
    plain = AH.serialise_raw(T["names"], T["sizes"], T["offsets"], T["flags1"], T["flags2"], T["hashes"], T["ark_sizes"],
                             T["ark_paths"], T["ps4"])
    img = np.frombuffer(plain, dtype=np.uint8).copy()
    assert O.hdr_encrypt(img, T["ps4"]) == 0 and img.size < 512 * 1024 - 65536  # well under CArk.cpp:911
    return plain, img.tobytes()


def pack_inputs(recipe, T):
    """The directory a `pack` case enumerates: one file per distinct name of the table (its bytes: the entry's first
    occurrence), plus the recipe's extra files, which the reference header does not know."""
    files = {}
    for nm, s, o in zip(T["names"], T["sizes"], T["offsets"]):
        files.setdefault(nm, T["data"][o:o + s].tobytes())
    for k, (nm, s) in enumerate(recipe.get("extra", [])):
        files[nm] = O.splitmix_bytes(s, recipe["data_seed"] + 1000 + k).tobytes()
    return files


def materialise(recipe, work):
    """Write the case's inputs into the (empty) directory `work`; returns the expanded table (None for DTA)."""
    if recipe["kind"] == "dta":
        with open(os.path.join(work, "in.dta"), "wb") as f:
            f.write(dta_image(recipe))
        return None
    T = expand(recipe)
    with open(os.path.join(work, T["header_name"]), "wb") as f:
        f.write(seed_header(T)[1])
    at = 0
    for path, size in zip(T["ark_paths"], T["ark_sizes"]):
        T["data"][at:at + size].tofile(os.path.join(work, path))
        at += size
    if recipe["kind"] == "pack":
        for nm, data in pack_inputs(recipe, T).items():
            p = os.path.join(os.fsencode(work), b"in", nm.encode("latin-1"))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(data)
    return T


def _tuples(node):
    return ("tree", node[1], node[2], [_tuples(c) for c in node[3]]) if node[0] == "tree" else tuple(node)


def dta_image(recipe):
    return DT.serialise([_tuples(n) for n in recipe["trees"]], separators=recipe["separators"])


def switches(recipe):
    return ([] if recipe.get("ps4", True) else ["--ps3"]) + list(recipe.get("switches", []))


# ------------------------------------------------------------------------------------------ the reference
def _dump(header, sw, cwd):
    st, txt = O.ref_host("dump", header, switches=sw, cwd=cwd)
    rec = {"status": st}
    if st == 0:
        d = json.loads(txt.decode().strip().splitlines()[-1])
        rec.update(table_record([(a["size"], bytes.fromhex(a["path"])) for a in d["arks"]],
                                [(bytes.fromhex(f["name"]), f["size"], f["offset"], f["flags1"], f["flags2"], f["hash"])
                                 for f in d["files"]]))
    return rec


def run_reference(recipe, work):
    """Materialise the case in `work` and put it through oracle/_ref/ref_host, one action per process."""
    T = materialise(recipe, work)
    sw = switches(recipe)
    if recipe["kind"] == "dta":
        st, _ = O.ref_host("dta-resave", "in.dta", "out.dta", switches=sw, cwd=work)
        rec = {"status": st}
        if st == 0:
            with open(os.path.join(work, "out.dta"), "rb") as f:
                rec["image"] = blob_record(f.read())
        return {"dta-resave": rec}
    hdr = T["header_name"]
    os.mkdir(os.path.join(work, "out"))
    if recipe["kind"] == "pack":
        st, _ = O.ref_host("pack", hdr, "in/", "out/", switches=sw, cwd=work)
        rec = {"status": st}
        if st == 0:
            rec.update(saved_record(os.path.join(work, "out"), hdr))
            rec["table"] = _dump("out/" + hdr, sw, work)
        return {"pack": rec}
    out = {"dump": _dump(hdr, sw, work)}
    st, _ = O.ref_host("resave", hdr, "out/", switches=sw, cwd=work)
    out["resave"] = {"status": st}
    if st == 0:
        out["resave"].update(saved_record(os.path.join(work, "out"), hdr))
        out["resave"]["table"] = _dump("out/" + hdr, sw, work)
    os.mkdir(os.path.join(work, "ex"))
    st, _ = O.ref_host("extract", hdr, "ex/", switches=sw, cwd=work)
    out["extract"] = {"status": st}
    if st == 0:
        out["extract"].update(tree_record(os.path.join(work, "ex")))
    return out


# ------------------------------------------------------------------------------------------ the matrix
def cases():
    C = {}

    def both(name, table, n_arks, data_seed):
        for ps4 in (False, True):
            C[f"{name}_{'ps4' if ps4 else 'ps3'}"] = {"kind": "ark", "ps4": ps4, "table": table, "n_arks": n_arks, "data_seed": data_seed}

    def synth(n, seed, max_size, zero_at=()):
        return {"gen": "synth", "n": n, "seed": seed, "max_size": max_size, "zero_at": list(zero_at)}

    # sizes x parts
    both("n1_parts1", synth(1, 11, 3000), 1, 1)
    both("n2_parts1", synth(2, 12, 3000), 1, 2)
    both("n57_parts3", synth(57, 13, 3000, zero_at=(4, 9)), 3, 3)
    both("n1000_parts3", synth(1000, 14, 3000, zero_at=(4, 9)), 3, 4)
    both("n5000_parts8", synth(5000, 15, 200, zero_at=(4, 9)), 8, 5)
    both("n2_parts8_more_parts_than_files", synth(2, 16, 3000), 8, 6)
    # names
    both("names_differ_only_in_case", {
        "names": ["Dir/File.bin", "dir/file.bin", "DIR/FILE.BIN", "dir/other.bin", "x.bin", "X.BIN", "dir/FILE.bin"],
        "sizes": [10, 20, 30, 40, 50, 60, 70], "flags1": [5, 3, 4, -1, 2, 1, 3], "flags2": [0, 1, 2, 3, 4, 5, 0]}, 2, 7)
    both("names_no_dir_no_ext_many_dots", {
        "names": ["noext", "nodir.txt", "a.b.c.d", "dir.v2/file.tar.gz", "dir/.hidden", "trailingdot.", "d/e/f/g/h/deep.bin", "d/e.f"],
        "sizes": [7, 0, 300, 41, 5, 1, 1000, 2]}, 2, 8)
    # the entry-name reader takes 255 bytes (kiMaxStringLength, CArk.cpp:616-629); one more and it stops INSIDE the name
    both("name_length_255", {"names": ["d/" + "a" * 253, "short.bin", "e/" + "c" * 253], "sizes": [100, 200, 300]}, 1, 9)
    both("name_length_256_one_over", {"names": ["d/" + "a" * 253, "e/" + "b" * 254, "short.bin"], "sizes": [100, 200, 300]}, 1, 9)
    both("names_with_high_bytes", {
        "names": ["caf\xe9/\xfcber.bin", "\xff\xfe/\x80.dat", "dir/na\xefve.\xe9xt", "\x7f\x80\x81", "plain/ascii.bin", "\xe9", "\xff\xff\xff\xff/\xff"],
        "sizes": [64, 65, 66, 67, 68, 69, 70]}, 2, 10)
    both("many_names_in_one_bucket", {"names": one_bucket_names(48, 30, 7), "sizes": synth_sizes(48, 17, 500)}, 3, 11)
    both("duplicate_names", {
        "names": ["a/dup.bin", "b/one.bin", "a/dup.bin", "c/two.bin", "a/dup.bin"], "sizes": [11, 22, 33, 44, 55],
        "flags1": [2, -1, 0, -1, 1], "flags2": [-1, 4, -1, -1, -1]}, 2, 12)
    both("zero_sizes_first_last_adjacent", {
        "names": [f"z/f{k}.bin" for k in range(8)], "sizes": [0, 0, 10, 0, 5, 7, 0, 0]}, 3, 13)
    both("flags_and_hash_fields_carried", {
        "names": synth_names(57), "sizes": synth_sizes(57, 18, 3000), "flags1": [k * 7 - 3 for k in range(57)],
        "flags2": [1000 - k for k in range(57)], "hashes": [int(x) for x in O.splitmix_bytes(4 * 57, 19).view("<u4")]}, 3, 14)

    # pack: Load of the reference header, ConstructFromDirectory, BuildArk, SaveArk
    def pack(name, table, n_arks, data_seed, ps4=True, extra=(), sw=()):
        C[name] = {"kind": "pack", "ps4": ps4, "table": table, "n_arks": n_arks, "data_seed": data_seed,
                   "extra": [list(e) for e in extra], "switches": list(sw)}

    pack_names = [f"ps4/dir{k % 7}/sub{k % 3}/f{k}.bin" for k in range(57)]
    pack_names[:4] = ["ps4/readme.txt", "ps4/songs/credits/c.bin", "ps4/songs/other/o.bin", "ps4/config/amp.dta"]
    pack_names[7:9] = ["ps4/Zeta/Upper.BIN", "ps4/alpha/lower.bin"]  # NTFS order: alpha before Zeta; byte order: the other way round
    pack_table = {"names": pack_names, "sizes": synth_sizes(57, 21, 3000)}
    pack_table["sizes"][5] = pack_table["sizes"][6] = 0
    pack("pack_57_parts3_ps4", pack_table, 3, 21)
    pack("pack_57_parts3_ps3", pack_table, 3, 21, ps4=False)
    pack("pack_file_ends_exactly_on_planned_part_size", {"names": ["p/a.bin", "p/b.bin", "p/c.bin"], "sizes": [100, 100, 100]}, 3, 22)
    pack("pack_file_ends_one_byte_past_planned_part_size", {"names": ["p/a.bin", "p/b.bin", "p/c.bin"], "sizes": [101, 100, 99]}, 3, 23)
    pack("pack_total_so_small_trailing_part_is_empty", {"names": ["p/a.bin", "p/b.bin"], "sizes": [1, 1]}, 3, 24)
    pack("pack_duplicate_names_in_reference_header", {
        "names": ["p/dup.bin", "p/one.bin", "p/dup.bin", "q/two.bin"], "sizes": [11, 22, 33, 44],
        "flags1": [2, -1, 0, -1], "flags2": [7, -1, 9, -1]}, 2, 25)
    extra = [("ps4/new/unknown.bin", 123), ("ps4/songs/brandnew/n.bin", 45), ("ps4/songs/tut0/t.bin", 67)]
    for ign in (True, False):
        for pall in (False, True):
            pack(f"pack_unknown_files_ignore_new_{'on' if ign else 'off'}_pack_all_{'on' if pall else 'off'}", pack_table, 3, 26,
                 extra=extra, sw=([] if ign else ["--allow-new"]) + (["--pack-all"] if pall else []))

    # DTA: CDtaFile::Load -> Save
    def dta(name, trees, separators=True):
        C[name] = {"kind": "dta", "trees": trees, "separators": separators}

    def tree(ttype, node_id, kids):
        return ["tree", ttype, node_id, kids]

    every = [["int", 0, 5], ["int", 6, 6], ["int", 8, 8], ["int", 9, 9], ["float", 1, 0x3F800000], ["str", 5, "string"], ["str", 18, "id"],
             ["str", 33, "include.dta"], ["str", 35, "DEFINE"], tree(16, 3, [["int", 0, 1]]), tree(17, 4, [["str", 5, "x"]])]
    dta("dta_every_node_type", [tree(16, 1, every)])
    dta("dta_empty_top_level_tree", [tree(16, 1, [])])
    dta("dta_empty_subtree", [tree(16, 1, [["int", 0, 1], tree(16, 2, []), ["int", 0, 2]])])
    deep = tree(17, 9, [["str", 5, "bottom"], ["int", 0, -9]])
    for lvl in range(8, 1, -1):
        deep = tree(16 + lvl % 2, lvl, [["int", 6, lvl], deep, ["str", 18, f"level{lvl}"]])
    dta("dta_nested_eight_levels", [tree(16, 1, [deep])])
    three = [tree(16, 1, [["str", 5, "first"], ["int", 0, 1]]), tree(17, 2, [["str", 5, "second"]]), tree(16, 3, every)]
    dta("dta_three_top_level_trees_with_separators", three, True)
    dta("dta_three_top_level_trees_back_to_back", three, False)
    dta("dta_strings_empty_and_long", [tree(16, 1, [["str", 5, ""], ["str", 18, ""], ["str", 33, "a"], ["str", 5, "long " * 600],
                                                    ["str", 35, "caf\xe9 \xff\x80"], ["str", 5, ""]])])
    dta("dta_negative_integers", [tree(16, 1, [["int", 0, -1], ["int", 6, -(1 << 31)], ["int", 8, (1 << 31) - 1], ["int", 9, -123456789], ["int", 0, 0]])])
    dta("dta_floats_negative_zero_nan_inf_denormal", [tree(16, 1, [["float", 1, b] for b in
                                                               (0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 1, 0x00000000, 0xC2F6E979)])])
    return C


def generate():
    assert O.have_ref_host(), "oracle/_ref/ref_host is not built: make -C oracle ref (needs the reference sources)"
    O.build(ref=False)
    out = {"format": 1,
           "made_by": "oracle/make_host_golden.py over oracle/_ref/ref_host (the reference's own CArk/CDtaFile, compiled)",
           "cases": {}}
    for name, recipe in cases().items():
        work = tempfile.mkdtemp(prefix="host_golden_")
        try:
            out["cases"][name] = {"recipe": recipe, "ref": run_reference(recipe, work)}
        finally:
            shutil.rmtree(work, ignore_errors=True)
    return json.dumps(out, indent=None, separators=(",", ":"), sort_keys=False).replace('},"', '},\n"') + "\n"


if __name__ == "__main__":
    text = generate()
    if "--check" in sys.argv:
        with open(GOLDEN) as f:
            same = f.read() == text
        print("host_golden.json:", "reproduced bit for bit" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(GOLDEN, "w") as f:
        f.write(text)
    print(f"wrote {GOLDEN}: {len(text)} bytes, {len(cases())} cases")
