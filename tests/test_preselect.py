"""Preselection without a GPU: Guess_Type_from_Name (zip-compress.adb:330-424) and Compress_Data's choice of a single method
(:243-327) as the product library exports them (zada_guess_type_from_name, zada_preselect), and the Python enums against the Ada
'Pos values.  The library is loaded in a child process (as test_host_asan.py does): the tables below are transcribed from the Ada
sources, not taken from the product."""
import json
import os
import subprocess
import sys

from _common import ROOT

# Compression_Method (zip-compress.ads:59-122), in declaration order: 'Pos is the index
ADA_METHODS = [
    "Store", "Shrink_1", "Reduce_1", "Reduce_2", "Reduce_3", "Reduce_4",
    "Deflate_Fixed", "Deflate_0", "Deflate_1", "Deflate_2", "Deflate_3", "Deflate_R",
    "BZip2_1", "BZip2_2", "BZip2_3",
    "LZMA_0", "LZMA_1", "LZMA_2", "LZMA_3",
    "LZMA_2_for_Zip_in_Zip", "LZMA_3_for_Zip_in_Zip", "LZMA_2_for_Source", "LZMA_3_for_Source",
    "LZMA_for_JPEG", "LZMA_for_ARW", "LZMA_for_ORF", "LZMA_for_MP3", "LZMA_for_MP4", "LZMA_for_PGM", "LZMA_for_PPM",
    "LZMA_for_PNG", "LZMA_for_GIF", "LZMA_for_WAV", "LZMA_for_AU",
    "Preselection_1", "Preselection_2",
]
P = {name: i for i, name in enumerate(ADA_METHODS)}

# Data_Content_Type (zip-compress.ads:151-160), in declaration order
ADA_TYPES = ["neutral", "source_code", "text_formatted_text_or_dna", "text_data", "JPEG", "ARW_RW2", "ORF_CR2", "Zip_in_Zip",
             "GIF", "PNG", "PGM", "PPM", "WAV", "AU", "MP3", "MP4"]
T = {name: i for i, name in enumerate(ADA_TYPES)}

# Guess_Type_from_Name's lists, in the order the function tests them (HTM / HTML appear twice: the first list wins)
EXT_LISTS = [
    (["JPG", "JPEG"], "JPEG"),
    (["A", "ADA", "ADS", "ADB", "PRC", "PKG", "HAC", "GPR", "F", "FOR", "C", "H", "CPP", "HPP", "DEF", "ASM", "JAVA", "CS",
      "PAS", "INC", "LPR", "PP", "M", "M4", "MAK", "IN", "SH", "BAT", "CMD", "PO", "XML", "XSL", "SGML", "AUP", "HTM", "HTML",
      "JS", "LSP", "SCM", "SQL", "PDB", "PL"], "source_code"),
    (["CFG", "INI", "LOG", "CSV", "SVG", "JSON"], "text_data"),
    (["TXT", "RTF", "HTM", "HTML", "GB", "FASTA"], "text_formatted_text_or_dna"),
    (["EPUB", "ZIP", "JAR", "ODB", "ODS", "ODT", "OTR", "OTS", "OTT", "CRX", "NTH", "DOCX", "PPTX", "XLSX", "XLSB", "XLSM"], "Zip_in_Zip"),
    (["ORF", "CR2", "RAF", "SRW"], "ORF_CR2"),
    (["ARW", "RW2", "NEF", "DNG", "X3F"], "ARW_RW2"),
    (["PGM"], "PGM"), (["PPM"], "PPM"), (["MP3"], "MP3"), (["MTS", "MP4", "M4A", "M4P"], "MP4"),
    (["PNG"], "PNG"), (["GIF"], "GIF"), (["WAV", "UAX"], "WAV"), (["AU"], "AU"),
]


def expected_names():
    want = {}
    for exts, t in EXT_LISTS:
        for e in exts:
            for name in ("file." + e, "file." + e.lower(), "dir/sub.d/x." + "".join(ch.lower() if k % 2 else ch for k, ch in enumerate(e))):
                want.setdefault(name, T[t])
    want.update({
        "README": T["neutral"], "noext": T["neutral"], "": T["neutral"], "trailing.": T["neutral"], ".": T["neutral"],
        "dir.jpg/file": T["neutral"], "dir.txt/readme": T["neutral"], "a.tar.gz": T["neutral"], "a.gz.txt": T["text_formatted_text_or_dna"],
        "page.htm": T["source_code"], "PAGE.HTML": T["source_code"], "x.jpeg.ZIP": T["Zip_in_Zip"], ".Adb": T["source_code"],
        "photo.JpG": T["JPEG"], "unknown.xyz": T["neutral"], "x.ADBX": T["neutral"], "x.mp": T["neutral"],
    })
    return want


def expected_preselect(method, hint, known, size):
    """Compress_Data (zip-compress.adb:243-327), transcribed."""
    if method < P["Preselection_1"]:
        return method
    below = lambda t: known and size < t
    fast = method == P["Preselection_1"] or below(10000)
    typed = {"JPEG": "LZMA_for_JPEG", "ARW_RW2": "LZMA_for_ARW", "ORF_CR2": "LZMA_for_ORF", "MP3": "LZMA_for_MP3", "MP4": "LZMA_for_MP4",
             "PGM": "LZMA_for_PGM", "PPM": "LZMA_for_PPM", "PNG": "LZMA_for_PNG", "WAV": "LZMA_for_WAV", "AU": "LZMA_for_AU"}
    h = ADA_TYPES[hint]
    if h in ("neutral", "text_data"):
        m = "Deflate_3" if below(9000) else "LZMA_2" if fast else "LZMA_3"
    elif h in typed:
        m = "Deflate_3" if below(2250) else typed[h]
    elif h == "GIF":
        m = "Deflate_1" if below(350) else "LZMA_for_GIF"
    elif h == "Zip_in_Zip":
        m = "Deflate_3" if below(1000) else "LZMA_2_for_Zip_in_Zip" if fast else "LZMA_3_for_Zip_in_Zip"
    elif h == "source_code":
        m = "Deflate_3" if below(8000) else "LZMA_2_for_Source" if fast else "LZMA_3_for_Source" if below(15000) else "BZip2_3"
    else:
        m = "Deflate_3" if below(9000) else "LZMA_2" if fast else "LZMA_3" if below(15000) else "BZip2_3"
    return P[m]


SIZES = sorted({0, 1} | {t + d for t in (350, 1000, 2250, 8000, 9000, 10000, 15000) for d in (-1, 0, 1)} | {1 << 20, 1 << 33})

CHILD = r'''
import ctypes, json, os, sys
ROOT = %(root)r
sys.path.insert(0, ROOT)
L = ctypes.CDLL(os.path.join(ROOT, "zip-ada_amd", "libzada_hip.so"))
L.zada_guess_type_from_name.argtypes = [ctypes.c_char_p]
L.zada_preselect.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64]
req = json.loads(sys.stdin.read())
out = {"names": {n: L.zada_guess_type_from_name(n.encode()) for n in req["names"]},
       "null": L.zada_guess_type_from_name(None),
       "presel": [L.zada_preselect(m, h, k, s) for m, h, k, s in req["presel"]]}
import importlib
za = importlib.import_module("zip-ada_amd")
out["py_names"] = {n: za.guess_type_from_name(n) for n in req["names"][:50]}
out["py_presel"] = [za.preselect(m, h, s if k else None) for m, h, k, s in req["presel"][:200]]
out["Method"] = {k: v for k, v in vars(za.Method).items() if not k.startswith("_")}
out["ContentType"] = {k: v for k, v in vars(za.ContentType).items() if not k.startswith("_")}
print(json.dumps(out))
'''


def run_child(req):
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], input=json.dumps(req), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


_cache = {}


def results():
    if "r" not in _cache:
        presel = [(m, h, k, s) for m in (P["Preselection_1"], P["Preselection_2"]) for h in range(16) for k in (0, 1) for s in (SIZES if k else [0])]
        presel += [(m, h, 1, 5000) for m in range(P["Preselection_1"]) for h in (0, 4, 8)]
        _cache["req"] = {"names": sorted(expected_names()), "presel": presel}
        _cache["r"] = run_child(_cache["req"])
    return _cache["req"], _cache["r"]


def test_guess_type_from_name_matches_the_reference_lists():
    req, r = results()
    want = expected_names()
    bad = {n: (r["names"][n], want[n]) for n in req["names"] if r["names"][n] != want[n]}
    assert not bad, bad
    assert r["null"] == T["neutral"]
    assert all(r["py_names"][n] == want[n] for n in r["py_names"])


def test_preselect_matches_compress_data_on_both_sides_of_every_threshold():
    req, r = results()
    bad = [(q, got, expected_preselect(*q)) for q, got in zip(req["presel"], r["presel"]) if got != expected_preselect(*q)]
    assert not bad, bad[:20]
    assert r["py_presel"] == r["presel"][:200]
    # the quirks the issue names, spelled out
    got = {tuple(q): g for q, g in zip(req["presel"], r["presel"])}
    p1, p2 = P["Preselection_1"], P["Preselection_2"]
    assert got[(p2, T["GIF"], 1, 349)] == P["Deflate_1"] and got[(p2, T["GIF"], 1, 350)] == P["LZMA_for_GIF"]
    assert got[(p2, T["source_code"], 1, 14999)] == P["LZMA_3_for_Source"] and got[(p2, T["source_code"], 1, 15000)] == P["BZip2_3"]
    assert got[(p2, T["text_formatted_text_or_dna"], 1, 15000)] == P["BZip2_3"] and got[(p1, T["source_code"], 1, 15000)] == P["LZMA_2_for_Source"]
    assert got[(p2, T["neutral"], 1, 9999)] == P["LZMA_2"] and got[(p2, T["neutral"], 1, 10000)] == P["LZMA_3"]
    assert got[(p2, T["neutral"], 0, 0)] == P["LZMA_3"] and got[(p1, T["neutral"], 0, 0)] == P["LZMA_2"]
    assert got[(p2, T["Zip_in_Zip"], 0, 0)] == P["LZMA_3_for_Zip_in_Zip"] and got[(p2, T["JPEG"], 1, 2249)] == P["Deflate_3"]


def test_python_enums_are_the_ada_pos_values():
    _, r = results()
    assert r["Method"] == P, {k: (r["Method"].get(k), P.get(k)) for k in set(r["Method"]) | set(P) if r["Method"].get(k) != P.get(k)}
    assert r["ContentType"] == T
