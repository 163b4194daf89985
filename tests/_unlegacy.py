"""Helpers of the Shrink / Reduce / Implode readers' tests: loaders of the CPU models (tests/unlegacy/unlegacy_host.cpp = the product's
zada_unlegacy_logic.h with one lane; tests/unlegacy/unlegacy_model.c = the decoders as the reference states them, and a small imploder), the
stand-alone program of the sanitizer run, the PKZIP fixtures, and the corpora of valid, damaged and crafted streams the CPU and GPU tests share."""
import ctypes
import json
import os
import random
import struct
import subprocess

import numpy as np

import _legacy as L
from _common import GOLDEN, ROOT

E_DATA = -7
_cache = {}
_DIR = os.path.join(ROOT, "tests", "unlegacy")
_HOST = os.path.join(_DIR, "unlegacy_host.cpp")
_MODEL = os.path.join(_DIR, "unlegacy_model.c")
_HDR = os.path.join(ROOT, "zip-ada_amd", "csrc", "zada_unlegacy_logic.h")
RULES = ("ok", "INPUT_END", "OUTPUT_FULL", "SHRINK_FIRST", "SHRINK_CODE_SIZE", "SHRINK_SPECIAL", "SHRINK_STACK", "IMPLODE_RUNS", "IMPLODE_TREE")   # enum UlgRule
CENSUS = ("sh_clears", "sh_rises", "sh_orphan_first", "sh_orphan_linked", "sh_full_table",
          "rd_lit144", "rd_two_byte_length", "rd_b1", "rd_b2", "rd_b3", "rd_b4", "rd_b5", "rd_b6", "rd_b8", "rd_zero_fill", "rd_overlap",
          "im_extra_length", "im_zero_fill", "im_overlap", "im_dist_4096", "im_dist_8192", "im_beyond_32k")
IMPLODE_FLAGS = (0, 2, 4, 6)                           # general-purpose bit 1: 8 KiB dictionary, bit 2: three trees


def _newer(p, *srcs):
    return os.path.exists(p) and os.path.getmtime(p) >= max(os.path.getmtime(s) for s in srcs)


def host():
    """The logic header on the CPU."""
    if "h" not in _cache:
        p = os.path.join(_DIR, "libunlegacy_host.so")
        if not _newer(p, _HOST, _HDR):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, _HOST], check=True)
        M = ctypes.CDLL(p)
        M.ug_unlegacy.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
        M.ug_rule_name.restype = ctypes.c_char_p
        M.ug_rule_name.argtypes = [ctypes.c_uint]
        _cache["h"] = M
    return _cache["h"]


def stated():
    """The decoders as the reference states them, and the imploder."""
    if "s" not in _cache:
        p = os.path.join(_DIR, "libunlegacy_model.so")
        if not _newer(p, _MODEL):
            subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", p, _MODEL], check=True)
        M = ctypes.CDLL(p)
        M.um_decode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        M.um_implode.restype = ctypes.c_uint64
        M.um_implode.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64]
        assert M.um_census_count() == len(CENSUS)
        _cache["s"] = M
    return _cache["s"]


def check_program():
    """The stand-alone program of unlegacy_host.cpp under ASan + UBSan (cases file -> results file)."""
    p = os.path.join(_DIR, "unlegacy_check_asan")
    if not _newer(p, _HOST, _HDR):
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17",
                        "-o", p, _HOST], check=True)
    return p


def _buf(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy() if len(b) else np.zeros(1, np.uint8)


def host_decode(method, flags, stream, cap, crc=0xFFFFFFFF):
    """The logic header -> (rc, bytes, out_len, in_used, crc register, (rule, input byte, output position, 0))."""
    src, out = _buf(stream), np.empty(max(cap, 1), dtype=np.uint8)
    res = (ctypes.c_uint64 * 8)()
    rc = host().ug_unlegacy(method, flags, src.ctypes.data, len(stream), out.ctypes.data, cap, crc, res)
    assert res[6] == 0, "the logic header put a byte beyond cap"
    return rc, out[:res[0]].tobytes(), int(res[0]), int(res[1]), int(res[4]), (int(res[2]), int(res[3]), int(res[5]), 0)


def stated_decode(method, flags, stream, cap, census=None):
    """The stated form -> (rc, bytes, out_len, in_used, (rule, input byte, output position, 0)); census (numpy, len (CENSUS)) is added to."""
    src, out = _buf(stream), np.empty(max(cap, 1), dtype=np.uint8)
    res = (ctypes.c_uint64 * 5)()
    cs = census if census is not None else np.zeros(len(CENSUS), dtype=np.uint64)
    rc = stated().um_decode(method, flags, src.ctypes.data, len(stream), out.ctypes.data, cap, res, cs.ctypes.data)
    return rc, out[:res[0]].tobytes(), int(res[0]), int(res[1]), (int(res[2]), int(res[3]), int(res[4]), 0)


def implode(data, flags, zero_reach=0):
    data = bytes(data)
    cap = 2 * len(data) + 1024
    src, out = _buf(data), np.empty(cap, dtype=np.uint8)
    k = stated().um_implode(src.ctypes.data, len(data), flags, zero_reach, out.ctypes.data, cap)
    assert k <= cap
    return out[:k].tobytes()


def fixtures():
    """PKZIP's own streams: [(row of many_formats_legacy.json, payload)]."""
    if "fx" not in _cache:
        with open(os.path.join(GOLDEN, "many_formats_legacy.json")) as f:
            rows = json.load(f)["entries"]
        _cache["fx"] = []
        for r in rows:
            with open(os.path.join(GOLDEN, r["file"]), "rb") as f:
                _cache["fx"].append((r, f.read()))
    return _cache["fx"]


def encode(data, method):
    """The stream of the project's encoder models for method 1 .. 5."""
    return L.shrink(data)[0] if method == 1 else L.reduce(data, method - 1)[0]


def shrink_no_clear(data):
    """A Shrink stream that never clears: plain LZW with "256, 1" in front of the first code of each size, which goes on with a full table (nodes
    up to 8192 are taken; the table then adds nothing, as PKZIP's format allows)."""
    bits, at, size, table, nxt, w = 0, 0, 9, {}, 257, b""
    def emit(code):
        nonlocal bits, at, size
        while code >> size:
            bits |= (256 | 1 << size) << at
            at += 2 * size
            size += 1
        bits |= code << at
        at += size
    for c in bytes(data):
        wc = w + bytes([c])
        if len(wc) == 1 or wc in table:
            w = wc
            continue
        emit(w[0] if len(w) == 1 else table[w])
        if nxt <= 8192:
            if nxt < 8192:                              # (node 8192 is taken by the decoder, but no 13-bit code names it)
                table[wc] = nxt
            nxt += 1
        w = bytes([c])
    if w:
        emit(w[0] if len(w) == 1 else table[w])
    return bits.to_bytes((at + 7) // 8, "little")


def full_table_input():
    return L.rnd(2, 80 << 10, b"abcd")                 # (more than 7936 LZW phrases: the table fills at 8192)


def far_input(max_dist, seed=31):
    """A block, then bytes with no repeats of it, then the block again at exactly max_dist."""
    r = random.Random(seed)
    block = bytes(r.choices(range(256), k=40))
    return block + bytes(r.choices(range(256), k=max_dist - 40)) + block + b"tail"


IMPLODE_SIZES = (1, 2, 3, 4095, 4096, 4097, 8191, 8192, 8193, 33000, 70000)


def implode_inputs():
    """[(name, data, zero_reach)]: the sizes the issue names, the largest distances, a long run (the extra length byte), leading zeros reached from in
    front of the entry (zero-fill), short periods (overlap)."""
    if "ii" not in _cache:
        ins = [("edge_%d" % n, L.edge_input(n, seed=17), 0) for n in IMPLODE_SIZES]
        ins += [("far_4096", far_input(4096), 0), ("far_8192", far_input(8192), 0), ("run", b"A" * 700 + b"xyz" + b"ab" * 300, 0),
                ("zeros_reach_5", bytes(50) + L.edge_input(600, seed=18), 5), ("zeros_reach_4096", bytes(400) + L.edge_input(300, seed=19), 4096),
                ("random_2k", L.rnd(20, 2000, bytes(range(256))), 0)]
        _cache["ii"] = ins
    return _cache["ii"]


def crafted():
    """name -> (method, flags, stream, cap, rule expected): streams for the rules and branches random damage does not reach."""
    def codes9(*cs):
        v = 0
        for i, c in enumerate(cs):
            v |= c << (9 * i)
        return v.to_bytes((9 * len(cs) + 7) // 8, "little")
    rise = codes9(97, 256, 1)                           # 9-bit codes; behind them the size is 10, 11, ..
    bits, at = int.from_bytes(rise, "little"), 27
    for size in (10, 11, 12, 13):
        bits |= 256 << at | 1 << (at + size)
        at += 2 * size
    return {
        "shrink_first_not_literal": (1, 0, codes9(300, 97), 10, 3),
        "shrink_size_14": (1, 0, bits.to_bytes((at + 7) // 8, "little"), 10, 4),
        "shrink_special_3": (1, 0, codes9(97, 256, 3), 10, 5),
        # 300 is free: the node added behind it (258) has a free parent; 258 twice in a row then walks 258 -> 300 -> Last_Incode = 258 -> ..
        "shrink_cycle": (1, 0, codes9(97, 300, 97, 258, 258), 100000, 6),
        "shrink_orphans_valid": (1, 0, codes9(97, 300, 97, 258, 98), 8, 0),
        "shrink_cap_0": (1, 0, b"", 0, 0),
        "reduce_zero_fill": (5, 0, bytes(192) + bytes([144, 1, 5, 144, 2, 0, 65]), 10, 0),
        "reduce_slen_63": (2, 0, _reduce_wide(), 6, 0),
        "reduce_cap_0_no_tables": (3, 0, bytes(100), 0, 1),
        "implode_runs_short": (6, 0, bytes([0, 0xF0]), 10, 7),
        "implode_runs_long": (6, 0, bytes([4, 0xF5, 0xF5, 0xF5, 0xF5, 0x05]), 10, 7),
        "implode_tree_over": (6, 0, bytes([3, 0xF0, 0xF0, 0xF0, 0xF0]), 10, 8),
        "implode_tree_incomplete": (6, 4, bytes([15] + [0xFF] * 16), 10, 8),
        "implode_no_trees": (6, 6, b"", 0, 1),
    }


def _reduce_wide():
    """Follower sets with Slen = 63 for the byte 0 (6 index bits), as the reference accepts: 'A' is follower 62 of 0."""
    bits, at = 0, 0
    for x in range(255, -1, -1):
        if x == 0:
            bits |= 63 << at
            at += 6
            for i in range(63):
                bits |= (65 if i == 62 else i + 100) << at
                at += 8
        else:
            at += 6
    # last_char = 0: flag 0 + index 62 -> 65; last_char = 65: Slen 0, 8 plain bits -> 0; and again
    for _ in range(3):
        at += 1
        bits |= 62 << at
        at += 6 + 8
    return bits.to_bytes((at + 7) // 8, "little")


def valid_streams():
    """[(method, flags, stream, data)]: small valid streams of every method and flag combination, the bases of the damaged corpus."""
    if "vs" not in _cache:
        out = []
        for method in (1, 2, 3, 4, 5):
            for n in (0, 1, 2, 40, 300, 1500, 3000):
                d = L.edge_input(n, seed=40 + method)
                out.append((method, 0, encode(d, method), d))
            d = L.rnd(50 + method, 600, bytes(range(256)))
            out.append((method, 0, encode(d, method), d))
        for flags in IMPLODE_FLAGS:
            for n in (1, 3, 40, 300, 1500, 3000):
                d = L.edge_input(n, seed=60 + flags)
                out.append((6, flags, implode(d, flags), d))
            d = bytes(30) + L.edge_input(500, seed=70)
            out.append((6, flags, implode(d, flags, zero_reach=7), d))
        _cache["vs"] = out
    return _cache["vs"]


def damaged_corpus(count=20000, seed=2024):
    """[(method, flags, stream, cap)]: seeded damage of valid streams, spread over the six methods and the Implode flags: bit flips, byte edits,
    truncations, cap one less / one more / half; behind them the crafted streams."""
    key = ("dc", count, seed)
    if key not in _cache:
        r = random.Random(seed)
        bases = valid_streams()
        by = {}
        for b in bases:
            by.setdefault((b[0], b[1]), []).append(b)
        groups = sorted(by)
        out = []
        for i in range(count):
            method, flags, s, d = r.choice(by[groups[i % len(groups)]])
            s, cap, kind = bytearray(s), len(d), r.randrange(8)
            if kind <= 1 and s:
                for _ in range(1 if kind == 0 else r.randint(2, 6)):
                    s[r.randrange(len(s))] ^= 1 << r.randrange(8)
            elif kind == 2 and s:
                s[r.randrange(len(s))] = r.randrange(256)
            elif kind == 3 and s:
                s = s[:r.randrange(len(s))]
            elif kind == 4:
                cap = max(cap - 1, 0)
            elif kind == 5:
                cap += 1
            elif kind == 6:
                cap //= 2
            elif s:                                         # an edit in the tables / the first codes
                s[r.randrange(min(len(s), 40))] = r.randrange(256)
            out.append((method, flags, bytes(s), cap))
        out += [(m, f, s, cap) for m, f, s, cap, _ in crafted().values()]
        _cache[key] = out
    return _cache[key]


def run_program(cases, tmp_path):
    """The cases through the sanitizer build of the stand-alone program -> numpy [len (cases), 9]: rc and the eight values of ug_unlegacy."""
    cf, rf = os.path.join(str(tmp_path), "cases.bin"), os.path.join(str(tmp_path), "results.bin")
    with open(cf, "wb") as f:
        for method, flags, s, cap in cases:
            f.write(struct.pack("<IIQQ", method, flags, cap, len(s)) + s)
    r = subprocess.run([check_program(), cf, rf], capture_output=True, text=True)
    assert r.returncode == 0 and ("%d cases" % len(cases)) in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    return np.fromfile(rf, dtype=np.uint64).reshape(len(cases), 9)


def one_entry_zip(name, payload, method, flags, crc, usize):
    nm = name.encode()
    local = struct.pack("<IHHHHHIIIHH", 0x04034B50, 10, flags, method, 0, 0x21, crc, len(payload), usize, len(nm), 0) + nm
    central = struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 20, 10, flags, method, 0, 0x21, crc, len(payload), usize, len(nm), 0, 0, 0, 0, 0, 0) + nm
    return local + payload, central


def zip_of(entries):
    """entries: [(name, payload, method, flags, crc, usize)] -> one archive."""
    body, cd = b"", b""
    for name, payload, method, flags, crc, usize in entries:
        local, central = one_entry_zip(name, payload, method, flags, crc, usize)
        central = central[:42] + struct.pack("<I", len(body)) + central[46:]
        body += local
        cd += central
    return body + cd + struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, len(entries), len(entries), len(cd), len(body), 0)
