"""Helpers of the Inflate tests: loader of the CPU model (tests/inflate/inflate_host.cpp = zip-ada_amd/csrc/zada_inflate_logic.h with one lane),
the corpora of valid and damaged streams, and the rule that says which damaged streams zlib accepts."""
import ctypes
import json
import os
import subprocess
import zlib

import numpy as np

from _common import GOLDEN, ROOT, edge_inputs, few_symbol_inputs, oracle_deflate

E_DATA = -7
_cache = {}
_DIR = os.path.join(ROOT, "tests", "inflate")
_SRC = os.path.join(_DIR, "inflate_host.cpp")
_HDR = os.path.join(ROOT, "zip-ada_amd", "csrc", "zada_inflate_logic.h")


def build_model(asan=False):
    p = os.path.join(_DIR, "libinflate_host_asan.so" if asan else "libinflate_host.so")
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if asan else ["-O2"]
        subprocess.run(["g++"] + flags + ["-std=c++17", "-fPIC", "-shared", "-o", p, _SRC], check=True)
    return p


def load_model(path):
    M = ctypes.CDLL(path)
    M.im_inflate.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    M.im_rule_name.restype = ctypes.c_char_p
    M.im_rule_name.argtypes = [ctypes.c_uint]
    M.im_crypt_decode.restype = None
    M.im_crypt_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    return M


def model():
    if "m" not in _cache:
        _cache["m"] = load_model(build_model())
    return _cache["m"]


def model_inflate(payload, cap, fmt=8, crc=0xFFFFFFFF, M=None):
    """-> (rc, bytes, out_len, in_used, crc register, rule name).  The buffers are exact-size heap copies, so that a sanitizer sees a byte too many."""
    M = M or model()
    src = np.frombuffer(bytes(payload), dtype=np.uint8).copy() if len(payload) else np.zeros(0, np.uint8)
    out = np.empty(cap, dtype=np.uint8)
    res = (ctypes.c_uint64 * 6)()
    rc = M.im_inflate(fmt, src.ctypes.data if len(src) else None, len(src), out.ctypes.data if cap else None, cap, crc, res)
    return rc, out[:res[0]].tobytes(), int(res[0]), int(res[1]), int(res[4]), M.im_rule_name(int(res[2])).decode()


ZLIB_WAYS = ((9, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE))


def zlib_raw(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def zlib_in_used(stream):
    o = zlib.decompressobj(-15)
    o.decompress(stream + b"\x55" * 7)
    assert o.eof
    return len(stream) + 7 - len(o.unused_data)


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def valid_inputs(big=True):
    """name -> bytes: the golden samples, the edge / format / few-symbol inputs, sizes 0 and 1."""
    d = {"sample.xls": golden("sample.xls"), "sample.jpg": golden("sample.jpg"), "sample_pgm_100k.bin": golden("sample_pgm_100k.bin"), "size0": b"", "size1": b"Z"}
    d.update(edge_inputs())
    if big:
        d.update(few_symbol_inputs())
    return d


def valid_streams(big=True):
    """Yields (label, original bytes, raw Deflate stream): every input through the six zlib ways and the oracle's Deflate_Fixed / _0 / _1 / _2 / _3."""
    for name, data in valid_inputs(big).items():
        for lv, st in ZLIB_WAYS:
            yield "%s/zlib%d.%d" % (name, lv, st), data, zlib_raw(data, lv, st)
        for m in (6, 7, 8, 9, 10):
            rc, stream, _ = oracle_deflate(data, m)
            if rc == 0:
                yield "%s/oracle%d" % (name, m), data, stream


def damaged_corpus():
    """The 20 000 damaged streams of the issue, deterministic: list of (stream, cap)."""
    bases = []
    for name in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin"):
        d = golden(name)[:30000]
        for lv, st in ZLIB_WAYS:
            bases.append((zlib_raw(d, lv, st), 2 * len(d)))
    rng = np.random.default_rng(1)
    cases = []
    for k in range(20000):
        s, cap = bases[k % 18]
        kind = k % 4
        if kind == 3:
            cases.append((s[:int(rng.integers(0, len(s)))], cap))
            continue
        pos = int(rng.integers(0, min(len(s), 200))) if kind == 0 else int(rng.integers(0, len(s)))
        bit = int(rng.integers(0, 8))
        b = bytearray(s)
        b[pos] ^= 1 << bit
        cases.append((bytes(b), cap))
    return cases, [b[0] for b in bases]


def zlib_verdict(stream, cap):
    """-> ("accepted", bytes, in_used) | ("error",) | ("not_eof",) | ("over_cap",)"""
    o = zlib.decompressobj(-15)
    try:
        out = o.decompress(stream, cap + 1)
    except zlib.error:
        return ("error",)
    if not o.eof:
        return ("not_eof",) if len(out) <= cap else ("over_cap",)
    if len(out) > cap:
        return ("over_cap",)
    return ("accepted", out, len(stream) - len(o.unused_data))


def many_formats():
    """The four payloads of the reference's test/many_formats.zip kept under tests/golden: list of (name, format, payload, size, crc, sha256)."""
    with open(os.path.join(GOLDEN, "many_formats.json")) as f:
        meta = json.load(f)
    return [(e["file"], e["format"], golden(e["file"]), e["size"], int(e["crc32"], 16), e["sha256"]) for e in meta["entries"]]
