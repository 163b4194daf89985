"""Helpers of the Trained_Compression tests: the reference's data files (tests/golden/trained), the oracle's three calls (stub, whole stream, message),
liblzma's verdict on a stream with the 5-byte header, and the loader of the CPU model of the forked decoder (tests/trained/trained_host.cpp =
zip-ada_amd/csrc/zada_unlzma_logic.h with one lane, stopped at a symbol boundary and started again from the state it left)."""
import ctypes
import os
import subprocess

import numpy as np

from _common import GOLDEN, ROOT

E_DATA = -7
DICT = 1 << 19                                         # TC_dictionary_size, trained_compression.adb
MARGIN = 140                                           # trtest_single.cmd: skip = the stub's length less this
FORK_MARGIN = 64                                       # ULZ_FORK_MARGIN, zada_unlzma_logic.h
KEEP_AFTER = 4369                                      # BT4_OPTS + BT4_LOOK, zada_bt4.h: the matcher's look-ahead
PAIRS = (("gs1.xls", "gs2.xls"), ("gs1.xls", "gs3.xls"), ("wsbase.csv", "wm1ns.csv"), ("wsbase.csv", "wm2ns.csv"))
_cache = {}
_DIR = os.path.join(ROOT, "tests", "trained")
_SRC = os.path.join(_DIR, "trained_host.cpp")
_HDR = os.path.join(ROOT, "zip-ada_amd", "csrc", "zada_unlzma_logic.h")


def fixture(name):
    if ("f", name) not in _cache:
        with open(os.path.join(GOLDEN, "trained", name), "rb") as f:
            _cache["f", name] = f.read()
    return _cache["f", name]


def tc_stream(text, end_marker=True):
    """LZMA.Encoding.Encode as Trained_Compression calls it (Level_3, 3 / 0 / 2, dictionary 2 ** 19), by the oracle; cached."""
    from _lzmah import oracle_lzma_encode
    key = ("s", bytes(text), end_marker)
    if key not in _cache:
        _cache[key] = oracle_lzma_encode(bytes(text), 3, 3, 0, 2, end_marker=end_marker, dictionary_size=DICT)[0]
    return _cache[key]


def stub_of(trainer):
    return tc_stream(trainer, False)


def message_of(trainer, data, skip):
    return tc_stream(bytes(trainer) + bytes(data))[skip:]


def common_prefix(a, b):
    n = min(len(a), len(b))
    x = np.frombuffer(a, np.uint8, n) != np.frombuffer(b, np.uint8, n)
    return int(np.argmax(x)) if x.any() else n


def fixture_cases():
    """(label, trainer, data, stub, skip = len (stub) - 140, whole stream) for the four pairs, with and without the ten noise bytes."""
    out = []
    for noise in (fixture("rnd_10.bin"), b""):
        for t, d in PAIRS:
            trainer = fixture(t) + noise
            stub = stub_of(trainer)
            out.append(("%s+%s%s" % (t, d, "+noise" if noise else ""), trainer, fixture(d), stub, max(0, len(stub) - MARGIN), tc_stream(trainer + fixture(d))))
    return out


def liblzma_verdict(stream, cap):
    """liblzma on a stream with the 5-byte header that ends on its marker -> ("accepted", bytes, in_used) | ("error",) | ("not_eof",) | ("over_cap",)"""
    from _unlzma import lzma_verdict
    v = lzma_verdict(b"\x09\x04\x05\x00" + bytes(stream), cap, True)
    return ("accepted", v[1], v[2] - 4) if v[0] == "accepted" else v


def build_model():
    p = os.path.join(_DIR, "libtrained_host.so")
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, _SRC], check=True)
    return p


def build_check():
    """The checker as a program of its own, under AddressSanitizer + UBSan."""
    p = os.path.join(_DIR, "trained_check_asan")
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DTRAINED_MAIN",
                        "-o", p, _SRC], check=True)
    return p


def model():
    if "m" not in _cache:
        M = ctypes.CDLL(build_model())
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        M.tm_decode.argtypes = [vp, u64, vp, u64, u32, vp]
        M.tm_decode_forked.argtypes = [vp, u64, vp, u64, u32, u64, u64, vp, vp]
        M.tm_rule_name.restype = ctypes.c_char_p
        M.tm_rule_name.argtypes = [ctypes.c_uint]
        M.tm_fork_margin.restype = u64
        _cache["m"] = M
    return _cache["m"]


NONE = 0xFFFFFFFFFFFFFFFF


def model_decode(stream, cap, in_limit=None, symbols=None):
    """One piece (no limit given) or stopped and started again -> ((rc, bytes, in_used, rule name, input byte, output position, end), fork) with
    fork = (input bytes taken, bytes written) at the boundary, or None when the decoder did not stop."""
    M = model()
    src = np.frombuffer(bytes(stream), dtype=np.uint8).copy() if len(stream) else np.zeros(0, np.uint8)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    res, f3 = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 3)()
    p = src.ctypes.data if len(src) else None
    if in_limit is None and symbols is None:
        rc = M.tm_decode(p, len(src), out.ctypes.data, cap, 1, res)
    else:
        rc = M.tm_decode_forked(p, len(src), out.ctypes.data, cap, 1, NONE if in_limit is None else in_limit, NONE if symbols is None else symbols, res, f3)
    rec = (rc, out[:res[0]].tobytes(), int(res[1]), M.tm_rule_name(int(res[2])).decode(), int(res[3]), int(res[5]), int(res[6]))
    return rec, ((int(f3[0]), int(f3[1])) if f3[2] else None)


def damaged_messages(count=2000, seed=21):
    """(stub part, message, cap, kind): messages of three small trainer / data pairs, one byte flipped or truncated at a seeded place."""
    key = ("dmg", count, seed)
    if key in _cache:
        return _cache[key]
    bases = []
    for t, d, tl, dl in (("gs1.xls", "gs2.xls", 9000, 2500), ("wsbase.csv", "wm1ns.csv", 7000, 3000), ("wsbase.csv", "wm2ns.csv", 5000, 600)):
        trainer, data = fixture(t)[:tl], fixture(d)[1000:1000 + dl]
        stub = stub_of(trainer)
        skip = max(0, len(stub) - MARGIN)
        bases.append((stub[:skip], message_of(trainer, data, skip), tl + dl))
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(count):
        head, msg, cap = bases[k % len(bases)]
        b = bytearray(msg)
        if k % 2 == 0:
            b[int(rng.integers(0, len(b)))] ^= int(rng.integers(1, 256))
        else:
            b = b[:int(rng.integers(0, len(b)))]
        cases.append((head, bytes(b), cap, k % 2))
    _cache[key] = cases
    return cases
