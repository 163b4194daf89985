"""Helpers of the tests of the parallel Inflate on Deflate64 streams: loader of the CPU model (tests/inflate_par/inflate_par64_host.cpp = the
format 9 pipeline of zip-ada_amd/csrc/zada_inflate_par_logic.h with one lane).  The streams come from _deflate64.py."""
import ctypes
import os
import subprocess

import numpy as np

from _common import ROOT
from _inflate_par import INFO, REASONS, REPAIR_PCT, _stale

_cache = {}
_DIR = os.path.join(ROOT, "tests", "inflate_par")
_SRC = os.path.join(_DIR, "inflate_par64_host.cpp")
_MAIN = os.path.join(_DIR, "par64_check_main.cpp")
_HDRS = [os.path.join(ROOT, "zip-ada_amd", "csrc", h) for h in ("zada_inflate_logic.h", "zada_inflate_par_logic.h")]
CHUNKS_KIB = (4, 16)      # the chunk sizes the CPU and the GPU test assert the record at


def build_model():
    p = os.path.join(_DIR, "libinflate_par64_host.so")
    if _stale(p, [_SRC] + _HDRS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, _SRC], check=True)
    return p


def build_check_program():
    """The stand-alone program of the sanitizer test: the model and its own main, under ASan + UBSan."""
    p = os.path.join(_DIR, "par64_check_asan")
    if _stale(p, [_SRC, _MAIN] + _HDRS):
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17", "-o", p,
                        _MAIN, _SRC], check=True)
    return p


def model():
    if "m" not in _cache:
        M = ctypes.CDLL(build_model())
        M.ipm64_inflate.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                    ctypes.c_void_p, ctypes.c_void_p]
        M.ipm64_census.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
        M.ipm64_rule_name.restype = ctypes.c_char_p
        M.ipm64_rule_name.argtypes = [ctypes.c_uint]
        M.ipm64_last_live.restype = ctypes.c_uint64
        M.ipm64_last_live.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        _cache["m"] = M
    return _cache["m"]


def model_inflate_par64(payload, cap, chunk_kib, crc=0xFFFFFFFF, repair_pct=REPAIR_PCT):
    """-> (rc, bytes, out_len, in_used, crc register, rule name, info dict) as _inflate_par.model_inflate_par; info ["live_bytes"]: the output bytes
    of every live chunk, in order, where the stream ran in parallel."""
    M = model()
    src = np.frombuffer(bytes(payload), dtype=np.uint8).copy() if len(payload) else np.zeros(0, np.uint8)
    out = np.empty(cap, dtype=np.uint8)
    res = (ctypes.c_uint64 * 6)()
    info = (ctypes.c_uint64 * 8)()
    rc = M.ipm64_inflate(9, src.ctypes.data if len(src) else None, len(src), out.ctypes.data if cap else None, cap, crc, chunk_kib, repair_pct, res, info)
    d = {k: int(info[i]) for i, k in enumerate(INFO)}
    d["reason"] = REASONS[d["reason"]]
    if not d["fell_back"]:
        live = (ctypes.c_uint64 * max(d["live_chunks"], 1))()
        assert M.ipm64_last_live(live, d["live_chunks"]) == d["live_chunks"]
        d["live_bytes"] = [int(x) for x in live[:d["live_chunks"]]]
    return rc, out[:res[0]].tobytes(), int(res[0]), int(res[1]), int(res[4]), M.ipm64_rule_name(int(res[2])).decode(), d


def census(stream, chunk_kib):
    """The finder on one valid stream, as _inflate_par.census."""
    src = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    out = (ctypes.c_uint64 * 8)()
    assert model().ipm64_census(src.ctypes.data, len(src), chunk_kib, out) == 0
    return dict(zip(("blocks", "dynamic", "chunks", "found_true", "false_positive", "found_nothing"), (int(x) for x in out[:6])))
