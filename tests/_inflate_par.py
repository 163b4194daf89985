"""Helpers of the parallel-Inflate tests: loader of the CPU model (tests/inflate_par/inflate_par_host.cpp = the whole pipeline of
zip-ada_amd/csrc/zada_inflate_par_logic.h with one lane), the 2 MiB corpus streams and the inputs the GPU tests and the finder census share."""
import ctypes
import os
import subprocess
import zlib

import numpy as np

import _inflate
from _common import ROOT, format_inputs, oracle_deflate, silesia_mix

_cache = {}
_DIR = os.path.join(ROOT, "tests", "inflate_par")
_SRC = os.path.join(_DIR, "inflate_par_host.cpp")
_MAIN = os.path.join(_DIR, "par_check_main.cpp")
_HDRS = [os.path.join(ROOT, "zip-ada_amd", "csrc", h) for h in ("zada_inflate_logic.h", "zada_inflate_par_logic.h")]
INFO = ("chunks", "live_chunks", "repairs", "scout_rounds", "marker_bytes", "fell_back", "reason", "streams")
REASONS = ("none", "damaged", "repairs", "single chunk", "format", "memory")
REPAIR_PCT = 25          # the default of "inflate_par_repair_pct" (profiles/inflate_par/NOTES.md says where it comes from)


def _stale(p, srcs):
    return not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(f) for f in srcs)


def build_model():
    p = os.path.join(_DIR, "libinflate_par_host.so")
    if _stale(p, [_SRC] + _HDRS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, _SRC], check=True)
    return p


def build_check_program():
    """The stand-alone program of the sanitizer test: the model and its own main, under ASan + UBSan."""
    p = os.path.join(_DIR, "par_check_asan")
    if _stale(p, [_SRC, _MAIN] + _HDRS):
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17", "-o", p,
                        _MAIN, _SRC], check=True)
    return p


def model():
    if "m" not in _cache:
        M = ctypes.CDLL(build_model())
        M.ipm_inflate.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_void_p, ctypes.c_void_p]
        M.ipm_census.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
        M.ipm_rule_name.restype = ctypes.c_char_p
        M.ipm_rule_name.argtypes = [ctypes.c_uint]
        _cache["m"] = M
    return _cache["m"]


def model_inflate_par(payload, cap, chunk_kib, fmt=8, crc=0xFFFFFFFF, repair_pct=REPAIR_PCT):
    """-> (rc, bytes, out_len, in_used, crc register, rule name, info dict).  Exact-size heap copies, as _inflate.model_inflate."""
    M = model()
    src = np.frombuffer(bytes(payload), dtype=np.uint8).copy() if len(payload) else np.zeros(0, np.uint8)
    out = np.empty(cap, dtype=np.uint8)
    res = (ctypes.c_uint64 * 6)()
    info = (ctypes.c_uint64 * 8)()
    rc = M.ipm_inflate(fmt, src.ctypes.data if len(src) else None, len(src), out.ctypes.data if cap else None, cap, crc, chunk_kib, repair_pct, res, info)
    d = {k: int(info[i]) for i, k in enumerate(INFO)}
    d["reason"] = REASONS[d["reason"]]
    return rc, out[:res[0]].tobytes(), int(res[0]), int(res[1]), int(res[4]), M.ipm_rule_name(int(res[2])).decode(), d


def census(stream, chunk_kib):
    """The finder on one valid stream: dict of blocks, dynamic (non-final dynamic blocks: what the finder looks for), chunks, found_true, false_positive,
    found_nothing."""
    src = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    out = (ctypes.c_uint64 * 8)()
    assert model().ipm_census(src.ctypes.data, len(src), chunk_kib, out) == 0
    return dict(zip(("blocks", "dynamic", "chunks", "found_true", "false_positive", "found_nothing"), (int(x) for x in out[:6])))


def corpus_2m():
    """The 2 MiB corpus input of the GPU tests and the census: silesia_mix version 2."""
    if "c2" not in _cache:
        _cache["c2"] = silesia_mix(2 << 20, version=2)
    return _cache["c2"]


def corpus_streams(methods=(8, 10), zlib_levels=(6, 9)):
    """(label, data, stream) of the 2 MiB corpus input through the oracle's methods and zlib's levels."""
    if ("cs", methods, zlib_levels) not in _cache:
        d = corpus_2m()
        out = []
        for m in methods:
            rc, s, _ = oracle_deflate(d, m)
            assert rc == 0
            out.append(("corpus_2m/oracle%d" % m, d, s))
        for lv in zlib_levels:
            out.append(("corpus_2m/zlib%d.0" % lv, d, _inflate.zlib_raw(d, lv, zlib.Z_DEFAULT_STRATEGY)))
        _cache[("cs", methods, zlib_levels)] = out
    return _cache[("cs", methods, zlib_levels)]


# the dynamic-block streams the GPU tests assert fell_back == 0 on: the CPU test holds the model to the same on them
NAMED_DYNAMIC = ("corpus_2m/oracle10", "corpus_2m/zlib9.0")


RUN_PIECE = 258          # bytes between two sync flushes of the run's stream


def marker_streams():
    """name -> (data, raw Deflate stream, whether any match can reach into an earlier chunk at 4 KiB chunks).
      period_32505 / 6 / 7: blocks of random bytes repeated at about the window's length, zlib 9: nearly every byte of a later chunk is a marker.
      run_300000: one byte 300 000 times, distance 1 and length 258 across every boundary.  zlib packs it into 308 bytes, a single chunk at any
        chunk size the knob allows; flushed (Z_SYNC_FLUSH, the window kept) every RUN_PIECE bytes it is 9 KiB of fixed and empty stored blocks.
      random_64k_x16: 64 KiB of random bytes sixteen times, zlib 9.  The period is twice Deflate's window of 32 KiB, so no match exists, the
        stream is stored blocks and no output byte is a marker: the record is asserted to say exactly that.
      random_16k_x64: the same with a period inside the window: copies of copies of the first 16 KiB through every chunk."""
    if "ms" not in _cache:
        f = format_inputs()
        d = {k: (f[k], _inflate.zlib_raw(f[k], 9, zlib.Z_DEFAULT_STRATEGY), True) for k in ("period_32505", "period_32506", "period_32507")}
        run = b"\x41" * 300000
        c = zlib.compressobj(9, zlib.DEFLATED, -15)
        s = b"".join(c.compress(run[i:i + RUN_PIECE]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(run), RUN_PIECE)) + c.flush()
        d["run_300000"] = (run, s, True)
        rnd = bytes(np.random.RandomState(9).randint(0, 256, 65536).astype(np.uint8))
        d["random_64k_x16"] = (rnd * 16, _inflate.zlib_raw(rnd * 16, 9, zlib.Z_DEFAULT_STRATEGY), False)
        d["random_16k_x64"] = (rnd[:16384] * 64, _inflate.zlib_raw(rnd[:16384] * 64, 9, zlib.Z_DEFAULT_STRATEGY), True)
        _cache["ms"] = d
    return _cache["ms"]


def planted_false_positive():
    """A level-0 (stored) stream whose payload is a zlib-9 stream of 256 KiB of text: the inner stream's dynamic headers lie byte-aligned inside
    stored blocks, where no block starts.  -> (data = the inner stream, the outer stream)"""
    inner = _inflate.zlib_raw(silesia_mix(256 << 10, class_mask=1), 9, zlib.Z_DEFAULT_STRATEGY)
    return inner, _inflate.zlib_raw(inner, 0, zlib.Z_DEFAULT_STRATEGY)
