"""Loader of the Shrink and Reduce CPU models (tests/legacy/shrink_model.c, reduce_model.c), compiled on first use into git-ignored
libraries the way _rich.model() builds its own, and the inputs the CPU and GPU tests of these methods share."""
import ctypes
import os
import random
import subprocess

import numpy as np

from _common import ROOT

DIR = os.path.join(ROOT, "tests", "legacy")
SHRINK_CENSUS = ("clears", "rises", "dup_adds", "add_under_freed", "alloc_with_child", "unreachable", "full_nonliteral")
REDUCE_CENSUS = ("lit144", "expanded", "two_byte", "slen0", "slen2", "slen4", "slen8", "slen16", "slen32")
LOOK_AHEAD = {1: 31, 2: 63, 3: 255, 4: 191}
_cache = {}
U64P = ctypes.POINTER(ctypes.c_uint64)


def _lib(name):
    if name not in _cache:
        src = os.path.join(DIR, name + ".c")
        p = os.path.join(DIR, "lib" + name + ".so")
        if not os.path.exists(p) or os.path.getmtime(p) < os.path.getmtime(src):
            subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", p, src], check=True)
        _cache[name] = ctypes.CDLL(p)
    return _cache[name]


def shrink_lib():
    M = _lib("shrink_model")
    for f in (M.shrink_stated, M.shrink_closed):
        f.restype = ctypes.c_uint64
        f.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, U64P]
    M.shrink_decode.restype = ctypes.c_int64
    M.shrink_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    M.shrink_selftest.argtypes = [ctypes.c_uint32, ctypes.c_int, U64P]
    return M


def reduce_lib():
    M = _lib("reduce_model")
    for f in (M.reduce_stated, M.reduce_closed):
        f.restype = ctypes.c_uint64
        f.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, U64P,
                      ctypes.c_void_p, ctypes.c_void_p, U64P]
    M.reduce_decode.restype = ctypes.c_int64
    M.reduce_decode.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    M.reduce_selftest.argtypes = [ctypes.c_uint32, ctypes.c_int, U64P]
    return M


def shrink(data, stated=False):
    """(stream, census) of the closed form (the kernel's), or of the stated form."""
    data = bytes(data)
    M = shrink_lib()
    cap = 5 * len(data) + 64
    out = ctypes.create_string_buffer(cap)
    cs = (ctypes.c_uint64 * len(SHRINK_CENSUS))()
    k = (M.shrink_stated if stated else M.shrink_closed)(data, len(data), out, cap, cs)
    assert k <= cap
    return out.raw[:k], dict(zip(SHRINK_CENSUS, cs))


def unshrink(stream, n):
    out = ctypes.create_string_buffer(n + 1)
    k = shrink_lib().shrink_decode(bytes(stream), len(stream), out, n)
    return None if k < 0 else out.raw[:k]


def reduce(data, factor, stated=False):
    """(stream, raw bytes, Slen [256], followers [256, 32], census) of the closed form (the kernels'), or of the stated form."""
    data = bytes(data)
    M = reduce_lib()
    rcap = 2 * len(data) + 16
    cap = rcap + rcap // 8 + 8500
    out, raw = ctypes.create_string_buffer(cap), ctypes.create_string_buffer(rcap)
    slen, foll = np.zeros(256, dtype=np.uint8), np.zeros((256, 32), dtype=np.uint8)
    cs = (ctypes.c_uint64 * len(REDUCE_CENSUS))()
    rl = ctypes.c_uint64(0)
    k = (M.reduce_stated if stated else M.reduce_closed)(factor, data, len(data), out, cap, raw, rcap, ctypes.byref(rl), slen.ctypes.data, foll.ctypes.data, cs)
    assert k <= cap and rl.value <= rcap
    return out.raw[:k], raw.raw[:rl.value], slen, foll, dict(zip(REDUCE_CENSUS, cs))


def unreduce(stream, factor, n):
    out = ctypes.create_string_buffer(n + 1)
    k = reduce_lib().reduce_decode(factor, bytes(stream), len(stream), out, n)
    return None if k < 0 else out.raw[:k]


def followers_in_use(slen, foll):
    """The followers a stream carries: row x counts only up to Slen [x]."""
    return [bytes(foll[x, :slen[x]]) for x in range(256)]


def model_result(data, method):
    """(rc, stream, running CRC register from 0xFFFFFFFF) the device calls must give for method 1 (Shrink) or 2 .. 5 (Reduce)."""
    import zlib
    s = shrink(data)[0] if method == 1 else reduce(data, method - 1)[0]
    return (1 if len(s) >= len(data) else 0), s, zlib.crc32(bytes(data)) ^ 0xFFFFFFFF


# ---- the inputs the tests share ---------------------------------------------------------------------------------------------
def rnd(seed, n, alphabet):
    return bytes(random.Random(seed).choices(alphabet, k=n))


def shrink_inputs():
    """name -> bytes: the compressible ones reach partial clears, code-size rises and duplicate adds after a clear."""
    if "si" not in _cache:
        _cache["si"] = {
            "abcd_48k": rnd(1, 48 << 10, b"abcd"),
            "abcd_128k": rnd(1, 128 << 10, b"abcd"),
            "sym16_96k": rnd(3, 96 << 10, bytes(range(65, 81))),
            "random_16k": rnd(4, 16 << 10, bytes(range(256))),
        }
    return _cache["si"]


def reduce_inputs():
    if "ri" not in _cache:
        r = random.Random(5)
        words = [bytes(r.choices(b"ab\x90 e", k=r.randint(2, 9))) for _ in range(60)]
        text = b""
        while len(text) < 24 << 10:
            text += r.choice(words) + b" "
        block = rnd(6, 3000, bytes(range(256)))
        big = bytearray()
        r2 = random.Random(7)
        while len(big) < 400 << 10:                      # poorly compressible: the raw stream passes 256 KiB
            big += bytes(r2.choices(bytes(range(256)), k=r2.randint(200, 900))) + bytes(big[-r2.randint(5, 40):]) * 2
        _cache["ri"] = {
            "words_24k": text[:24 << 10],
            "runs_A_90": (700 * b"A" + 50 * b"\x90" + b"xyz") * 12,
            "far_repeats": (block + b"0123456789" * 3) * 4,
            "abcd_12k": rnd(8, 12 << 10, b"abcd"),
            "big_400k": bytes(big[:400 << 10]),
        }
    return _cache["ri"]


def edge_sizes(factor=None):
    la = sorted(LOOK_AHEAD.values()) if factor is None else [LOOK_AHEAD[factor]]
    s = {0, 1, 2, 4095, 4096, 4097}
    for f in la:
        s |= {f - 1, f, f + 1, 4096 + f}
    return sorted(s)


def edge_input(n, seed=11):
    """n bytes with matches and 144s in them."""
    r = random.Random(seed * 100003 + n)
    out = bytearray()
    while len(out) < n:
        out += bytes(r.choices(b"abc\x90", k=r.randint(1, 40))) * r.randint(1, 3)
    return bytes(out[:n])


def batch_inputs(count=300, seed=12):
    r = random.Random(seed)
    res = []
    for i in range(count):
        n = r.choice((0, 1, 5, 700)) if i % 10 == 0 else r.randint(0, 9000)
        res.append(edge_input(n, seed=i) if i % 3 else rnd(i, n, bytes(range(256))))
    return res


# ---- what the GPU tests hand the device, by helper: test_legacy_model.py holds stated form = closed form on every one of them -----------
def contract_input(method):
    """The input of the 256 alignments of the _device calls (Reduce: short, one wave walks the matcher's tree byte after byte)."""
    return edge_input(5000 if method == 1 else 1000)


def contract_small_inputs(method):
    """Small entries the _device calls take with cap = n."""
    return [edge_input(n) for n in ((0, 1, 2, 31, 4097) if method == 1 else (0, 1, 2, 191, 4097))]


def contract_random_input():
    return shrink_inputs()["random_16k"][:3000]


def batch_contract_inputs(method):
    """The entries of the guarded arena of the _batch calls: compressible ones, an empty one, one byte, and random bytes."""
    if method == 1:
        return [edge_input(n, seed=3) for n in (5000, 300, 0, 4097, 1, 2500)] + [shrink_inputs()["random_16k"][:2000]]
    return [edge_input(n, seed=3) for n in (5000, 600, 0, 4097, 1, 2500)] + [rnd(9, 2000, bytes(range(256)))]


def zip_inputs():
    """The entries of the Compress_Data and ZipCreate tests, under every method."""
    return [edge_input(3000), reduce_inputs()["runs_A_90"], rnd(21, 1500, bytes(range(256))), b"", b"q", shrink_inputs()["abcd_48k"][:20000]]


def gpu_test_inputs(method):
    """Every input a GPU test hands the device under `method` (1 Shrink_1, 2 .. 5 Reduce_1 .. _4), without repeats."""
    if method == 1:
        ins = [edge_input(n) for n in edge_sizes()] + list(shrink_inputs().values()) + [contract_random_input()] + batch_inputs()
    else:
        ins = [edge_input(n) for n in edge_sizes(method - 1)] + list(reduce_inputs().values())
    ins += [contract_input(method)] + zip_inputs()
    if method in (1, 5):                                   # (the small _device entries and the batches run under Shrink_1 and Reduce_4)
        ins += contract_small_inputs(method) + batch_contract_inputs(method)
    if method == 5:
        ins += batch_inputs()
    seen, out = set(), []
    for d in ins:
        if d not in seen:
            seen.add(d)
            out.append(d)
    return out
