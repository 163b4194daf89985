"""The Inflate decoder (zip-ada_amd/csrc/zada_inflate_logic.h) as a CPU model, against zlib: valid streams, 20 000 damaged ones, the reference's
own Deflate / Deflate64 fixtures and Deflate64 streams no zlib can make -- and the same once more under ASan + UBSan.  No GPU."""
import hashlib
import os
import subprocess
import sys
import zlib

import pytest

from _common import ROOT
import _inflate
from _inflate import E_DATA, model_inflate


def _check_valid(label, data, stream, M=None):
    rc, out, ol, used, crc, rule = model_inflate(stream, len(data), 8, M=M)
    assert rc == 0, (label, rule)
    assert out == data and ol == len(data), label
    iu = _inflate.zlib_in_used(stream)
    assert used == iu, label
    assert crc ^ 0xFFFFFFFF == zlib.crc32(data), label
    # trailing bytes are not an error, a larger cap neither; one byte less of cap is
    rc, out, ol, used, _, _ = model_inflate(stream + b"\x55" * 7, len(data) + 5, 8, M=M)
    assert (rc, out, used) == (0, data, iu), label
    if len(data):
        assert model_inflate(stream, len(data) - 1, 8, M=M)[0] == E_DATA, label


def test_valid_streams():
    n = 0
    for label, data, stream in _inflate.valid_streams():
        _check_valid(label, data, stream)
        n += 1
    assert n > 500


def test_empty_input_and_empty_entry():
    assert model_inflate(b"", 10)[0] == E_DATA
    assert model_inflate(b"", 0)[0] == E_DATA
    assert model_inflate(b"\x03\x00", 0)[:4] == (0, b"", 0, 2)          # what zlib writes for no bytes: an empty fixed block
    assert model_inflate(b"\x01\x00\x00\xff\xff", 0)[:4] == (0, b"", 0, 5)


def run_damaged(M=None, counts=None):
    cases, _ = _inflate.damaged_corpus()
    assert len(cases) == 20000
    counts = counts if counts is not None else {}
    for k, (s, cap) in enumerate(cases):
        v = _inflate.zlib_verdict(s, cap)
        counts[v[0]] = counts.get(v[0], 0) + 1
        rc, out, ol, used, _, rule = model_inflate(s, cap, 8, M=M)
        if v[0] == "accepted":
            assert rc == 0, (k, rule)
            assert out == v[1] and ol == len(v[1]) and used == v[2], k
        else:
            assert rc == E_DATA, (k, v[0], rc, ol)
    return counts


def test_damaged_streams_follow_zlib():
    counts = run_damaged()
    print(counts)
    for kind in ("accepted", "error", "not_eof"):
        assert counts.get(kind, 0) >= 1000, counts


def test_reference_fixtures():
    for name, fmt, payload, size, crc, sha in _inflate.many_formats():
        rc, out, ol, used, reg, rule = model_inflate(payload, size, fmt)
        assert rc == 0 and ol == size and used == len(payload), (name, rule)
        assert hashlib.sha256(out).hexdigest() == sha and reg ^ 0xFFFFFFFF == crc, name
        if fmt == 8:
            assert zlib.decompress(payload, -15) == out


# ---- a fixed-block Deflate64 writer: token lists -> streams no zlib can make ----
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227]
_LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5]


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):                      # k bits of v, least significant first
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, k):                     # a Huffman code: most significant bit first
        self.put(int(format(v, "0%db" % k)[::-1], 2), k)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def _litlen(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def deflate64_fixed(tokens):
    """tokens: ints (literals) and (length, distance) pairs -> (one final fixed block, its expansion)."""
    w, out = _Bits(), bytearray()
    w.put(1, 1)
    w.put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            _litlen(w, t)
            out.append(t)
            continue
        ln, d = t
        if ln <= 258:
            c = max(i for i in range(28) if _LBASE[i] <= ln)
            _litlen(w, 257 + c)
            w.put(ln - _LBASE[c], _LEXTRA[c])
        else:
            _litlen(w, 285)
            w.put(ln - 3, 16)
        dc = d - 1 if d <= 4 else max(c for c in range(4, 32) if 1 + ((2 + (c & 1)) << ((c >> 1) - 1)) <= d)
        w.code(dc, 5)
        if dc >= 4:
            e = (dc >> 1) - 1
            w.put(d - (1 + ((2 + (dc & 1)) << e)), e)
        for _ in range(ln):
            out.append(out[-d])
    _litlen(w, 256)
    return w.done(), bytes(out)


def deflate64_cases():
    """name -> (token list, uses a distance code 30 / 31)"""
    import numpy as np
    head = [int(x) for x in np.random.RandomState(3).randint(0, 256, 70000)]
    c = {}
    c["short"] = ([65, 66, 67, (3, 3), (258, 1), (259, 2), (65538, 5), 90], False)
    c["lengths"] = (head[:300] + [(n, 7 + n % 250) for n in (3, 4, 10, 11, 257, 258, 259, 260, 1000, 65537, 65538)], False)
    c["dist_32768"] = (head[:33000] + [(5, 32768), (300, 32768), (40000, 32768)], False)
    c["dist_32769"] = (head[:33000] + [(5, 32769), (259, 32769)], True)
    c["dist_65536"] = (head[:66000] + [(3, 65536), (65538, 65536), (9, 49153), (9, 49152), (100, 1)], True)
    c["overlap"] = ([1, 2, 3, 4, 5] + [(ln, d) for d in (1, 2, 3, 5) for ln in (3, 64, 65, 300, 4097)], False)
    return c


def test_deflate64_streams_no_zlib_can_make():
    for name, (tokens, far) in deflate64_cases().items():
        stream, want = deflate64_fixed(tokens)
        rc, out, ol, used, crc, rule = model_inflate(stream, len(want), 9)
        assert rc == 0 and out == want and used == len(stream), (name, rule)
        assert crc ^ 0xFFFFFFFF == zlib.crc32(want)
        if far:
            assert model_inflate(stream, len(want), 8)[0] == E_DATA, name
        assert model_inflate(stream, len(want) - 1, 9)[0] == E_DATA, name
        assert model_inflate(stream[:-1], len(want), 9)[0] == E_DATA, name


def test_deflate64_first_distance_beyond_output_is_an_error():
    stream, _ = deflate64_fixed([1, 2, 3])
    bad, _ = deflate64_fixed([1, 2, 3, (3, 3)])
    assert model_inflate(bad, 100, 9)[0] == 0
    w = _Bits()
    w.put(1, 1); w.put(1, 2)
    _litlen(w, 65); _litlen(w, 257); w.code(1, 5); _litlen(w, 256)       # distance 2 after one byte
    assert model_inflate(w.done(), 100, 9)[0] == E_DATA
    assert model_inflate(w.done(), 100, 8)[0] == E_DATA


ASAN_DRIVER = r'''
import os, sys
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import _inflate, test_inflate_model as t
M = _inflate.load_model(%(lib)r)
n = 0
for label, data, stream in _inflate.valid_streams(big=False):
    if len(data) <= 400000:
        t._check_valid(label, data, stream, M=M); n += 1
counts = t.run_damaged(M=M)
for name, fmt, payload, size, crc, sha in _inflate.many_formats():
    assert _inflate.model_inflate(payload, size, fmt, M=M)[0] == 0
for name, (tokens, far) in t.deflate64_cases().items():
    stream, want = t.deflate64_fixed(tokens)
    assert _inflate.model_inflate(stream, len(want), 9, M=M)[:2] == (0, want)
    assert _inflate.model_inflate(stream, len(want) // 2, 9, M=M)[0] == -7
print("asan ok", n, counts)
'''


def test_model_is_clean_under_asan_and_ubsan():
    lib = _inflate.build_model(asan=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True, check=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=" ".join(x for x in (libasan, os.environ.get("LD_PRELOAD", "")) if x), ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([sys.executable, "-c", ASAN_DRIVER % {"root": ROOT, "lib": lib}], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "asan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
