"""The BZip2 decoder (zip-ada_amd/csrc/zada_bunzip2_logic.h) as a CPU model with serial later stages, against libbz2 (bz2.BZ2Decompressor, one
stream): valid streams of five writers, 20 000 damaged ones, the reference's own BZip2 entry and crafted blocks no writer makes -- and the same
once more under ASan + UBSan.  No GPU."""
import bz2
import hashlib
import os
import subprocess
import sys
import zlib

from _common import ROOT
import _bunzip2
from _bunzip2 import E_DATA, model_bunzip2


def _check_valid(label, data, stream, M=None):
    v = _bunzip2.bz2_verdict(stream, len(data) if data is not None else 1 << 20)
    assert v[0] == "accepted", label
    if data is not None:
        assert v[1] == data, label
    data = v[1]
    rc, out, ol, used, crc, rule = model_bunzip2(stream, len(data), M=M)
    assert rc == 0, (label, rule)
    assert out == data and ol == len(data), label
    assert used == v[2] == len(stream), label
    assert crc ^ 0xFFFFFFFF == zlib.crc32(data), label
    # trailing bytes are not an error (only the first stream of a concatenation is decoded), a larger cap neither; one byte less of cap is
    rc, out, ol, used, _, _ = model_bunzip2(stream + b"\x55\x00\xaa", len(data) + 5, M=M)
    assert (rc, out, used) == (0, data, len(stream)), label
    if len(data):
        r = model_bunzip2(stream, len(data) - 1, M=M)
        assert r[0] == E_DATA and r[5] == "output beyond cap", label


def test_valid_streams():
    n = 0
    for label, data, stream in _bunzip2.valid_streams():
        _check_valid(label, data, stream)
        n += 1
    assert n > 350


def test_three_blocks_off_byte_boundaries():
    d = _bunzip2.three_blocks()
    s = bz2.compress(d, 1)
    r = model_bunzip2(s, len(d), records=8)
    assert r[0] == 0 and r[1] == d and len(r[6]) == 3
    assert any(int(end) % 8 for _, _, _, end in r[6])
    assert sum(int(n) for n, _, _, _ in r[6]) >= len(d)
    two = model_bunzip2(s + s, 2 * len(d))                    # a concatenation: the first stream only
    assert two[:4] == (0, d, len(d), len(s))


def test_reference_payload():
    p, size, crc, sha = _bunzip2.reference_payload()
    assert len(p) == 22176 and size == 81682 and crc == 0x840ff735
    rc, out, ol, used, reg, rule = model_bunzip2(p, size)
    assert rc == 0 and ol == size and used == len(p), rule
    assert hashlib.sha256(out).hexdigest() == sha and reg ^ 0xFFFFFFFF == crc


def test_empty_and_short_input():
    for cap in (0, 10):
        assert model_bunzip2(b"", cap)[0::5] == (E_DATA, "input exhausted")
    s = bz2.compress(b"")
    assert len(s) == 14 and model_bunzip2(s, 0)[:4] == (0, b"", 0, 14)
    for k in range(14):
        assert model_bunzip2(s[:k], 10)[0::5] == (E_DATA, "input exhausted"), k
    assert model_bunzip2(b"BZh0" + s[4:], 0)[5] == "no BZh1 .. BZh9 stream header"
    assert model_bunzip2(b"BZh9" + b"\x00" * 20, 10)[5] == "neither block nor footer magic"


def test_the_reference_writers_empty_block_is_refused_as_libbz2_refuses_it():
    for s in _bunzip2.empty_block_streams():
        assert _bunzip2.bz2_verdict(s, 10)[0] == "error"
        assert model_bunzip2(s, 10)[0::5] == (E_DATA, "mapping table names no byte value")


def run_damaged(M=None, counts=None):
    cases, _ = _bunzip2.damaged_corpus()
    assert len(cases) == 20000
    counts = counts if counts is not None else {}
    for k, (s, cap, kind) in enumerate(cases):
        v = _bunzip2.bz2_verdict(s, cap)
        counts[v[0]] = counts.get(v[0], 0) + 1
        rc, out, ol, used, _, rule = model_bunzip2(s, cap, M=M)
        if v[0] == "accepted":
            assert rc == 0, (k, rule)
            assert out == v[1] and ol == len(v[1]) and used == v[2], k
        else:
            assert rc == E_DATA, (k, v[0], rc, ol)
        if kind == 3:
            assert rule == "input exhausted", (k, rule)
    return counts


def test_damaged_streams_follow_libbz2():
    counts = run_damaged()
    print(counts)
    # (libbz2's two CRCs leave a flipped bit next to no chance: the corpus is about the rejections)
    assert counts.get("error", 0) >= 10000 and counts.get("not_eof", 0) >= 5000 and sum(counts.values()) == 20000, counts


def check_crafted(M=None):
    cases = _bunzip2.crafted_cases()
    assert len(cases) == 8
    for name, (stream, expect, rule) in cases.items():
        v = _bunzip2.bz2_verdict(stream, 1 << 20)
        r = model_bunzip2(stream, 1 << 20, M=M)
        if expect is None:
            assert v[0] == "error" and r[0] == E_DATA and r[5] == rule, (name, v[0], r[5])
        else:
            assert v[0] == "accepted" and v[1] == expect, name
            assert r[0] == 0 and r[1] == expect and r[3] == v[2], (name, r[5])
    # (a) is what it says: the serial reading of its block goes round a cycle shorter than the block
    s, exp, _ = cases["a_cycles"]
    assert len(set(exp)) > 1 and any(exp[:p] * (len(exp) // p) == exp[:p * (len(exp) // p)] for p in range(1, 1500))
    # (b): the magic really is in the coded data, where the helper says
    for shift in (0, 3, 7):
        s, exp, at = _bunzip2.magic_inside_block(shift)
        assert (int.from_bytes(s, "big") >> (len(s) * 8 - at - 48)) & ((1 << 48) - 1) == _bunzip2.BLOCK_MAGIC and at % 8 == (at - 9 * shift + shift) % 8


def test_crafted_blocks():
    check_crafted()


def test_model_is_clean_under_asan_and_ubsan():
    """The valid streams (every third), the crafted blocks and the whole damaged corpus once more in a child process whose model is built with
    -fsanitize=address,undefined: every buffer the model reads or writes is an exact-size heap block."""
    lib = _bunzip2.build_model(asan=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True, check=True).stdout.strip()
    code = ("import sys; sys.path.insert(0, %r); import _bunzip2, test_bunzip2_model as t; M = _bunzip2.load_model(%r)\n"
            "for k, (label, data, stream) in enumerate(_bunzip2.valid_streams()):\n"
            "    if k %% 3 == 0: t._check_valid(label, data, stream, M)\n"
            "t.check_crafted(M); print(t.run_damaged(M)); print('asan ok')\n") % (os.path.join(ROOT, "tests"), lib)
    env = dict(os.environ, LD_PRELOAD=" ".join(x for x in (libasan, os.environ.get("LD_PRELOAD", "")) if x), ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "asan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
