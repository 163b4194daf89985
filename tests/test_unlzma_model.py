"""The LZMA reader's decoder logic (zip-ada_amd/csrc/zada_unlzma_logic.h) compiled for the CPU with one lane (tests/unlzma/unlzma_host.cpp): the bytes of
valid streams, liblzma's verdict, bytes and input count on 20 000 damaged cases, the verdicts of the reference's rules on crafted streams, and the
whole corpus again under AddressSanitizer + UBSan with exact-size heap buffers.

liblzma writes and reads lc + lp <= 4 only.  The parameter sets (8, 0, 2) and (4, 4, 4), and the reference's methods with lc = 8, are therefore
written by the oracle's LZMA.Encoding; for them the yardstick is the input's bytes, and the input count is the payload's length less the at most
four bytes of the range coder's flush that no normalisation asks for."""
import hashlib
import os
import subprocess
import sys
import zlib

import pytest

import _unlzma
from _common import ROOT
from _unlzma import E_DATA, END_MARKER, END_NO_MARKER, lzma_verdict, model_unlzma


@pytest.fixture(scope="module")
def streams():
    return _unlzma.cached_valid_streams()


def test_valid_streams(streams):
    wide, early = 0, []
    assert len(streams) > 3000
    for k, (label, data, payload, eos) in enumerate(streams):
        cap = len(data)
        rc, out, ol, used, reg, rule, rec = model_unlzma(payload, cap, eos)
        assert rc == 0 and out == data and reg ^ 0xFFFFFFFF == zlib.crc32(data), (label, rule)
        assert rec[3] == (END_MARKER if eos else END_NO_MARKER), label
        v = lzma_verdict(payload, cap, eos)
        if v[0] == "unsupported":
            wide += 1
            assert len(payload) - 4 <= used <= len(payload), label
        else:
            assert v == ("accepted", data, used), (label, v[0], used)
        # three trailing bytes are not an error and are not counted
        if k % 3 == 0 or len(data) < 300:
            m3 = model_unlzma(payload + b"\x00\xff\x31", cap, eos)
            assert m3[:4] == (0, data, ol, used), label
            v3 = lzma_verdict(payload + b"\x00\xff\x31", cap, eos)
            assert v3[0] == "unsupported" or v3 == ("accepted", data, used), label
        # one byte less of cap: the output rule.  A stream WITHOUT marker does not say where it ends: where the range decoder's code is 0 one
        # byte early (a last byte whose every bit took the lower part of the range), cap - 1 bytes are a valid end by the reference's own rule --
        # and by liblzma's, which must then give the same bytes.  Such streams are counted; with a marker there is no such case.
        if cap and (k % 3 == 1 or len(data) < 300):
            m1 = model_unlzma(payload, cap - 1, eos)
            v1 = lzma_verdict(payload, cap - 1, eos)
            if m1[0] == 0:
                assert not eos and m1[1] == data[:-1] and m1[6][3] == END_NO_MARKER and v1 in (("unsupported",), ("accepted", data[:-1], m1[3])), label
                early.append(label)
                continue
            assert m1[0] == E_DATA and m1[5] == "output beyond cap" and m1[1:4] == (b"", 0, 0), (label, m1[5])
            assert v1[0] != "accepted", label
    print("streams without marker that also end one byte early: %d of %d" % (len(early), len(streams)))
    assert wide > 500 and len(early) * 20 < len(streams)


def test_reference_payload():
    p, size, crc, sha = _unlzma.reference_payload()
    assert len(p) == 20990 and p[4:9] == bytes.fromhex("5d00800100")
    rc, out, ol, used, reg, rule, rec = model_unlzma(p, size, eos=False)
    assert rc == 0 and ol == size == 81682 and used == len(p) and rec[3] == END_NO_MARKER
    assert reg ^ 0xFFFFFFFF == crc == 0x840ff735 and hashlib.sha256(out).hexdigest() == sha
    assert lzma_verdict(p, size, False) == ("accepted", out, len(p))
    assert model_unlzma(p, size, eos=True)[0] == E_DATA                  # with the marker promised, its end is no end


def _run_corpus(M=None):
    cases = _unlzma.damaged_corpus()
    assert len(cases) == 20000
    accepted, excused = 0, []
    for k, (s, cap, eos, kind) in enumerate(cases):
        assert len(s) >= 9
        rc, out, ol, used, reg, rule, rec = model_unlzma(s, cap, eos, M=M)
        if rc == 0 and rec[3] == END_MARKER and not eos:                  # the reference accepts a marker in a stream of known size, liblzma does not
            excused.append(k)
            continue
        v = lzma_verdict(s, cap, eos)
        if v[0] == "accepted":
            accepted += 1
            assert (rc, out, used) == (0, v[1], v[2]), (k, kind, rule, rec)
            assert reg ^ 0xFFFFFFFF == zlib.crc32(out), k
        else:
            assert rc == E_DATA and (out, ol, used, reg) == (b"", 0, 0, 0xFFFFFFFF), (k, kind, v[0], rec)
    return accepted, excused


def test_damaged_corpus_equals_liblzma():
    accepted, excused = _run_corpus()
    print("accepted by liblzma: %d of 20000; excused (marker with eos = 0): %s" % (accepted, excused))
    assert accepted >= 1000
    assert len(excused) <= 5


def test_damaged_corpus_under_the_sanitizers():
    """The whole damaged corpus, the crafted cases and the reference's payload once more in a child process whose model is built with
    -fsanitize=address,undefined: every buffer the model reads or writes is an exact-size heap block."""
    lib = _unlzma.build_model(asan=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True, check=True).stdout.strip()
    code = ("import sys; sys.path.insert(0, %r); import _unlzma, test_unlzma_model as t; M = _unlzma.load_model(%r)\n"
            "print(t._run_corpus(M)[0]); t._check_crafted(M); p, size, crc, sha = _unlzma.reference_payload()\n"
            "assert _unlzma.model_unlzma(p, size, False, M=M)[2] == size; print('asan ok')\n") % (os.path.join(ROOT, "tests"), lib)
    env = dict(os.environ, LD_PRELOAD=" ".join(x for x in (libasan, os.environ.get("LD_PRELOAD", "")) if x), ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "asan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_crafted_cases():
    _check_crafted()


def _check_crafted(M=None):
    cases = _unlzma.crafted_cases()
    for want in ("props_size_4", "props_size_6", "props_byte_225", "dict_4999_distance_5000", "dict_5000_distance_5000", "dict_100_distance_3000",
                 "dict_100_distance_5000", "marker_eos0", "no_marker_eos1", "rep_match_first", "first_byte_1", "cut_11"):
        assert want in cases
    for name, (payload, cap, eos, expect, rule, end) in cases.items():
        rc, out, ol, used, reg, got_rule, rec = model_unlzma(payload, cap, eos, M=M)
        if expect is None:
            assert rc == E_DATA and (out, ol, used, reg) == (b"", 0, 0, 0xFFFFFFFF) and rec[3] == 0, name
            assert rule is None or got_rule == rule, (name, got_rule)
        else:
            assert rc == 0 and out == expect and rec[3] == end and reg ^ 0xFFFFFFFF == zlib.crc32(expect), (name, got_rule)
    # the first byte of the range coder and the distances beyond the dictionary are where liblzma and the reference part: liblzma's verdicts, for the record
    print({n: lzma_verdict(c[0], c[1], c[2])[0] for n, c in cases.items() if n.startswith(("dict_", "first_byte", "marker_eos0"))})
