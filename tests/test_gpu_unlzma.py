"""The LZMA reader on the GPU (csrc/zada_unlzma.hip: one wave per entry) against the expected bytes and the CPU model of the same decoder logic
(tests/unlzma/unlzma_host.cpp, tested against liblzma and under ASan + UBSan in test_unlzma_model.py); the archive reader on top."""
import ctypes
import hashlib
import io
import subprocess
import time
import zipfile
import zlib

import numpy as np
import pytest

import _readers
import _unlzma
from _unlzma import E_DATA, model_unlzma
from _common import product, silesia_mix

pytestmark = pytest.mark.gpu
PW = "p\xe4ss \xff"
R_OUTPUT_FULL = 2


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b) if len(b) else bytearray(1), dtype=torch.uint8).cuda()


def _device_unlzma(enc, payload, cap, eos, a_in=0, a_out=0, crc=0xFFFFFFFF):
    """unlzma_device with the input at alignment a_in and the output at alignment a_out of a 256-byte aligned allocation, guard bytes on both
    sides of the output.  -> (bytes, in_used, crc register)"""
    import torch
    t_in = torch.zeros(len(payload) + 32, dtype=torch.uint8, device="cuda")
    t_in[a_in:a_in + len(payload)] = _dev(payload)[:len(payload)]
    t_out = torch.full((cap + 48,), 0xA5, dtype=torch.uint8, device="cuda")
    try:
        ol, used, reg = enc.unlzma_device(t_in.data_ptr() + a_in, len(payload), t_out.data_ptr() + a_out, cap, eos, crc)
    finally:
        host = bytes(t_out.cpu().numpy())
        assert host[:a_out] == b"\xa5" * a_out and host[a_out + cap:] == b"\xa5" * (48 - a_out), "bytes outside the output buffer were written"
    assert ol <= cap
    return host[a_out:a_out + ol], used, reg


def _guarded_batch(enc, payloads, caps, eos):
    """zada_unlzma_batch with 16 guard bytes on both sides of every output buffer -> (rcs, out_lens, in_useds, crcs, outputs); asserts the guards."""
    cnt = len(payloads)
    lens = np.array([len(s) for s in payloads], dtype=np.uint64)
    caps = np.array(caps, dtype=np.uint64)
    flags = np.array([int(bool(x)) for x in eos], dtype=np.int32)
    keep = [s if len(s) else b"\0" for s in payloads]
    ins = np.array([ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p).value for s in keep], dtype=np.uint64)
    offs = (np.concatenate(([0], np.cumsum(caps + 32)[:-1])) + 16).astype(np.uint64)
    arena = np.full(int((caps + 32).sum()), 0xA5, dtype=np.uint8)
    outp = (arena.ctypes.data + offs).astype(np.uint64)
    ols, ius = np.zeros(cnt, np.uint64), np.zeros(cnt, np.uint64)
    crcs = np.full(cnt, 0xFFFFFFFF, dtype=np.uint32)
    rcs = np.full(cnt, 99, dtype=np.int32)
    worst = enc.lib.zada_unlzma_batch(enc.ctx, cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data, caps.ctypes.data, flags.ctypes.data, ols.ctypes.data,
                                      ius.ctypes.data, crcs.ctypes.data, rcs.ctypes.data)
    assert worst in (0, E_DATA), (worst, enc.lib.zada_last_error(enc.ctx))
    outs = []
    for k in range(cnt):
        o, cap = int(offs[k]), int(caps[k])
        assert arena[o - 16:o].tobytes() == b"\xa5" * 16 and arena[o + cap:o + cap + 16].tobytes() == b"\xa5" * 16, k
        outs.append(arena[o:o + int(ols[k])].tobytes() if rcs[k] == 0 else None)
    return rcs, ols, ius, crcs, outs


@pytest.fixture(scope="module")
def streams():
    """(label, data, payload, eos): every input of the CPU test through liblzma's raw writer; the inputs of up to 5 000 bytes through all nineteen
    methods of the oracle's writer, with and without marker, and through the two parameter sets beyond liblzma; longer inputs of up to 70 000
    bytes through four methods (one per home of the literal table and level); the reference's own payload."""
    out = list(_unlzma.valid_streams(oracle_limit=5000))
    from _bunzip2 import valid_inputs
    for name, data in valid_inputs().items():
        if 5000 < len(data) <= 70000:
            for m in (15, 18, 20, 32):
                out.append(("%s/m%d" % (name, m), bytes(data), _unlzma.oracle_payload(bytes(data), m, m != 18), m != 18))
    p, size, crc, sha = _unlzma.reference_payload()
    out.append(("reference/$16_lzma.tmp", model_unlzma(p, size, False)[1], p, False))
    return out


def _model_of(streams):
    return [model_unlzma(p, len(d), eos) for _, d, p, eos in streams]


def test_valid_streams_batch(encoder, streams):
    assert len(streams) > 1000
    models = _model_of(streams)
    got = encoder.unlzma_batch([p for _, _, p, _ in streams], [len(d) for _, d, _, _ in streams], [e for _, _, _, e in streams])
    for (label, data, payload, eos), m, (rc, out, ol, used, reg) in zip(streams, models, got):
        assert m[0] == 0 and m[1] == data, label
        assert rc == 0 and out == data and ol == len(data), label
        assert used == m[3] and reg == m[4] and reg ^ 0xFFFFFFFF == zlib.crc32(data), label
    # trailing bytes change nothing; nor does a larger cap where the stream has a marker
    some = streams[::7]
    got = encoder.unlzma_batch([p + b"\x55\x00\xaa" for _, _, p, _ in some], [len(d) + (5 if e else 0) for _, d, _, e in some], [e for _, _, _, e in some])
    for (label, data, payload, eos), (rc, out, ol, used, reg) in zip(some, got):
        assert (rc, out, used) == (0, data, model_unlzma(payload, len(data), eos)[3]), label
    # one byte less of cap for every eleventh stream: E_DATA by the output rule for that entry alone, the guard bytes around every buffer untouched
    some = [x for x in streams if len(x[1])]
    caps = [len(d) - (1 if i % 11 == 0 else 0) for i, (_, d, _, _) in enumerate(some)]
    rcs, ols, ius, crcs, outs = _guarded_batch(encoder, [p for _, _, p, _ in some], caps, [e for _, _, _, e in some])
    rules = encoder.unlzma_last_records()
    for i, (label, data, payload, eos) in enumerate(some):
        if i % 11 == 0:
            m = model_unlzma(payload, len(data) - 1, eos)       # (a stream without marker may end one byte early as well: test_unlzma_model.py)
            assert m[0] == E_DATA or not eos, label
            assert (int(rcs[i]), int(ols[i]), int(ius[i])) == (m[0], m[2], m[3]) and tuple(int(x) for x in rules[i]) == m[6], label
            assert rcs[i] == 0 or (ols[i] == 0 and ius[i] == 0 and int(rules[i, 0]) == R_OUTPUT_FULL), label
        else:
            assert rcs[i] == 0 and outs[i] == data and int(rules[i, 3]) == model_unlzma(payload, len(data), eos)[6][3], label


def test_valid_streams_single(encoder, streams):
    """The single call on host buffers; size unknown and one byte less of cap for every eleventh stream."""
    za = product()
    for k, (label, data, payload, eos) in enumerate(streams[::3]):
        out, used, reg = encoder.unlzma(payload, len(data), eos)
        assert out == data and used == model_unlzma(payload, len(data), eos)[3] and reg == zlib.crc32(data) ^ 0xFFFFFFFF, label
        if k % 11:
            continue
        if eos:
            assert encoder.unlzma(payload)[0] == data, label
        if len(data) and model_unlzma(payload, len(data) - 1, eos)[0]:
            with pytest.raises(za.DataError):
                encoder.unlzma(payload, len(data) - 1, eos)
    with pytest.raises(za.DataError):
        encoder.unlzma(b"", 10)
    assert encoder.unlzma_batch([], []) == []


def test_valid_streams_device(encoder, streams):
    """Device pointers: the alignments of input and output rotate over all sixteen each from stream to stream."""
    for k, (label, data, payload, eos) in enumerate(streams[::3]):
        out, used, reg = _device_unlzma(encoder, payload, len(data), eos, k % 16, (k // 16) % 16)
        assert out == data and used == model_unlzma(payload, len(data), eos)[3] and reg ^ 0xFFFFFFFF == zlib.crc32(data), (label, k)


def test_reference_payload_without_marker(encoder):
    p, size, crc, sha = _unlzma.reference_payload()
    out, used, reg = encoder.unlzma(p, size, eos=False)
    assert len(out) == size and used == len(p) and hashlib.sha256(out).hexdigest() == sha and reg ^ 0xFFFFFFFF == crc
    assert [int(x) for x in encoder.unlzma_last_records()[0]] == [0, len(p), size, _unlzma.END_NO_MARKER]
    za = product()
    with pytest.raises(za.DataError):                             # its flags promise no marker, and it has none
        encoder.unlzma(p, size, eos=True)


DAMAGED_TIME_LIMIT = 600          # seconds for the child process of the damaged corpus


def test_damaged_corpus_equals_the_cpu_model():
    """20 000 damaged payloads in ONE zada_unlzma_batch call: rc, rule, bytes written, input used, the bytes themselves and the CRC equal the CPU
    model's for every entry (the model follows liblzma: test_unlzma_model.py), and the 16 guard bytes around every output buffer are untouched.
    It runs once, in a child process of its own under its own time limit, and nothing here runs it again if it fails."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import test_gpu_unlzma as t; t._damaged_corpus_main()" % here
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=DAMAGED_TIME_LIMIT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "damaged corpus ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _damaged_corpus_main():
    za = product()
    encoder = za.Encoder(0)
    cases = _unlzma.damaged_corpus()
    assert len(cases) == 20000
    t0 = time.time()
    rcs, ols, ius, crcs, outs = _guarded_batch(encoder, [s for s, _, _, _ in cases], [c for _, c, _, _ in cases], [e for _, _, e, _ in cases])
    print("damaged corpus: %.2f s (%s)" % (time.time() - t0, encoder.lib.zada_last_error(encoder.ctx).decode()))
    rules = encoder.unlzma_last_records()
    n_ok = 0
    for k, (s, cap, eos, kind) in enumerate(cases):
        rc, out, ol, used, reg, rule, rec = model_unlzma(s, cap, eos)
        assert (int(rcs[k]), int(ols[k]), int(ius[k])) == (rc, ol, used), (k, kind, rule, [int(x) for x in rules[k]])
        assert tuple(int(x) for x in rules[k]) == rec, (k, kind, rule, rec, [int(x) for x in rules[k]])
        if rc == 0:
            assert outs[k] == out and int(crcs[k]) == reg, k
            n_ok += 1
        else:
            assert int(crcs[k]) == 0xFFFFFFFF, k
    print("accepted", n_ok)
    assert n_ok >= 1000
    # the same on device buffers, one entry per call, guard bytes in device memory on both sides of the output
    for k in range(0, len(cases), 197):
        s, cap, eos, _ = cases[k]
        rc, out, ol, used, reg, _, _ = model_unlzma(s, cap, eos)
        if rc == 0:
            assert _device_unlzma(encoder, s, cap, eos, k % 16, (k // 16) % 16) == (out, used, reg), k
        else:
            try:
                _device_unlzma(encoder, s, cap, eos, k % 16, (k // 16) % 16)
            except za.DataError:
                pass
            else:
                raise AssertionError("entry %d: the device call accepted what the model refuses" % k)
    # what zada.h promises a C caller for such an entry: *out_len = *in_used = 0, the CRC register as it was
    import torch
    s, cap, eos, _ = next(c for c in cases if model_unlzma(c[0], c[1], c[2])[0] != 0)
    t_in, t_out = _dev(s), torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    ol, iu, reg = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(0x1234)
    assert encoder.lib.zada_unlzma_device(encoder.ctx, t_in.data_ptr(), len(s), t_out.data_ptr(), cap, int(eos), ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg)) == E_DATA
    assert (ol.value, iu.value, reg.value) == (0, 0, 0x1234)
    assert b"unlzma: entry 0: " in encoder.lib.zada_last_error(encoder.ctx) and b" at input byte " in encoder.lib.zada_last_error(encoder.ctx)
    # null pointers, and sizes no device holds, are refused before anything is sized from them
    assert encoder.lib.zada_unlzma_device(encoder.ctx, t_in.data_ptr(), len(s), t_out.data_ptr(), (1 << 64) - 8, 1, None, None, None) == -4
    assert encoder.lib.zada_unlzma_device(encoder.ctx, None, 5, t_out.data_ptr(), 5, 1, None, None, None) == -1
    assert encoder.lib.zada_unlzma_device(encoder.ctx, t_in.data_ptr(), len(s), None, 5, 1, None, None, None) == -1
    assert encoder.lib.zada_unlzma(encoder.ctx, None, 5, None, 0, 1, None, None, None) == -1
    assert encoder.lib.zada_unlzma_batch(encoder.ctx, 1, None, None, None, None, None, None, None, None, None) == -1
    try:
        encoder.unlzma_batch([s, s], [(1 << 64) - 8, 40])
    except za.ZadaError:
        pass
    else:
        raise AssertionError("a cap near 2 ** 64 was taken")
    encoder.close()
    print("damaged corpus ok")


def test_crafted_streams_alone_and_as_neighbours(encoder):
    cases = _unlzma.crafted_cases()
    names = list(cases)
    for name in names:
        payload, cap, eos, expect, rule, end = cases[name]
        got = encoder.unlzma_batch([payload], [cap], [eos])[0]
        rec = encoder.unlzma_last_records()
        m = model_unlzma(payload, cap, eos)
        assert tuple(int(x) for x in rec[0]) == m[6], name
        if expect is None:
            assert got[0] == E_DATA and (rule is None or rule == m[5]), name
        else:
            assert got[0] == 0 and got[1] == expect and got[3] == m[3] and int(rec[0, 3]) == end, name
    # as neighbours in one arena with exact caps: the staging of one entry does not read its neighbour's bytes (a cut stream reads zeros behind
    # its end, not the next entry's first bytes)
    order = names + list(reversed(names))
    batch = [cases[n] for n in order]
    rcs, ols, ius, crcs, outs = _guarded_batch(encoder, [c[0] for c in batch], [c[1] for c in batch], [c[2] for c in batch])
    rec = encoder.unlzma_last_records()
    for k, c in enumerate(batch):
        m = model_unlzma(c[0], c[1], c[2])
        assert (int(rcs[k]), outs[k], int(ius[k])) == (m[0], m[1] if m[0] == 0 else None, m[3]) and tuple(int(x) for x in rec[k]) == m[6], order[k]
        assert (rcs[k] == 0) == (c[3] is not None), order[k]


def _rle_payload(n, lc=3, lp=0, pb=2):
    return _unlzma.raw_payload(b"A" * n, lc, lp, pb)


def test_smallest_shapes(encoder):
    """Entries of 0, 1 and 2 bytes; a match with distance 1 and length 273; a match that ends exactly at cap; inputs of the stage size +- 1; the
    literal table in LDS (lc + lp = 3) and in HBM (4, 8, 12), the last as two entries in two launch groups."""
    cases = []
    for d in (b"", b"x", b"xy"):
        cases.append((d, _unlzma.raw_payload(d), True))
        cases.append((d, _unlzma.oracle_payload(d, 18, False), False))
    d = b"A" * 274                                              # a literal, then distance 1 and length 273, ending exactly at cap
    cases.append((d, _unlzma.raw_payload(d), True))
    cases.append((d, _unlzma.oracle_payload(d, 18, False), False))
    cases.append((b"A" * 275, _unlzma.raw_payload(b"A" * 275), True))
    d = b"abcdefg" * 100 + b"xyz" + b"abcdefg" * 39             # a long match that ends exactly at cap
    cases.append((d, _unlzma.oracle_payload(d, 17, False), False))
    rng = np.random.default_rng(4)
    rnd = bytes(rng.integers(0, 256, 2000, dtype=np.uint8))
    sized = {}
    for n in range(300, 460):                                   # random bytes: the payload grows with the input -- find the lengths around the stage
        p = _unlzma.raw_payload(rnd[:n], 0, 0, 0)
        sized.setdefault(len(p), (rnd[:n], p, True))
    hit = [sized[k] for k in (_unlzma.STAGE - 1, _unlzma.STAGE, _unlzma.STAGE + 1, 2 * _unlzma.STAGE - 1) if k in sized]
    assert len(hit) >= 3, sorted(sized)
    cases += hit
    text = _unlzma.golden("sample.xls")[:30000]
    for lc, lp, pb in ((3, 0, 2), (2, 1, 0), (4, 0, 2), (0, 4, 0)):                  # lc + lp = 3, 3, 4, 4
        cases.append((text, _unlzma.raw_payload(text, lc, lp, pb), True))
    for m in (23, 30, 20, 24):                                  # lc + lp = 8, 8, 12, 12
        cases.append((text, _unlzma.oracle_payload(text, m, True), True))
        cases.append((text[:999], _unlzma.oracle_payload(text[:999], m, False), False))
    got = encoder.unlzma_batch([p for _, p, _ in cases], [len(d) for d, _, _ in cases], [e for _, _, e in cases])
    for k, ((d, p, eos), (rc, out, ol, used, reg)) in enumerate(zip(cases, got)):
        m = model_unlzma(p, len(d), eos)
        assert m[0] == 0 and m[1] == d, k
        assert (rc, out, used, reg) == (0, d, m[3], m[4]), k
    # two entries with 6 MiB tables, the knob set so that each is a launch group of its own
    encoder.set_knob("lzma_lit_mib", 6)
    try:
        two = [(text, _unlzma.oracle_payload(text, 24, True), True), (text[5000:], _unlzma.oracle_payload(text[5000:], 20, False), False)]
        got = encoder.unlzma_batch([p for _, p, _ in two], [len(d) for d, _, _ in two], [e for _, _, e in two])
        for (d, p, eos), (rc, out, ol, used, reg) in zip(two, got):
            assert (rc, out, used) == (0, d, model_unlzma(p, len(d), eos)[3])
    finally:
        encoder.set_knob("lzma_lit_mib", 12288)


@pytest.fixture(scope="module")
def mix2():
    return silesia_mix(4 << 20, version=2)


@pytest.mark.parametrize("method", (15, 18, 23, 32))
def test_round_trip_of_small_entries(encoder, mix2, method):
    rng = np.random.default_rng(method)
    datas, off = [], 0
    for ln in rng.integers(0, 40001, 2000):
        datas.append(mix2[off % (3 << 20):off % (3 << 20) + int(ln)]); off += int(ln)
    t0 = time.time()
    packed = encoder.lzma_batch(datas, method)
    t1 = time.time()
    got = encoder.unlzma_batch([p[1] for p in packed], [len(d) for d in datas], True)
    t2 = time.time()
    print("method %d: %d entries, lzma_batch %.2f s, unlzma_batch %.2f s" % (method, len(datas), t1 - t0, t2 - t1))
    for i, (rc, out, ol, used, reg) in enumerate(got):
        assert rc == 0 and out == datas[i] and used == len(packed[i][1]) and reg == packed[i][2], i
    # test_only: verdicts, sizes and CRCs without bytes
    got = encoder.unlzma_batch([p[1] for p in packed[:300]], [len(d) for d in datas[:300]], True, deliver=False)
    for i, (rc, out, ol, used, reg) in enumerate(got):
        assert (rc, out, ol, reg) == (0, None, len(datas[i]), packed[i][2]), i


def _entries(mix2):
    return [("a/text.txt", silesia_mix(200000, class_mask=1)), ("b/rand.bin", bytes(np.random.RandomState(3).randint(0, 256, 3000).astype(np.uint8))),
            ("empty", b""), ("mix.bin", mix2[:1200000]), ("one", b"z"), ("c/ümlaut.txt", b"abc" * 5000), ("photo.jpg", _unlzma.golden("sample.jpg"))]


@pytest.mark.parametrize("password", (None, PW))
@pytest.mark.parametrize("method", ("LZMA_3", "Preselection_2"))
def test_archives_of_the_writer(encoder, mix2, method, password):
    za = product()
    entries = _entries(mix2)
    zc = za.ZipCreate(encoder, getattr(za.Method, method))
    zc.add_streams([e[0] for e in entries], [e[1] for e in entries], password=password)
    arc = zc.finish()
    info = za.ZipInfo.load(arc)
    uz = za.UnZip(encoder, bzip2=True, lzma=True)
    want = dict(entries)
    assert uz.extract(info, password=password) == want
    assert uz.extract(info, password=password, test_only=True) == {nm: None for nm in want}
    assert uz.extract(info, what=[entries[3][0], entries[0][0]], password=password) == {entries[3][0]: entries[3][1], entries[0][0]: entries[0][1]}
    assert 14 in {e.method for e in info.entries}
    assert all(e.encrypted == (password is not None) for e in info.entries)
    # the readers without lzma=True still leave these entries alone, with the words they always had
    for uz0, words in ((za.UnZip(encoder), ("BZip2 and LZMA decoding are out of scope",)), (za.UnZip(encoder, bzip2=True), ("LZMA decoding is out of scope",))):
        got = uz0.extract(info, password=password, errors="collect")
        for e in info.entries:
            if e.method == 14:
                assert isinstance(got[e.name], za.UnsupportedMethod) and all(w in str(got[e.name]) for w in words)
                assert ("method 14 (LZMA) is not decoded by this reader: Store, Deflate" in str(got[e.name]))
            elif e.method != 12:
                assert got[e.name] == want[e.name]


def test_archive_of_zipfile_and_one_flipped_byte(encoder, mix2):
    za = product()
    entries = _entries(mix2)
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w", zipfile.ZIP_LZMA) as z:
        for nm, d in entries:
            z.writestr(nm, d)
        z.writestr(zipfile.ZipInfo("deflated.txt"), entries[0][1], compress_type=zipfile.ZIP_DEFLATED)
        z.writestr(zipfile.ZipInfo("bzip2.bin"), entries[5][1], compress_type=zipfile.ZIP_BZIP2)
    arc = b.getvalue()
    info = za.ZipInfo.load(arc)
    everything = dict(entries + [("deflated.txt", entries[0][1]), ("bzip2.bin", entries[5][1])])
    uz = za.UnZip(encoder, bzip2=True, lzma=True)
    assert uz.extract(info) == everything
    assert uz.extract(info, test_only=True) == {nm: None for nm in everything}
    # lzma alone: the BZip2 entry stays unsupported, in words that still say so
    got = za.UnZip(encoder, lzma=True).extract(info, errors="collect")
    assert isinstance(got["bzip2.bin"], za.UnsupportedMethod) and "BZip2" in str(got["bzip2.bin"]) and "out of scope" in str(got["bzip2.bin"])
    assert {k: v for k, v in got.items() if k != "bzip2.bin"} == {k: v for k, v in everything.items() if k != "bzip2.bin"}
    # one flipped payload byte: DataError, CRCError or SizeError for that entry only
    for name, at in (("mix.bin", 100000), ("a/text.txt", 30), ("photo.jpg", 40000), ("mix.bin", 11)):
        e = info[name]
        assert e.method == 14
        bad = bytearray(arc)
        bad[e.data_offset + min(at, e.csize - 1)] ^= 0x10
        got = uz.extract(za.ZipInfo.load(bytes(bad)), errors="collect")
        assert isinstance(got[name], (za.CRCError, za.DataError, za.SizeError)), name
        assert {k: v for k, v in got.items() if k != name} == {k: v for k, v in everything.items() if k != name}
        t = uz.extract(za.ZipInfo.load(bytes(bad)), test_only=True)
        assert isinstance(t[name], za.ZadaError) and all(x is None for k, x in t.items() if k != name)
    # a stream that ends on its marker with fewer bytes than the directory promises is a SizeError: a directory that promises three bytes more
    longer = za.ZipInfo.load(arc)
    longer["c/ümlaut.txt"].usize += 3
    got = za.UnZip(encoder, lzma=True).extract(longer, what="c/ümlaut.txt", errors="collect")
    assert isinstance(got["c/ümlaut.txt"], za.SizeError), got
    # the fixture's payload without marker through the batch, flags 0
    p, size, crc, sha = _unlzma.reference_payload()
    rc, out, ol, used, reg = encoder.unlzma_batch([p], [size], [False])[0]
    assert (rc, ol, used, reg ^ 0xFFFFFFFF) == (0, size, len(p), crc) and hashlib.sha256(out).hexdigest() == sha


def test_argument_checks_come_first(encoder):
    _readers.argument_checks(encoder, "unlzma")


def test_several_launch_groups(encoder):
    """batch_mib = 1: the entries go through several groups; liblzma says what every entry holds."""
    _readers.several_launch_groups(encoder, "unlzma")
