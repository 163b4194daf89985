"""Inflate on the GPU (csrc/zada_inflate.hip: one wave per entry) against zlib, the expected bytes and the CPU model of the same decoder logic
(tests/inflate/inflate_host.cpp, tested against zlib and under ASan + UBSan in test_inflate_model.py); the archive reader on top of it."""
import ctypes
import hashlib
import io
import shutil
import subprocess
import time
import zipfile
import zlib

import numpy as np
import pytest

import _inflate
import _readers
from _inflate import E_DATA, model_inflate
from _common import product, silesia_mix
from test_inflate_model import deflate64_cases, deflate64_fixed

pytestmark = pytest.mark.gpu
PW = "p\xe4ss \xff"


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b) if len(b) else bytearray(1), dtype=torch.uint8).cuda()


def _device_inflate(enc, stream, cap, fmt=8, a_in=0, a_out=0, crc=0xFFFFFFFF):
    """inflate_device with the input at alignment a_in and the output at alignment a_out of a 256-byte aligned allocation, 16 guard bytes behind
    the output.  -> (bytes, in_used, crc register)"""
    import torch
    t_in = torch.zeros(len(stream) + 32, dtype=torch.uint8, device="cuda")
    t_in[a_in:a_in + len(stream)] = _dev(stream)[:len(stream)]
    t_out = torch.full((cap + 48,), 0xA5, dtype=torch.uint8, device="cuda")
    ol, used, reg = enc.inflate_device(t_in.data_ptr() + a_in, len(stream), t_out.data_ptr() + a_out, cap, fmt, crc)
    host = bytes(t_out.cpu().numpy())
    assert host[:a_out] == b"\xa5" * a_out and host[a_out + cap:] == b"\xa5" * (48 - a_out), "bytes outside the output buffer were written"
    assert ol <= cap
    return host[a_out:a_out + ol], used, reg


@pytest.fixture(scope="module")
def streams(encoder):
    """(label, data, stream): every input of the CPU test through the six zlib ways and through the product's Deflate_Fixed / _0 / _1 / _2 / _3
    (bit for bit the oracle's streams, test_gpu_parity.py -- made here on the GPU, where the oracle's Deflate_3 would take minutes)."""
    za = product()
    out = []
    for name, data in _inflate.valid_inputs().items():
        for lv, st in _inflate.ZLIB_WAYS:
            out.append(("%s/zlib%d.%d" % (name, lv, st), data, _inflate.zlib_raw(data, lv, st)))
        for m in (6, 7, 8, 9, 10):
            try:
                out.append(("%s/deflate%d" % (name, m), data, encoder.deflate(data, m)[0]))
            except za.CompressionInefficient:
                pass
    return out


def test_valid_streams_batch_single_and_device(encoder, streams):
    assert len(streams) > 500
    got = encoder.inflate_batch([s for _, _, s in streams], [len(d) for _, d, _ in streams], 8)
    for (label, data, stream), (rc, out, ol, used, reg) in zip(streams, got):
        assert rc == 0 and out == data and ol == len(data), label
        assert used == _inflate.zlib_in_used(stream), label
        assert reg ^ 0xFFFFFFFF == zlib.crc32(data), label
    # trailing bytes and a larger cap change nothing; one byte less of cap is a DataError for that entry alone
    some = streams[::7]
    got = encoder.inflate_batch([s + b"\x55" * 7 for _, _, s in some], [len(d) + 5 for _, d, _ in some], 8)
    for (label, data, stream), (rc, out, ol, used, reg) in zip(some, got):
        assert (rc, out, used) == (0, data, _inflate.zlib_in_used(stream)), label
    some = [x for x in streams[::5] if len(x[1])]
    caps = [len(d) - (i & 1) for i, (_, d, _) in enumerate(some)]
    got = encoder.inflate_batch([s for _, _, s in some], caps, 8)
    for i, ((label, data, stream), r) in enumerate(zip(some, got)):
        assert (r[0] == E_DATA and r[1] is None) if i & 1 else (r[0] == 0 and r[1] == data), label
    # the single call on host buffers: every stream with its size known; size unknown (the cap doubles from four times the payload, every
    # failed try decodes the stream again) and one byte less of cap for every 11th stream, and unknown only below 2 MiB -- a few-symbol stream of
    # 4 MiB would be decoded seven times over by one wave
    za = product()
    for k, (label, data, stream) in enumerate(streams):
        assert encoder.inflate(stream, len(data)) == (data, _inflate.zlib_in_used(stream), zlib.crc32(data) ^ 0xFFFFFFFF), label
        if k % 11:
            continue
        if len(data) < 2 << 20:
            assert encoder.inflate(stream)[0] == data, label
        if len(data):
            with pytest.raises(za.DataError):
                encoder.inflate(stream, len(data) - 1)
    with pytest.raises(za.DataError):
        encoder.inflate(b"", 10)
    with pytest.raises(za.ZadaError):
        encoder.inflate(b"\x03\x00", 0, format=7)
    assert encoder.inflate(b"\x03\x00", 0) == (b"", 2, 0xFFFFFFFF)
    assert encoder.inflate_batch([], []) == []
    # device pointers: every stream, the alignments of input and output rotating from stream to stream -- the pair (k mod 16, k div 16 mod 16)
    # walks through all 256 combinations in 256 streams --, then six streams at all sixteen alignments of both
    for k, (label, data, stream) in enumerate(streams):
        out, used, reg = _device_inflate(encoder, stream, len(data), 8, k % 16, (k // 16) % 16)
        assert out == data and used == _inflate.zlib_in_used(stream) and reg ^ 0xFFFFFFFF == zlib.crc32(data), (label, k)
    picks = [x for x in streams if x[0] in ("sample.xls/zlib9.0", "sample.jpg/zlib0.0", "text_65537/deflate10", "text_0/zlib9.0", "ab_80000/zlib6.4", "mix_300000/zlib0.0")]
    assert len(picks) == 6
    for label, data, stream in picks:
        for a in range(16):
            out, used, reg = _device_inflate(encoder, stream, len(data), 8, a, (a * 7 + 3) % 16)
            assert out == data and used == len(stream) and reg ^ 0xFFFFFFFF == zlib.crc32(data), (label, a)


def test_reference_fixtures_and_deflate64(encoder):
    za = product()
    cases = [(name, fmt, payload, hashlib.sha256, sha, size, crc) for name, fmt, payload, size, crc, sha in _inflate.many_formats()]
    want = {}
    for name, (tokens, far) in deflate64_cases().items():
        stream, exp = deflate64_fixed(tokens)
        want[name] = (stream, exp, far)
    payloads = [c[2] for c in cases] + [w[0] for w in want.values()]
    sizes = [c[5] for c in cases] + [len(w[1]) for w in want.values()]
    fmts = [c[1] for c in cases] + [9] * len(want)
    got = encoder.inflate_batch(payloads, sizes, fmts)
    for (name, fmt, payload, _, sha, size, crc), (rc, out, ol, used, reg) in zip(cases, got):
        assert rc == 0 and ol == size and used == len(payload) and hashlib.sha256(out).hexdigest() == sha and reg ^ 0xFFFFFFFF == crc, name
        assert encoder.inflate(payload, size, fmt)[0] == out
        assert _device_inflate(encoder, payload, size, fmt, 5, 9)[0] == out
    for (name, (stream, exp, far)), (rc, out, ol, used, reg) in zip(want.items(), got[len(cases):]):
        assert rc == 0 and out == exp and used == len(stream) and reg ^ 0xFFFFFFFF == zlib.crc32(exp), name
        assert encoder.inflate(stream, len(exp), 9)[0] == exp and encoder.inflate(stream, None, 9)[0] == exp, name
        assert _device_inflate(encoder, stream, len(exp), 9, 3, 1)[0] == exp, name
        if far:
            with pytest.raises(za.DataError):
                encoder.inflate(stream, len(exp), 8)
    # the same streams as format 8 in one batch: those that use a distance code 30 / 31 fail, alone
    got8 = encoder.inflate_batch([w[0] for w in want.values()], [len(w[1]) for w in want.values()], 8)
    for (name, (stream, exp, far)), r in zip(want.items(), got8):
        if far:
            assert r[0] == E_DATA, name


DAMAGED_TIME_LIMIT = 300          # seconds for the child process of the damaged corpus: it took 4 s when it was written


def test_damaged_corpus_equals_the_cpu_model():
    """20 000 damaged streams in ONE zada_inflate_batch call: rc, bytes written, input used and the bytes themselves equal the CPU model's for
    every entry (the model follows zlib's rule: test_inflate_model.py), and the 16 guard bytes behind every output buffer are untouched.
    An error-path test on inputs the same decoder logic has survived on a CPU under ASan + UBSan; it runs once, in a child process of its own under
    its own time limit, and nothing here runs it again if it fails."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import test_gpu_inflate as t; t._damaged_corpus_main()" % here
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=DAMAGED_TIME_LIMIT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "damaged corpus ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _damaged_corpus_main():
    za = product()
    encoder = za.Encoder(0)
    cases, _ = _inflate.damaged_corpus()
    cnt = len(cases)
    assert cnt == 20000
    lens = np.array([len(s) for s, _ in cases], dtype=np.uint64)
    caps = np.array([c for _, c in cases], dtype=np.uint64)
    keep = [s if len(s) else b"\0" for s, _ in cases]
    ins = np.array([ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p).value for s in keep], dtype=np.uint64)
    offs = np.concatenate(([0], np.cumsum(caps + 16)[:-1])).astype(np.uint64)
    arena = np.full(int((caps + 16).sum()), 0xA5, dtype=np.uint8)
    outp = (arena.ctypes.data + offs).astype(np.uint64)
    fm = np.full(cnt, 8, dtype=np.int32)
    ols, ius = np.zeros(cnt, np.uint64), np.zeros(cnt, np.uint64)
    crcs = np.full(cnt, 0xFFFFFFFF, dtype=np.uint32)
    rcs = np.full(cnt, 99, dtype=np.int32)
    t0 = time.time()
    worst = encoder.lib.zada_inflate_batch(encoder.ctx, cnt, fm.ctypes.data, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data, caps.ctypes.data,
                                           ols.ctypes.data, ius.ctypes.data, crcs.ctypes.data, rcs.ctypes.data)
    print("damaged corpus: %.2f s, worst rc %d (%s)" % (time.time() - t0, worst, encoder.lib.zada_last_error(encoder.ctx).decode()))
    assert worst == E_DATA
    n_ok = 0
    for k, (s, cap) in enumerate(cases):
        rc, out, ol, used, reg, rule = model_inflate(s, cap, 8)
        o = int(offs[k])
        assert (int(rcs[k]), int(ols[k]), int(ius[k])) == (rc, ol, used), (k, rule)
        assert arena[o + cap:o + cap + 16].tobytes() == b"\xa5" * 16, k
        if rc == 0:
            assert arena[o:o + ol].tobytes() == out and int(crcs[k]) == reg, k
            n_ok += 1
    assert n_ok > 10000
    # the same on device buffers, one entry per call, guard bytes in device memory on both sides of the output
    for k in range(0, cnt, 97):
        s, cap = cases[k]
        rc, out, ol, used, reg, _ = model_inflate(s, cap, 8)
        if rc == 0:
            assert _device_inflate(encoder, s, cap, 8, k % 16, (k // 16) % 16) == (out, used, reg), k
        elif len(s):
            try:
                _device_inflate(encoder, s, cap, 8, k % 16, (k // 16) % 16)
            except za.DataError:
                pass
            else:
                raise AssertionError("entry %d: the device call accepted what the model refuses" % k)
    # what zada.h promises a C caller for such an entry: *out_len = *in_used = 0, the CRC register as it was
    import torch
    s, cap = next((s, cap) for s, cap in cases if len(s) and model_inflate(s, cap, 8)[0] != 0)
    t_in, t_out = _dev(s), torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    ol, iu, reg = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(0x1234)
    assert encoder.lib.zada_inflate_device(encoder.ctx, 8, t_in.data_ptr(), len(s), t_out.data_ptr(), cap, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg)) == E_DATA
    assert (ol.value, iu.value, reg.value) == (0, 0, 0x1234)
    hostbuf = ctypes.create_string_buffer(cap + 1)
    ol, iu = ctypes.c_uint64(77), ctypes.c_uint64(77)
    assert encoder.lib.zada_inflate(encoder.ctx, 8, ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p), len(s), ctypes.addressof(hostbuf), cap, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg)) == E_DATA
    assert (ol.value, iu.value, reg.value) == (0, 0, 0x1234)
    # sizes no device holds are refused before anything is sized from them
    assert encoder.lib.zada_inflate_device(encoder.ctx, 8, t_in.data_ptr(), len(s), t_out.data_ptr(), (1 << 64) - 8, None, None, None) == -4
    try:
        encoder.inflate_batch([s, s], [(1 << 64) - 8, 40], 8)
    except za.ZadaError:
        pass
    else:
        raise AssertionError("a cap near 2 ** 64 was taken")
    encoder.close()
    print("damaged corpus ok")


@pytest.fixture(scope="module")
def mix():
    return silesia_mix(200 << 20)


@pytest.mark.parametrize("method", (6, 7, 8, 9, 10, 11))
def test_round_trip_at_the_writers_shapes(encoder, mix, method):
    rng = np.random.default_rng(method)
    shapes = [[mix[i * 16384:(i + 1) * 16384] for i in range(10000)], []]
    off = 0
    for ln in rng.integers(0, 40001, 5000):
        shapes[1].append(mix[off:off + int(ln)]); off += int(ln)
    for datas in shapes:
        t0 = time.time()
        packed = encoder.deflate_batch(datas, method)
        t1 = time.time()
        comp = [i for i, (rc, _, _) in enumerate(packed) if rc == 0]
        got = encoder.inflate_batch([packed[i][1] for i in comp], [len(datas[i]) for i in comp], 8)
        t2 = time.time()
        print("method %d: %d entries, deflate_batch %.2f s, inflate_batch %.2f s" % (method, len(datas), t1 - t0, t2 - t1))
        assert len(comp) > len(datas) * 0.9
        for i, (rc, out, ol, used, reg) in zip(comp, got):
            assert rc == 0 and out == datas[i] and used == len(packed[i][1]) and reg == packed[i][2], i


def test_one_long_stream_on_device(encoder, mix):
    import torch
    n = 16 << 20
    data = mix[5 << 20:(5 << 20) + n]
    stream, reg_w = encoder.deflate(data, 10)
    t_in, t_out = _dev(stream), torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    t0 = time.time()
    ol, used, reg = encoder.inflate_device(t_in.data_ptr(), len(stream), t_out.data_ptr(), n)
    print("16 MiB stream, one wave: %.2f s" % (time.time() - t0))
    assert (ol, used, reg) == (n, len(stream), reg_w) and reg ^ 0xFFFFFFFF == zlib.crc32(data)
    assert bytes(t_out[:n].cpu().numpy()) == data


def _entries(mix):
    return [("a/text.txt", silesia_mix(200000, class_mask=1)), ("b/rand.bin", bytes(np.random.RandomState(3).randint(0, 256, 3000).astype(np.uint8))),
            ("empty", b""), ("mix.bin", mix[:600000]), ("one", b"z"), ("c/ümlaut.txt", b"abc" * 5000), ("photo.jpg", _inflate.golden("sample.jpg"))]


def _check_archive(encoder, archive, entries, password=None):
    za = product()
    info = za.ZipInfo.load(archive)
    uz = za.UnZip(encoder)
    want = dict(entries)
    assert uz.extract(info, password=password) == want
    assert uz.extract(info, password=password, test_only=True) == {nm: None for nm in want}
    assert uz.extract(info, what=[entries[3][0], entries[0][0]], password=password) == {entries[3][0]: entries[3][1], entries[0][0]: entries[0][1]}
    assert uz.extract(info, what=entries[1][0], password=password) == {entries[1][0]: entries[1][1]}
    return info


@pytest.mark.parametrize("password", (None, PW))
def test_archives_of_the_writer(encoder, mix, password):
    za = product()
    entries = _entries(mix)
    # Preselection_1 on names and sizes that stay Deflate (neutral content below 9 000 bytes: Deflate_3, zip-compress.adb:243-327)
    small = [("s/a.txt", silesia_mix(7000, class_mask=1)), ("s/rand.bin", entries[1][1]), ("s/empty", b""), ("s/mix.dat", mix[:5000]), ("s/abc", b"abc" * 2000)]
    for method, ents in ((za.Method.Deflate_3, entries), (za.Method.Deflate_1, entries), (za.Method.Preselection_1, small)):
        zc = za.ZipCreate(encoder, method)
        zc.add_streams([e[0] for e in ents], [e[1] for e in ents], password=password)
        info = _check_archive(encoder, zc.finish(), ents, password)
        assert {e.method for e in info.entries} <= {0, 8}
        kinds = {e.method for e in info.entries}
        assert 8 in kinds and 0 in kinds                   # Deflate, and Store by fallback (random bytes, the empty entry)
        assert all(e.encrypted == (password is not None) for e in info.entries)
    zc = za.ZipCreate(encoder, za.Method.Deflate_2)
    for name, data in entries:
        zc.add_stream(name, data, password=password)
    _check_archive(encoder, zc.finish(), entries, password)


def test_archives_of_zipfile_and_zip(encoder, mix, tmp_path):
    entries = _entries(mix)
    for method in (zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED):
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w", method) as z:
            for nm, d in entries:
                z.writestr(nm, d)
            z.comment = b"made by zipfile"
        _check_archive(encoder, b.getvalue(), entries)

    class W(io.RawIOBase):                                  # an unseekable writer: bit 3, sizes and CRC behind the data
        def __init__(self):
            self.b = bytearray()

        def writable(self):
            return True

        def write(self, d):
            self.b += d
            return len(d)
    w = W()
    with zipfile.ZipFile(w, "w", zipfile.ZIP_DEFLATED) as z:
        for nm, d in entries:
            z.writestr(nm, d)
    info = _check_archive(encoder, bytes(w.b), entries)
    assert all(e.flags & 8 for e in info.entries)
    if shutil.which("zip"):
        ascii_entries = [(nm, d) for nm, d in entries if nm.isascii()]
        for nm, d in ascii_entries:
            p = tmp_path / nm
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_bytes(d)
        for pw in (None, "zip-pw"):
            arc = tmp_path / ("pw.zip" if pw else "plain.zip")
            cmd = ["zip", "-q", "-X"] + (["-P", pw] if pw else []) + [str(arc)] + [nm for nm, _ in ascii_entries]
            subprocess.run(cmd, cwd=tmp_path, check=True, timeout=120)
            _check_archive(encoder, arc.read_bytes(), ascii_entries, pw)


def test_what_the_reader_refuses(encoder, mix):
    za = product()
    uz = za.UnZip(encoder)
    entries = _entries(mix)
    zc = za.ZipCreate(encoder, za.Method.Deflate_3)
    zc.add_streams([e[0] for e in entries], [e[1] for e in entries], password=PW)
    arc = zc.finish()
    info = za.ZipInfo.load(arc)
    with pytest.raises(za.WrongPassword):
        uz.extract(info, password="not it")
    with pytest.raises(za.WrongPassword):
        uz.extract(info)
    v = uz.extract(info, password="not it", test_only=True)
    assert sum(isinstance(x, za.WrongPassword) for x in v.values()) >= len(entries) - 1      # (one header in 256 passes the check byte by chance)
    # one flipped payload byte: CRCError or DataError for that entry, the others still extracted
    plain = za.ZipCreate(encoder, za.Method.Deflate_3)
    plain.add_streams([e[0] for e in entries], [e[1] for e in entries])
    arc = plain.finish()
    info = za.ZipInfo.load(arc)
    for name, at in (("mix.bin", 1000), ("a/text.txt", 30), ("b/rand.bin", 5), ("photo.jpg", 40000)):
        e = info[name]
        bad = bytearray(arc)
        bad[e.data_offset + min(at, e.csize - 1)] ^= 0x10
        got = uz.extract(za.ZipInfo.load(bytes(bad)), errors="collect")
        # (CRCError or DataError as a rule; SizeError is the third legitimate verdict: a flipped bit can make a stream that ends early and validly)
        assert isinstance(got[name], (za.CRCError, za.DataError, za.SizeError)), name
        assert {k: v for k, v in got.items() if k != name} == {k: v for k, v in entries if k != name}
        with pytest.raises((za.CRCError, za.DataError, za.SizeError)) as ex:
            uz.extract(za.ZipInfo.load(bytes(bad)))
        assert ex.value.results[name] is ex.value
        t = uz.extract(za.ZipInfo.load(bytes(bad)), test_only=True)
        assert isinstance(t[name], za.ZadaError) and all(x is None for k, x in t.items() if k != name)
    # a BZip2 entry: UnsupportedMethod for it only
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr("one.txt", entries[0][1])
        z.writestr(zipfile.ZipInfo("two.bz2"), entries[3][1], compress_type=zipfile.ZIP_BZIP2)
        z.writestr("three.txt", entries[5][1])
    got = uz.extract(za.ZipInfo.load(b.getvalue()), errors="collect")
    assert got["one.txt"] == entries[0][1] and got["three.txt"] == entries[5][1]
    assert isinstance(got["two.bz2"], za.UnsupportedMethod) and "BZip2" in str(got["two.bz2"]) and "out of scope" in str(got["two.bz2"])
    with pytest.raises(za.UnsupportedMethod):
        uz.extract(za.ZipInfo.load(b.getvalue()))


def test_crypt_decode_batch_undoes_encode(encoder, mix):
    rng = np.random.default_rng(9)
    lens = [0, 1, 11, 12, 13, 255, 256, 257, 70000] + [int(x) for x in rng.integers(0, 5000, 300)]
    datas = [mix[i * 7000:i * 7000 + ln] for i, ln in enumerate(lens)]
    keys = [tuple(int(x) for x in row) for row in rng.integers(0, 1 << 32, (len(lens), 3), dtype=np.uint64)]
    coded = encoder.crypt_encode_batch(keys, datas)
    back = encoder.crypt_decode_batch(keys, [c for c, _ in coded])
    M = _inflate.model()
    for d, k, (c, kc), (p, kp) in zip(datas, keys, coded, back):
        assert p == d and kp == kc
        kk = (ctypes.c_uint32 * 3)(*k)
        buf = np.frombuffer(c, dtype=np.uint8).copy() if len(c) else np.zeros(1, np.uint8)
        M.im_crypt_decode(kk, buf.ctypes.data, len(c))
        assert buf[:len(c)].tobytes() == d and tuple(kk) == kc
    assert encoder.crypt_decode_batch([], []) == []


def test_argument_checks_come_first(encoder):
    _readers.argument_checks(encoder, "inflate")


def test_several_launch_groups(encoder):
    """batch_mib = 1: the entries go through several groups; zlib says what every entry holds."""
    _readers.several_launch_groups(encoder, "inflate")
