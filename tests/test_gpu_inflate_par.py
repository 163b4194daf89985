"""One large Deflate stream on many waves (csrc/zada_inflate_par.hip) through the C ABI: against zlib, against the one-wave decoder
(zada_inflate_device) and against the CPU models, with the record of every call asserted next to the bytes, so that a silent hand-over to the one
wave cannot pass as success.  Device buffers come from _devbuf.py: the input ends at its last byte, the output has guard bytes on both sides."""
import ctypes
import io
import os
import subprocess
import sys
import zipfile
import zlib

import numpy as np
import pytest

import _inflate
import _inflate_par as P
from _common import product, silesia_mix
from _devbuf import device_call
from _inflate import E_DATA, model_inflate

pytestmark = pytest.mark.gpu
PW = "p\xe4ss \xff"
DEFAULT_CHUNK_KIB = 64


@pytest.fixture()
def par(encoder):
    """The session's encoder with the knobs of the parallel path at their defaults before and after."""
    def reset():
        encoder.set_knob("inflate_par_chunk_kib", DEFAULT_CHUNK_KIB)
        encoder.set_knob("inflate_par_repair_pct", P.REPAIR_PCT)
        encoder.set_knob("inflate_par_min_kib", 0)
    reset()
    yield encoder
    reset()


def _par(enc, stream, cap, a_in=0, a_out=0, crc=0xFFFFFFFF):
    """zada_inflate_par_device on guarded buffers -> (rc, bytes, out_len, in_used, crc register, error text, record)"""
    ol, iu, reg = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(crc)

    def fn(d_in, n, d_out, cap):
        return enc.lib.zada_inflate_par_device(enc.ctx, 8, d_in, n, d_out, cap, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg))
    rc, out = device_call(fn, stream, cap, a_in, a_out)
    return rc, out[:ol.value], ol.value, iu.value, reg.value, enc.lib.zada_last_error(enc.ctx).decode(), enc.inflate_par_last()


def _one_wave(enc, stream, cap, a_in=0, a_out=0, crc=0xFFFFFFFF):
    ol, iu, reg = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(crc)

    def fn(d_in, n, d_out, cap):
        return enc.lib.zada_inflate_device(enc.ctx, 8, d_in, n, d_out, cap, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg))
    rc, out = device_call(fn, stream, cap, a_in, a_out)
    return rc, out[:ol.value], ol.value, iu.value, reg.value, enc.lib.zada_last_error(enc.ctx).decode()


@pytest.fixture(scope="module")
def streams(encoder):
    """(label, data, stream): the three golden samples and the 2 MiB corpus input through the six zlib ways and the product's Deflate_Fixed / _0 /
    _1 / _2 / _3 (bit for bit the oracle's methods 6 .. 10, test_gpu_parity.py -- made here on the GPU, where the oracle's Deflate_3 takes long)."""
    za = product()
    inputs = {k: _inflate.golden(k) for k in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin")}
    inputs["corpus_2m"] = P.corpus_2m()
    out = []
    for name, data in inputs.items():
        for lv, st in _inflate.ZLIB_WAYS:
            out.append(("%s/zlib%d.%d" % (name, lv, st), data, _inflate.zlib_raw(data, lv, st)))
        for m in (6, 7, 8, 9, 10):
            try:
                out.append(("%s/oracle%d" % (name, m), data, encoder.deflate(data, m)[0]))
            except za.CompressionInefficient:
                pass
    return out


def test_parity_on_valid_streams(par, streams):
    par.set_knob("inflate_par_chunk_kib", 4)
    assert len(streams) >= 40
    took = 0
    for label, data, stream in streams:
        got = _par(par, stream, len(data))
        info = got[6]
        assert got[:5] == (0, data, len(data), _inflate.zlib_in_used(stream), zlib.crc32(data) ^ 0xFFFFFFFF), (label, info)
        assert got[:5] == _one_wave(par, stream, len(data))[:5], label
        assert info["streams"] == 1 and info["chunks"] == (len(stream) + 4095) // 4096, (label, info)
        if label in P.NAMED_DYNAMIC:
            assert info["fell_back"] == 0 and info["reason"] == "none" and info["live_chunks"] >= 2, (label, info)
            assert info["repairs"] <= info["chunks"] * P.REPAIR_PCT // 100 + 2 and info["scout_rounds"] == 1 + info["repairs"], (label, info)
        took += not info["fell_back"]
    assert took >= 20, took
    # the host-pointer form and the Python layer
    label, data, stream = next(x for x in streams if x[0] == "corpus_2m/oracle10")
    assert par.inflate_par(stream, len(data)) == (data, len(stream), zlib.crc32(data) ^ 0xFFFFFFFF)
    assert par.inflate_par_last()["fell_back"] == 0
    # Deflate64 is the one wave's
    assert par.inflate_par(b"\x03\x00", 0, format=9) == (b"", 2, 0xFFFFFFFF)
    assert par.inflate_par_last()["reason"] == "format"
    with pytest.raises(product().ZadaError):
        par.inflate_par(b"\x03\x00", 0, format=7)


def test_chunk_size_sweep(par, streams):
    label, data, stream = next(x for x in streams if x[0] == "corpus_2m/oracle10")
    want = (0, data, len(data), len(stream), zlib.crc32(data) ^ 0xFFFFFFFF)
    for ck in (4, 8, 16, 64, 4096):
        par.set_knob("inflate_par_chunk_kib", ck)
        got = _par(par, stream, len(data))
        assert got[:5] == want, ck
        if ck == 4096:
            assert got[6]["fell_back"] == 1 and got[6]["reason"] == "single chunk", got[6]
        else:
            assert got[6]["fell_back"] == 0 and got[6]["live_chunks"] >= 2 and got[6]["chunks"] == (len(stream) + (ck << 10) - 1) // (ck << 10), (ck, got[6])
    za = product()
    for name, bad in (("inflate_par_chunk_kib", 3), ("inflate_par_chunk_kib", 65537), ("inflate_par_repair_pct", -1), ("inflate_par_min_kib", -1)):
        with pytest.raises(za.ZadaError):
            par.set_knob(name, bad)


def test_markers_through_copies_of_copies(par):
    """The streams of _inflate_par.marker_streams (the CPU test holds the model to the same record): references into earlier chunks, through
    copies of copies; the 64 KiB period lies outside Deflate's window and has none."""
    par.set_knob("inflate_par_chunk_kib", 4)
    for name, (data, stream, markers) in P.marker_streams().items():
        got = _par(par, stream, len(data))
        assert got[:5] == (0, data, len(data), len(stream), zlib.crc32(data) ^ 0xFFFFFFFF), (name, got[6])
        assert got[6]["fell_back"] == 0 and got[6]["live_chunks"] >= 2, (name, got[6])
        assert (got[6]["marker_bytes"] > 0) == markers, (name, got[6])
        assert got[6] == P.model_inflate_par(stream, len(data), 4)[6], name


def test_a_planted_false_positive(par):
    par.set_knob("inflate_par_chunk_kib", 4)
    inner, outer = P.planted_false_positive()
    got = _par(par, outer, len(inner))
    assert got[:5] == (0, inner, len(inner), len(outer), zlib.crc32(inner) ^ 0xFFFFFFFF), got[6]
    assert got[6]["repairs"] >= 1 and got[6]["fell_back"] == 0, got[6]


def test_pointer_contract(par, streams):
    par.set_knob("inflate_par_chunk_kib", 4)
    picks = [x for x in streams if x[0] in ("sample_pgm_100k.bin/zlib9.0", "sample.jpg/zlib0.0", "sample_pgm_100k.bin/oracle10", "sample.xls/zlib6.2", "sample.jpg/zlib6.3",
                                            "sample_pgm_100k.bin/zlib1.0")]
    assert len(picks) == 6
    rng = np.random.default_rng(5)
    for label, data, stream in picks:
        assert len(stream) > 8192, label
        for a in range(16):
            a_out = (a * 7 + 3) % 16
            start = int(rng.integers(0, 1 << 32))
            got = _par(par, stream, len(data), a, a_out, start)
            assert got[:5] == (0, data, len(data), len(stream), zlib.crc32(data, start ^ 0xFFFFFFFF) ^ 0xFFFFFFFF), (label, a, got[6])
            assert got[6]["fell_back"] == 0 and got[6]["live_chunks"] >= 2, (label, a, got[6])
            # one byte short: the one wave's verdict and text, nothing delivered, the register as it was
            short = _par(par, stream, len(data) - 1, a, a_out, start)
            assert short[0] == E_DATA and short[2:5] == (0, 0, start) and short[6]["fell_back"] == 1 and short[6]["reason"] == "damaged", (label, a, short[6])
            assert short[5] == _one_wave(par, stream, len(data) - 1, a, a_out, start)[5] and "output beyond cap" in short[5], (label, a)
    # argument checks come first
    assert par.lib.zada_inflate_par_device(par.ctx, 8, None, 5, None, 0, None, None, None) == -1
    assert par.lib.zada_inflate_par_device(par.ctx, 8, 16, 5, 16, (1 << 64) - 8, None, None, None) == -4


DAMAGED_TIME_LIMIT = 300          # seconds for the child process of the damaged streams


def test_damaged_streams_equal_the_cpu_model():
    """Every tenth case of the damaged corpus at 4 KiB chunks, one call each: rc, bytes written, input used and CRC equal the CPU model's of the
    one-wave decoder and the guard bytes are intact.  An error-path test on inputs the same logic has survived on a CPU under ASan + UBSan; it runs
    once, in a child process of its own under its own time limit, and nothing here runs it again if it fails."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import test_gpu_inflate_par as t; t._damaged_main()" % here
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=DAMAGED_TIME_LIMIT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "damaged streams ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _damaged_main():
    za = product()
    enc = za.Encoder(0)
    enc.set_knob("inflate_par_chunk_kib", 4)
    cases, _ = _inflate.damaged_corpus()
    n_ok = n_par = 0
    for k in range(0, len(cases), 10):
        s, cap = cases[k]
        rc, out, ol, used, reg, rule = model_inflate(s, cap, 8)
        if len(s) == 0:
            assert enc.lib.zada_inflate_par_device(enc.ctx, 8, None, 0, None, 0, None, None, None) == E_DATA
            continue
        got = _par(enc, s, cap, k % 16, (k // 16) % 16)
        assert got[:5] == (rc, out, ol, used, reg if rc == 0 else 0xFFFFFFFF), (k, rule, got[5], got[6])
        if rc:
            assert rule in got[5] and got[6]["fell_back"] == 1, (k, rule, got[5], got[6])
        else:
            n_ok += 1
            n_par += not got[6]["fell_back"]
    assert n_ok > 1000 and n_par > 100, (n_ok, n_par)
    enc.close()
    print("damaged streams ok: %d accepted, %d of them in parallel" % (n_ok, n_par))


def _archive_entries():
    mix = silesia_mix(5 << 20, version=2)
    ents = [("big/three_mib.bin", mix[:3 << 20])]
    ents += [("small/%02d.txt" % i, mix[(3 << 20) + i * 5000:(3 << 20) + i * 5000 + 300 + 233 * i]) for i in range(20)]
    ents += [("big/secret.bin", mix[3 << 20:4 << 20]), ("big/damaged.bin", mix[4 << 20:5 << 20])]
    return ents, ("stored.bin", mix[1000:41000])


def _flip(arc, info, name):
    """One bit of the entry's payload flipped, near its middle: the first place where zlib then refuses the stream (a DataError) or decodes as many
    bytes as before (a CRCError) -- not fewer or more, which would be a SizeError."""
    e = info[name]
    for pos in range(e.data_offset + e.csize // 2, e.data_offset + e.csize):
        b = bytearray(arc)
        b[pos] ^= 0x10
        try:
            ok = len(zlib.decompressobj(-15).decompress(bytes(b[e.data_offset:e.data_offset + e.csize]), e.usize + 1)) == e.usize
        except zlib.error:
            ok = True
        if ok:
            return bytes(b)
    raise AssertionError("no such place")


@pytest.mark.parametrize("writer", ("ZipCreate", "zipfile"))
def test_unzip_with_parallel_inflate(par, writer):
    """One archive with a 3 MiB Deflate entry, twenty small ones, a stored one, an encrypted large one (ZipCreate only: zipfile writes no encrypted
    entries) and a large one with a flipped payload byte: UnZip (parallel_inflate=64) gives what the default gives, entry for entry and error for
    error, and the record shows that the large entries went the parallel way."""
    import torch
    za = product()
    ents, stored = _archive_entries()
    if writer == "ZipCreate":
        zc = za.ZipCreate(par, za.Method.Deflate_3)
        for nm, d in ents:
            zc.add_stream(nm, d, password=PW if nm == "big/secret.bin" else None)
        zc.add_compressed(stored[0], stored[1], zlib.crc32(stored[1]), len(stored[1]), 0)
        arc = zc.finish()
        large = ["big/three_mib.bin", "big/secret.bin", "big/damaged.bin"]
    else:
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w", zipfile.ZIP_DEFLATED) as z:
            for nm, d in ents:
                z.writestr(nm, d)
            z.writestr(zipfile.ZipInfo(stored[0]), stored[1], compress_type=zipfile.ZIP_STORED)
        arc = b.getvalue()
        large = ["big/three_mib.bin", "big/secret.bin", "big/damaged.bin"]
    arc = _flip(arc, za.ZipInfo.load(arc), "big/damaged.bin")
    info = za.ZipInfo.load(arc)
    assert all(info[nm].csize >= 64 << 10 for nm in large) and all(e.csize < 64 << 10 for e in info.entries if e.name not in large and e.method == 8)
    t = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).cuda()
    dinfo = za.ZipInfo.load_device(t)
    plain, fast = za.UnZip(par), za.UnZip(par, parallel_inflate=64)
    want = plain.extract(info, password=PW, errors="collect")
    assert type(want["big/damaged.bin"]) in (za.CRCError, za.DataError) and want["big/three_mib.bin"] == ents[0][1] and want[stored[0]] == stored[1]

    def same(got, device):
        assert list(got) == list(want)
        for nm, w in want.items():
            g = got[nm]
            if isinstance(w, Exception):
                assert type(g) is type(w) and str(g) == str(w), (nm, g, w)
            else:
                assert (bytes(g.cpu().numpy()) if device else g) == w, nm
    same(fast.extract(info, password=PW, errors="collect"), False)
    assert [nm for nm, _ in fast.last_parallel] == large
    for nm, rec in fast.last_parallel:
        assert rec["streams"] == 1 and (rec["fell_back"] == 0 and rec["live_chunks"] >= 2 or nm == "big/damaged.bin"), (nm, rec)
    same(plain.extract_device(dinfo, password=PW, errors="collect"), True)
    same(fast.extract_device(dinfo, password=PW, errors="collect"), True)
    rec = par.inflate_par_last()
    assert rec["streams"] == 3 and rec["fell_back"] <= 1 and rec["live_chunks"] >= 4, rec
    with pytest.raises(type(want["big/damaged.bin"])) as a:
        fast.extract_device(dinfo, password=PW)
    assert str(a.value) == str(want["big/damaged.bin"])
    # the knob is off again behind the call, and the default reader never set it
    plain.extract_device(dinfo, password=PW, errors="collect")
    assert par.inflate_par_last() == rec


def test_one_stream_at_size(par):
    """16 MiB of the corpus, written on the device with Deflate_3 and read back with the default chunk size: bytes and CRC against the input."""
    import torch
    za = product()
    data = silesia_mix(16 << 20, version=2)
    t_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    t_z = torch.empty(len(data) + 64, dtype=torch.uint8, device="cuda")
    t_out = torch.full((len(data) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, zl, reg = par.deflate_device(t_in.data_ptr(), len(data), t_z.data_ptr(), len(data) + 64, za.Method.Deflate_3)
    assert rc == 0 and reg ^ 0xFFFFFFFF == zlib.crc32(data)
    ol, used, reg2 = par.inflate_par_device(t_z.data_ptr(), zl, t_out.data_ptr() + 16, len(data))
    rec = par.inflate_par_last()
    assert (ol, used, reg2) == (len(data), zl, reg), rec
    assert rec["fell_back"] == 0 and rec["live_chunks"] >= 40 and rec["chunks"] == (zl + (DEFAULT_CHUNK_KIB << 10) - 1) // (DEFAULT_CHUNK_KIB << 10), rec
    host = t_out.cpu().numpy()
    assert host[16:16 + len(data)].tobytes() == data
    assert (host[:16] == 0xA5).all() and (host[16 + len(data):] == 0xA5).all()
