"""One large Deflate64 stream on many waves (csrc/zada_inflate_par.hip with the knob "inflate_par_deflate64") through the C ABI: against the
one-wave decoder (zada_inflate_device, format 9) and the input, with the record of every call asserted next to the bytes -- what
test_inflate_par64_model.py shows the CPU model to do on the same streams (_deflate64.py) --, so that a silent hand-over to the one wave cannot
pass as success.  Device buffers come from _devbuf.py: the input ends at its last byte, the output has guard bytes on both sides."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import _deflate64 as D
import _inflate_par as P8
import _inflate_par64 as P
from _common import product
from _devbuf import device_call
from _inflate import E_DATA

pytestmark = pytest.mark.gpu
KNOB = "inflate_par_deflate64"


@pytest.fixture()
def par(encoder):
    """The session's encoder with the knobs of the parallel path at their defaults before and after."""
    def reset():
        encoder.set_knob("inflate_par_chunk_kib", 64)
        encoder.set_knob("inflate_par_repair_pct", P8.REPAIR_PCT)
        encoder.set_knob("inflate_par_min_kib", 0)
        if _has_knob(encoder):
            encoder.set_knob(KNOB, 0)
    reset()
    yield encoder
    reset()


def _has_knob(enc):
    return enc.lib.zada_set_knob(enc.ctx, KNOB.encode(), 0) == 0


def _call(entry, enc, fmt, stream, cap, a_in=0, a_out=0, crc=0xFFFFFFFF):
    """entry (zada_inflate_par_device or zada_inflate_device) on guarded buffers -> (rc, bytes, out_len, in_used, crc register, error text)"""
    ol, iu, reg = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(crc)

    def fn(d_in, n, d_out, cap):
        return entry(enc.ctx, fmt, d_in, n, d_out, cap, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg))
    rc, out = device_call(fn, stream, cap, a_in, a_out)
    return rc, out[:ol.value], ol.value, iu.value, reg.value, enc.lib.zada_last_error(enc.ctx).decode()


def _par(enc, stream, cap, a_in=0, a_out=0, crc=0xFFFFFFFF, fmt=9):
    return _call(enc.lib.zada_inflate_par_device, enc, fmt, stream, cap, a_in, a_out, crc) + (enc.inflate_par_last(),)


def _one_wave(enc, stream, cap, a_in=0, a_out=0, crc=0xFFFFFFFF, fmt=9):
    return _call(enc.lib.zada_inflate_device, enc, fmt, stream, cap, a_in, a_out, crc)


def test_knob_off_is_the_one_wave(par):
    data, stream, _, _ = D.streams()["period_49152"]
    assert par.inflate_par(stream, len(data), format=9) == (data, len(stream), zlib.crc32(data) ^ 0xFFFFFFFF)
    rec = par.inflate_par_last()
    assert rec["fell_back"] == 1 and rec["reason"] == "format" and rec["streams"] == 1, rec
    got = _par(par, stream, len(data))
    assert got[:5] == _one_wave(par, stream, len(data))[:5] and got[1] == data and got[6]["reason"] == "format", got[6]


@pytest.mark.parametrize("chunk_kib", P.CHUNKS_KIB)
@pytest.mark.parametrize("name", ("period_49152", "period_65000", "far_first", "near_first"))
def test_parity_with_the_one_wave(par, name, chunk_kib):
    """zada_inflate_par_device with the knob set equals zada_inflate_device (format 9) in rc, bytes, out_len, in_used and CRC register, the bytes
    are the input, and the record is the CPU model's."""
    par.set_knob(KNOB, 1)
    par.set_knob("inflate_par_chunk_kib", chunk_kib)
    data, stream, _, _ = D.streams()[name]
    got = _par(par, stream, len(data))
    info = got[6]
    assert got[:5] == (0, data, len(data), len(stream), zlib.crc32(data) ^ 0xFFFFFFFF), info
    assert got[:5] == _one_wave(par, stream, len(data))[:5]
    assert info["streams"] == 1 and info["chunks"] == (len(stream) + (chunk_kib << 10) - 1) // (chunk_kib << 10), info
    assert info["fell_back"] == 0 and info["reason"] == "none" and info["live_chunks"] >= 2 and info["marker_bytes"] > 0, info
    assert info["repairs"] <= info["chunks"] * P8.REPAIR_PCT // 100 + 2 and info["scout_rounds"] == 1 + info["repairs"], info
    model = P.model_inflate_par64(stream, len(data), chunk_kib)[6]
    model.pop("live_bytes")
    assert info == model


def test_pointer_contract(par):
    par.set_knob(KNOB, 1)
    par.set_knob("inflate_par_chunk_kib", 4)
    for name in ("far_first", "near_first"):
        data, stream, _, _ = D.streams()[name]
        for a_in, a_out, start in ((0, 0, 0xFFFFFFFF), (3, 1, 0x12345678), (1, 5, 0x9E3779B9)):
            got = _par(par, stream, len(data), a_in, a_out, start)          # cap exact; device_call asserts the guard bytes on both sides
            assert got[:5] == (0, data, len(data), len(stream), zlib.crc32(data, start ^ 0xFFFFFFFF) ^ 0xFFFFFFFF), (name, a_out, got[6])
            assert got[6]["fell_back"] == 0 and got[6]["live_chunks"] >= 2, (name, a_out, got[6])
            # one byte short: the one wave's verdict and text, nothing delivered, the register as it was
            short = _par(par, stream, len(data) - 1, a_in, a_out, start)
            want = _one_wave(par, stream, len(data) - 1, a_in, a_out, start)
            assert short[0] == E_DATA and short[:6] == want and short[2:5] == (0, 0, start), (name, a_out, short[5], want[5])
            assert short[6]["fell_back"] == 1 and short[6]["reason"] == "damaged", (name, a_out, short[6])
    # the host-pointer form and the Python layer
    data, stream, _, _ = D.streams()["period_65000"]
    assert par.inflate_par(stream, len(data), format=9) == (data, len(stream), zlib.crc32(data) ^ 0xFFFFFFFF)
    rec = par.inflate_par_last()
    assert rec["fell_back"] == 0 and rec["live_chunks"] >= 2 and rec["marker_bytes"] > 0, rec
    assert par.inflate_par(stream, len(data), format=9, crc=0x0BADF00D)[2] == zlib.crc32(data, 0x0BADF00D ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
    za = product()
    for bad in (-1, 2):
        with pytest.raises(za.ZadaError):
            par.set_knob(KNOB, bad)


def test_damaged_streams_equal_the_one_wave(par):
    """60 of the damaged cases of near_first, all four kinds of damage: verdict, bytes, lengths, register and error text are the one wave's, and a
    refused stream is always the one wave's to judge."""
    par.set_knob(KNOB, 1)
    par.set_knob("inflate_par_chunk_kib", 4)
    picked = D.gpu_damaged_picks()
    assert len(picked) == 60
    n_bad = n_par = 0
    for j, s, cap in picked:
        assert len(s) > 0
        got = _par(par, s, cap, j % 16, (j // 16) % 16)
        want = _one_wave(par, s, cap, j % 16, (j // 16) % 16)
        assert got[:5] == want[:5], (j, got[6])
        if got[0]:
            assert got[0] == E_DATA and got[5] == want[5] and got[6]["fell_back"] == 1, (j, got[5], want[5], got[6])
            n_bad += 1
        n_par += not got[6]["fell_back"]
    assert n_bad > 60 // 10 and n_par > 60 // 20, (n_bad, n_par)          # (the shares the CPU test asserts, on all 2 000 and on these 60)


def test_deflate_is_untouched_by_the_knob(par):
    data = P8.corpus_2m()
    stream = par.deflate(data, 10)[0]
    par.set_knob("inflate_par_chunk_kib", 4)
    off = _par(par, stream, len(data), fmt=8)
    par.set_knob(KNOB, 1)
    on = _par(par, stream, len(data), fmt=8)
    assert off[:5] == (0, data, len(data), len(stream), zlib.crc32(data) ^ 0xFFFFFFFF) and on == off
    assert on[6]["fell_back"] == 0 and on[6]["live_chunks"] >= 2, on[6]


def _zip_of(entries):
    """entries: [(name, payload, method, data)] -> one archive, its headers written here"""
    body, cd = b"", b""
    for name, payload, method, data in entries:
        nm, crc = name.encode(), zlib.crc32(data)
        cd += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 21, 21, 0, method, 0, 0x21, crc, len(payload), len(data), len(nm), 0, 0, 0, 0, 0, len(body)) + nm
        body += struct.pack("<IHHHHHIIIHH", 0x04034B50, 21, 0, method, 0, 0x21, crc, len(payload), len(data), len(nm), 0) + nm + payload
    return body + cd + struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, len(entries), len(entries), len(cd), len(body), 0)


def test_unzip_with_parallel_deflate64(par):
    """A stored entry, a small Deflate64 entry and period_65000 as a method 9 entry: UnZip (parallel_inflate=64, parallel_deflate64=True) gives
    what the default reader gives through extract and extract_device, and the records show one stream on the parallel path."""
    import torch
    za = product()
    big, big_s, _, _ = D.streams()["period_65000"]
    small = big[3000:9000] + big[:5000]
    small_s = D.deflate64(small, 700)
    stored = big[100:30100]
    arc = _zip_of([("stored.bin", stored, 0, stored), ("small.d64", small_s, 9, small), ("big/period_65000.d64", big_s, 9, big)])
    info = za.ZipInfo.load(arc)
    assert [(e.method, e.csize >= 64 << 10) for e in info.entries] == [(0, False), (9, False), (9, True)]
    dinfo = za.ZipInfo.load_device(torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).cuda())
    want = za.UnZip(par).extract(info)
    assert want == {"stored.bin": stored, "small.d64": small, "big/period_65000.d64": big}
    on_host = lambda got: {nm: bytes(t.cpu().numpy()) for nm, t in got.items()}
    with pytest.raises(za.ZadaError):
        za.UnZip(par, parallel_deflate64=True)
    fast = za.UnZip(par, parallel_inflate=64, parallel_deflate64=True)
    assert fast.extract(info) == want
    assert [nm for nm, _ in fast.last_parallel] == ["big/period_65000.d64"]
    rec = fast.last_parallel[0][1]
    assert rec["streams"] == 1 and rec["fell_back"] == 0 and rec["live_chunks"] >= 2 and rec["marker_bytes"] > 0, rec
    assert on_host(fast.extract_device(dinfo)) == want
    rec = par.inflate_par_last()
    assert rec["streams"] == 1 and rec["fell_back"] == 0 and rec["live_chunks"] >= 2 and rec["marker_bytes"] > 0, rec
    # without the keyword no Deflate64 entry goes that way
    deflate_only = za.UnZip(par, parallel_inflate=64)
    assert deflate_only.extract(info) == want and deflate_only.last_parallel == []
    assert on_host(deflate_only.extract_device(dinfo)) == want
    assert par.inflate_par_last()["streams"] == 0, par.inflate_par_last()
    # the knob is back at 0 behind the calls
    par.inflate_par(big_s, len(big), format=9)
    assert par.inflate_par_last()["reason"] == "format"
