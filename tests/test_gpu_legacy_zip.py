"""Shrink_1 and Reduce_1 .. _4 through Compress_Data and Zip.Create: compress_data with and without a password against the ZipCrypto model
(tests/crypt/crypt_model.c) over the CPU models' streams, with the Store fallback where the stream does not beat the input; a ZipCreate archive of
the five methods read back by ZipInfo.load and decoded by the models' decoders."""
import zlib

import pytest

import _crypt
import _legacy as L
from _common import product

gpu = pytest.mark.gpu
METHODS = (1, 2, 3, 4, 5)
H11 = bytes(range(101, 112))


_inputs = L.zip_inputs


def _decode(payload, zt, usize):
    return payload if zt == 0 else L.unshrink(payload, usize) if zt == 1 else L.unreduce(payload, zt - 1, usize)


@gpu
def test_compress_data_plain_and_encrypted(encoder):
    stored = 0
    for method in METHODS:
        for d in _inputs():
            rc, stream, _ = L.model_result(d, method)
            crc = zlib.crc32(d) & 0xFFFFFFFF
            want = (stream, crc, method) if rc == 0 else (d, crc, 0)                   # zip_type: 1 Shrink, 2 .. 5 Reduce by factor, 0 stored
            stored += rc
            assert encoder.compress_data(d, method) == want, (method, len(d))
            hdr, kept = _crypt.header(_crypt.init_keys("legacy pw"), H11, crc)
            assert encoder.compress_data(d, method, password="legacy pw", header=H11) == (hdr + _crypt.encode(kept, want[0])[0], crc, want[2]), (method, len(d))
    assert stored >= 3 * len(METHODS)                                                  # the random, the empty and the one-byte input


@gpu
def test_zipcreate_archive_of_the_five_methods(encoder):
    za = product()
    datas = _inputs()
    for method in METHODS:
        zc = za.ZipCreate(encoder, method)
        nm = ["m%d/e%d.bin" % (method, i) for i in range(len(datas))]
        zc.add_stream(nm[0], datas[0])                                                 # Add_Stream, then the rest as one batch per method
        zc.add_streams(nm[1:], datas[1:])
        arc = zc.finish()
        one = za.ZipCreate(encoder, method)
        for n_, d in zip(nm, datas):
            one.add_stream(n_, d)
        assert one.finish() == arc, method                                             # the batch writes what entry after entry writes
        info = za.ZipInfo.load(arc)
        assert [e.name for e in info.entries] == nm
        for e, d in zip(info.entries, datas):
            rc = L.model_result(d, method)[0]
            assert e.method == (method if rc == 0 else 0) and e.usize == len(d) and e.crc == zlib.crc32(d) & 0xFFFFFFFF, (method, e.name)
            payload = arc[e.data_offset:e.data_offset + e.csize]
            assert _decode(payload, e.method, e.usize) == d, (method, e.name)
    # ... and with a password: the same entries, encrypted by one crypt_encode_batch
    zc = za.ZipCreate(encoder, za.Method.Reduce_4)
    zc.add_streams(["p%d" % i for i in range(len(datas))], datas, password="legacy pw", _headers=[H11] * len(datas))
    info = za.ZipInfo.load(zc.finish())
    assert all(e.flags & 1 for e in info.entries) and [e.csize for e in info.entries] == [12 + len(encoder.compress_data(d, 5)[0]) for d in datas]
