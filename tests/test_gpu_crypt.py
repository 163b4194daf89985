"""ZipCrypto on the GPU (csrc/zada_crypt.hip) against the byte-serial CPU model (tests/crypt/crypt_model.c, pinned by zipfile and unzip in
test_crypt_model.py): Encode over one buffer, in pieces, over a batch of buffers; Compress_Data with a password; encrypted archives."""
import io
import os
import shutil
import struct
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

import _crypt
from _common import GOLDEN, oracle_deflate, oracle_zip, product, silesia_mix

pytestmark = pytest.mark.gpu

KEYS = [(0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x12345678, 0x23456789, 0x34567890), (0x9E3779B9, 0x7F4A7C15, 0xDEADBEEF)]
LENGTHS = (0, 1, 255, 256, 257, 16383, 16384, 16385, (1 << 20) + 3)
BIG = (64 << 20) + 5
PW = "p\xe4ss \xff"


def _h11(seed):
    return bytes(np.random.RandomState(seed).randint(0, 256, 11).astype(np.uint8))


@pytest.fixture(scope="module")
def mix():
    return silesia_mix(BIG)


def test_encode_equals_the_model(encoder, mix):
    for n in LENGTHS:
        for content in (bytes(n), b"\xa7" * n, mix[:n]):
            for keys in KEYS:
                assert encoder.crypt_encode(keys, content) == _crypt.encode(keys, content), (n, keys)
    # 64 MiB + 5: several strips of the scan over the tiles (4 097 tiles)
    for content, keys in ((mix, KEYS[2]), (mix, KEYS[1]), (bytes(BIG), KEYS[0])):
        got = encoder.crypt_encode(keys, content)
        want = _crypt.encode(keys, content)
        assert got[1] == want[1] and got[0] == want[0], keys


def test_encode_in_pieces_host_and_device(encoder, mix):
    import torch
    for piece, n in ((1 << 20, (5 << 20) + 77), (4097, (1 << 20) + 3), (12, 5000), (1, 600)):
        data = mix[1000:1000 + n]
        keys = KEYS[3]
        want, kw = _crypt.encode(keys, data)
        k, out = keys, []
        for o in range(0, n, piece):
            ct, k = encoder.crypt_encode(k, data[o:o + piece])
            out.append(ct)
        assert b"".join(out) == want and k == kw, piece
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        k = keys
        for o in range(0, n, piece):                       # (pieces at every alignment of the device address)
            k = encoder.crypt_encode_device(k, t.data_ptr() + o, min(piece, n - o))
        assert k == kw and bytes(t.cpu().numpy()) == want, piece
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        assert encoder.crypt_encode_device(keys, t.data_ptr(), n) == kw and bytes(t.cpu().numpy()) == want
    assert encoder.crypt_encode_device(KEYS[3], None, 0) == KEYS[3]


def test_batch_equals_the_model_per_entry(encoder, mix):
    rng = np.random.default_rng(5)
    lens = [int(x) for x in rng.integers(0, 40001, 5000)]
    for i in (0, 17, 18, 2500, 4999):
        lens[i] = 0
    lens[1234] = 8 << 20
    lens[3000] = 300000                                    # (longer than one wave takes, shorter than a piece of the tiled path)
    datas, off = [], 0
    for ln in lens:
        datas.append(mix[off:off + ln]); off = (off + ln) % (len(mix) - (9 << 20))
    ks = rng.integers(0, 1 << 32, (len(lens), 3), dtype=np.uint64)
    keys = [tuple(int(x) for x in row) for row in ks]
    got = encoder.crypt_encode_batch(keys, datas)
    assert len(got) == len(datas)
    for i, (k, d, g) in enumerate(zip(keys, datas, got)):
        assert g == _crypt.encode(k, d), (i, len(d))
    assert encoder.crypt_encode_batch([], []) == []
    assert encoder.crypt_encode_batch([KEYS[1]], [b""]) == [(b"", KEYS[1])]


def _inputs(mix):
    return {"empty": b"", "one": b"x", "random_4096": bytes(np.random.RandomState(3).randint(0, 256, 4096).astype(np.uint8)),
            "mix_1m": mix[:1 << 20], "sample.jpg": open(os.path.join(GOLDEN, "sample.jpg"), "rb").read()}


# Deflate_Fixed, Deflate_3, Deflate_R, BZip2_3, LZMA_1, LZMA_3, LZMA_for_JPEG
@pytest.mark.parametrize("method", (6, 10, 11, 14, 16, 18, 23))
def test_compress_data_with_a_password(encoder, mix, method):
    for i, (name, data) in enumerate(_inputs(mix).items()):
        h11 = _h11(method * 10 + i)
        want, crc, zt, attempt = _crypt.compress_data_pw(data, method, PW, h11)
        got = encoder.compress_data(data, method, password=PW, header=h11)
        assert got[1] == crc and got[2] == zt and got[0] == want, (name, method)
        assert crc == zlib.crc32(data) & 0xFFFFFFFF
        if name == "random_4096":                          # inefficient for every method: Store from the kept keys, n + 12 bytes behind the same header
            assert zt == 0 and len(got[0]) == len(data) + 12 and got[0][:12] == attempt[:12], method


def test_compress_data_with_a_password_preselection_and_store(encoder, mix):
    za = product()
    C = za.ContentType
    for i, (name, data) in enumerate(_inputs(mix).items()):
        hint = C.JPEG if name == "sample.jpg" else C.neutral
        h11 = _h11(500 + i)
        want, crc, zt, _ = _crypt.compress_data_pw(data, za.Method.Preselection_2, PW, h11, content_hint=hint)
        assert encoder.compress_data(data, za.Method.Preselection_2, content_hint=hint, password=PW, header=h11) == (want, crc, zt), name
        want, crc, zt, _ = _crypt.compress_data_pw(data, 0, PW.encode("latin-1"), h11)
        assert encoder.compress_data(data, za.Method.Store, password=PW.encode("latin-1"), header=h11) == (want, crc, 0) and zt == 0, name
    with pytest.raises(za.ZadaError):
        encoder.compress_data(b"abc", 10, password=b"")


def _entries(mix):
    return [("a/text.txt", silesia_mix(200000, class_mask=1)), ("b\\rand.bin", bytes(np.random.RandomState(3).randint(0, 256, 3000).astype(np.uint8))),
            ("empty", b""), ("mix.bin", mix[:600000]), ("one", b"z")]


def _with_password(plain, payloads):
    """The archive `plain` (no Zip_64 records) with every entry's payload replaced and Encryption_Flag_Bit set: flag, sizes, offsets and payload change,
    nothing else does."""
    zf = zipfile.ZipFile(io.BytesIO(plain))
    infos = zf.infolist()
    out, cd, offs = bytearray(), bytearray(), []
    for info, payload in zip(infos, payloads):
        o = info.header_offset
        nl, el = struct.unpack_from("<HH", plain, o + 26)
        assert el == 0
        hdr = bytearray(plain[o:o + 30 + nl])
        flag, = struct.unpack_from("<H", hdr, 6)
        struct.pack_into("<H", hdr, 6, flag | 1)
        struct.pack_into("<I", hdr, 18, len(payload))
        offs.append(len(out))
        out += hdr + payload
    p = zf.start_dir
    for info, payload, off in zip(infos, payloads, offs):
        nl, el, cl = struct.unpack_from("<HHH", plain, p + 28)
        rec = bytearray(plain[p:p + 46 + nl + el + cl])
        flag, = struct.unpack_from("<H", rec, 8)
        struct.pack_into("<H", rec, 8, flag | 1)
        struct.pack_into("<I", rec, 20, len(payload))
        struct.pack_into("<I", rec, 42, off)
        cd += rec
        p += len(rec)
    end = bytearray(plain[p:])
    assert end[:4] == b"PK\x05\x06"
    struct.pack_into("<I", end, 16, len(out))
    return bytes(out + cd + end)


@pytest.mark.parametrize("method", (10, 8))
def test_encrypted_archives(encoder, mix, method):
    za = product()
    entries = _entries(mix)
    heads = [_h11(900 + i) for i in range(len(entries))]
    one = za.ZipCreate(encoder, method)
    for (name, data), h in zip(entries, heads):
        one.add_stream(name, data, password=PW, _header=h)
    one = one.finish()
    many = za.ZipCreate(encoder, method)
    many.add_streams([e[0] for e in entries], [e[1] for e in entries], password=PW, _headers=heads)
    assert many.finish() == one
    # the archive without a password is today's (the oracle's); with one, its flag, sizes, offsets and payloads change and nothing else
    plain = za.ZipCreate(encoder, method)
    plain.add_streams([e[0] for e in entries], [e[1] for e in entries])
    plain = plain.finish()
    assert plain == oracle_zip(entries, method)
    model = [_crypt.compress_data_pw(d, method, PW, h) for (_, d), h in zip(entries, heads)]
    assert one == _with_password(plain, [m[0] for m in model])
    zf, zp = zipfile.ZipFile(io.BytesIO(one)), zipfile.ZipFile(io.BytesIO(plain))
    kinds = set()
    for (name, data), info, pinfo, m in zip(entries, zf.infolist(), zp.infolist(), model):
        assert info.flag_bits & 1 and info.flag_bits == pinfo.flag_bits | 1 and info.compress_size == pinfo.compress_size + 12 == len(m[0])
        assert info.CRC == zlib.crc32(data) & 0xFFFFFFFF == pinfo.CRC and info.extract_version == 10 and info.compress_type == m[2]
        assert zf.read(info, pwd=PW.encode("latin-1")) == data, name
        kinds.add((info.compress_type, len(data) == 0))
    assert (8, False) in kinds and (0, False) in kinds and (0, True) in kinds          # Deflate, stored by fallback, empty


def test_encrypted_bzip2_and_lzma_entries_open_in_zipfile(encoder, mix):
    za = product()
    data = mix[:150000]
    for method, zt in ((za.Method.BZip2_3, 12), (za.Method.LZMA_3, 14)):
        zc = za.ZipCreate(encoder, method)
        zc.add_streams(["x.bin", "y.bin"], [data, data[:40000]], password=b"pw-\x80\xfe", _headers=[_h11(1), _h11(2)])
        zf = zipfile.ZipFile(io.BytesIO(zc.finish()))
        assert [i.compress_type for i in zf.infolist()] == [zt, zt] and all(i.flag_bits & 1 for i in zf.infolist())
        assert zf.read("x.bin", pwd=b"pw-\x80\xfe") == data and zf.read("y.bin", pwd=b"pw-\x80\xfe") == data[:40000]


@pytest.mark.skipif(shutil.which("unzip") is None, reason="unzip is not installed")
def test_encrypted_archive_opens_in_unzip(encoder, mix, tmp_path):
    za = product()
    entries = _entries(mix)
    zc = za.ZipCreate(encoder, za.Method.Deflate_3)
    zc.add_streams([e[0] for e in entries], [e[1] for e in entries], password="unzip-pw")
    p = tmp_path / "gpu.zip"
    p.write_bytes(zc.finish())
    r = subprocess.run(["unzip", "-P", "unzip-pw", "-t", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "No errors detected" in r.stdout, r.stdout + r.stderr
    assert subprocess.run(["unzip", "-P", "not-it", "-t", str(p)], capture_output=True, text=True, timeout=120).returncode != 0
    zf = zipfile.ZipFile(io.BytesIO(p.read_bytes()))          # (random header bytes: os.urandom)
    assert all(zf.read(i, pwd=b"unzip-pw") == d for i, (_, d) in zip(zf.infolist(), entries))


def test_without_a_password_nothing_changes(encoder, mix):
    za = product()
    for name, data in _inputs(mix).items():
        rc, ref, crc = oracle_deflate(data, 10)
        want = (ref, crc ^ 0xFFFFFFFF, 8) if rc == 0 else (data, crc ^ 0xFFFFFFFF, 0)
        assert encoder.compress_data(data, 10) == want, name
        assert encoder.compress_data(data, 10, password=None, header=_h11(1)) == want, name
    entries = _entries(mix)
    zc = za.ZipCreate(encoder, 10)
    for name, data in entries:
        zc.add_stream(name, data, password=None)
    assert zc.finish() == oracle_zip(entries, 10)
