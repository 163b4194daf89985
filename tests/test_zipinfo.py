"""ZipInfo.load (Zip.Load) against zipfile's reading of the same archives, and on damaged directories.  Pure Python: no GPU, no library."""
import io
import zipfile
import zlib

import pytest

from _common import oracle_zip, oracle_zip_compressed, product, silesia_mix


def _same(archive, n_expected=None):
    za = product()
    info = za.ZipInfo.load(archive)
    zl = zipfile.ZipFile(io.BytesIO(archive)).infolist()
    assert len(info.entries) == len(zl) and (n_expected is None or len(zl) == n_expected)
    for e, z in zip(info.entries, zl):
        assert (e.name, e.method, e.crc, e.csize, e.usize, e.header_offset, e.flags) == \
               (z.filename, z.compress_type, z.CRC, z.compress_size, z.file_size, z.header_offset, z.flag_bits), e.name
        assert e.encrypted == bool(z.flag_bits & 1)
    return info


def _datas():
    return [("a.txt", silesia_mix(5000, class_mask=1)), ("dir/b.bin", silesia_mix(70000)), ("empty", b""), ("ümläut-中.txt", b"x" * 300)]


def _zipfile_archive(method, comment=b"", force64=False):
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w", method) as z:
        for nm, d in _datas():
            if force64:
                zi = zipfile.ZipInfo(nm)
                zi.compress_type = method
                with z.open(zi, "w", force_zip64=True) as f:
                    f.write(d)
            else:
                z.writestr(nm, d)
        z.comment = comment
    return b.getvalue()


def test_zipfile_stored_and_deflated():
    for m in (zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED):
        info = _same(_zipfile_archive(m), 4)
        for e, (nm, d) in zip(info.entries, _datas()):
            raw = info.data[e.data_offset:e.data_offset + e.csize]
            assert (raw if m == zipfile.ZIP_STORED else zlib.decompress(raw, -15)) == d


def test_archive_comment():
    for c in (b"x", b"a comment with PK inside it", b"c" * 65535):
        assert _same(_zipfile_archive(zipfile.ZIP_DEFLATED, comment=c), 4).comment == c
    # a comment that holds an end record's signature (zipfile itself gives up on it): the record is the one whose comment ends with the file
    c = b"tricky PK\x05\x06 inside"
    info = product().ZipInfo.load(_zipfile_archive(zipfile.ZIP_DEFLATED, comment=c))
    assert info.comment == c and [e.name for e in info.entries] == [nm for nm, _ in _datas()]


def test_force_zip64_entries():
    info = _same(_zipfile_archive(zipfile.ZIP_DEFLATED, force64=True), 4)
    for e, (nm, d) in zip(info.entries, _datas()):
        assert zlib.decompress(info.data[e.data_offset:e.data_offset + e.csize], -15) == d


class _Unseekable(io.RawIOBase):
    def __init__(self):
        self.b = bytearray()

    def writable(self):
        return True

    def write(self, d):
        self.b += d
        return len(d)


def test_streamed_archive_has_bit_3_and_sizes_from_the_directory():
    w = _Unseekable()
    with zipfile.ZipFile(w, "w", zipfile.ZIP_DEFLATED) as z:
        for nm, d in _datas():
            z.writestr(nm, d)
    info = _same(bytes(w.b), 4)
    for e, (nm, d) in zip(info.entries, _datas()):
        assert e.flags & 8
        assert zlib.decompress(info.data[e.data_offset:e.data_offset + e.csize], -15) == d and e.crc == zlib.crc32(d)


def test_oracle_archives():
    _same(oracle_zip(_datas(), 8), 4)
    _same(oracle_zip([("only", b"")], 10), 1)
    _same(oracle_zip([], 10), 0)


def test_oracle_zip64_offset_bias():
    ents = []
    for nm, d in _datas():
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        p = c.compress(d) + c.flush()
        ents.append((nm, p, zlib.crc32(d), len(d), 8))
    for bias in (0, 2 ** 32 - 100, 2 ** 32 + 12345):
        # (zipfile refuses an archive whose Zip64 locator points beyond the file, so beyond bias 0 the entries are compared with what went in)
        arc = oracle_zip_compressed(ents, bias=bias)
        info = _same(arc, 4) if bias == 0 else product().ZipInfo.load(arc)
        assert len(info.entries) == 4
        for e, (nm, d), (_, p, crc, usize, zt) in zip(info.entries, _datas(), ents):
            assert (e.name, e.method, e.crc, e.csize, e.usize) == (nm, zt, crc, len(p), usize)
            assert info.data[e.header_offset:e.header_offset + 4] == b"PK\x03\x04"
            assert zlib.decompress(info.data[e.data_offset:e.data_offset + e.csize], -15) == d


def test_damaged_directories_raise_zada_error():
    za = product()
    good = _zipfile_archive(zipfile.ZIP_DEFLATED)
    eocd = good.rfind(b"PK\x05\x06")
    cd = good.find(b"PK\x01\x02")
    bad = [b"", b"PK", good[:eocd], good[:eocd + 10], good[:-1],
           good[:eocd + 16] + (2 ** 32 - 1).to_bytes(4, "little") + good[eocd + 20:],          # directory offset beyond the file
           good[:eocd + 12] + (2 ** 31).to_bytes(4, "little") + good[eocd + 16:],              # directory size beyond the file
           good[:cd + 2] + b"xx" + good[cd + 4:],                                              # damaged central header
           good[:cd + 28] + b"\xff\xff" + good[cd + 30:],                                      # name length beyond the directory
           good[:eocd + 10] + (500).to_bytes(2, "little") + good[eocd + 12:],                  # more entries than there are
           good[:cd + 42] + (2 ** 31).to_bytes(4, "little") + good[cd + 46:],                  # local header offset beyond the file
           bytes(100), good[eocd:]]
    for k, a in enumerate(bad):
        with pytest.raises(za.ZadaError):
            za.ZipInfo.load(a)
    import numpy as np
    rng = np.random.default_rng(5)
    for _ in range(3000):                                   # random damage in the directory: ZadaError or a directory, never another exception
        b = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(cd, len(b)))] = int(rng.integers(0, 256))
        try:
            za.ZipInfo.load(bytes(b))
        except za.ZadaError:
            pass
