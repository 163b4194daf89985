"""ZipInfo.load_device on cpu tensors against ZipInfo.load of the same bytes: the entries field by field, the comment, and the text of the errors.
No GPU: the tensor is only where the bytes are fetched from."""
import io
import zipfile

import numpy as np
import pytest

from _common import oracle_zip_compressed, product, silesia_mix
from test_zipinfo import _Unseekable, _datas, _zipfile_archive

FIELDS = ("name", "raw_name", "method", "flags", "crc", "csize", "usize", "header_offset", "data_offset", "dos_time", "encrypted")


def _tensor(archive):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(archive), dtype=np.uint8).copy()) if len(archive) else torch.zeros(0, dtype=torch.uint8)


class _Counting:
    """What load_device asks the tensor for: every slice and every gather, by the bytes it fetches."""

    def __init__(self, t):
        self.t, self.fetched, self.gathers = t, 0, 0

    def run(self, za):
        import torch
        real = torch.Tensor.__getitem__
        me = self

        def spy(tensor, key):
            out = real(tensor, key)
            if tensor is me.t:
                me.fetched += out.numel()
                me.gathers += isinstance(key, torch.Tensor)
            return out
        torch.Tensor.__getitem__ = spy
        try:
            return za.ZipInfo.load_device(self.t)
        finally:
            torch.Tensor.__getitem__ = real


def _same(archive):
    za = product()
    want = za.ZipInfo.load(archive)
    t = _tensor(archive)
    got = za.ZipInfo.load_device(t)
    assert got.data is None and got.device_data is t and want.device_data is None
    assert got.comment == want.comment and len(got.entries) == len(want.entries)
    for a, b in zip(got.entries, want.entries):
        for f in FIELDS:
            assert getattr(a, f) == getattr(b, f), (b.name, f)
    return got


def _streamed():
    w = _Unseekable()
    with zipfile.ZipFile(w, "w", zipfile.ZIP_DEFLATED) as z:
        for nm, d in _datas():
            z.writestr(nm, d)
    return bytes(w.b)


def test_load_device_equals_load():
    deflated = _zipfile_archive(zipfile.ZIP_DEFLATED)
    assert len(_same(deflated).entries) == 4
    _same(_zipfile_archive(zipfile.ZIP_STORED))
    assert _same(_zipfile_archive(zipfile.ZIP_DEFLATED, comment=b"a comment with PK\x05\x06 inside it")).comment.startswith(b"a comment")
    _same(_zipfile_archive(zipfile.ZIP_DEFLATED, comment=b"c" * 65535))
    assert all(e.flags & 8 for e in _same(_streamed()).entries)
    _same(_zipfile_archive(zipfile.ZIP_DEFLATED, force64=True))
    got = _same(b"\x3c" * 100 + deflated)                       # 100 bytes prepended: the shift the end record implies
    assert got.entries[0].header_offset == 100
    b = io.BytesIO()
    zipfile.ZipFile(b, "w").close()
    assert _same(b.getvalue()).entries == []                   # an empty archive
    # Zip64 end record and locator with offsets beyond 4 GiB (the archive was cut out of a larger file)
    import zlib
    ents = []
    for nm, d in _datas():
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        ents.append((nm, c.compress(d) + c.flush(), zlib.crc32(d), len(d), 8))
    _same(oracle_zip_compressed(ents, bias=2 ** 32 + 12345))


def test_load_device_fetches_the_directory_only():
    za = product()
    big = [("big%d.bin" % k, silesia_mix(300000, seed=k)) for k in range(3)]
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w", zipfile.ZIP_STORED) as z:
        for nm, d in big:
            z.writestr(nm, d)
    arc = b.getvalue()
    c = _Counting(_tensor(arc))
    info = c.run(za)
    assert len(info.entries) == 3 and c.gathers == 1           # the local headers in one gather
    assert c.fetched < 2 * (22 + 65535) + 90 + 2000, c.fetched  # the tail, the locator's place, the directory, three local headers: not the 900 000 bytes of data


def test_load_device_raises_what_load_raises():
    za = product()
    good = _zipfile_archive(zipfile.ZIP_DEFLATED)
    eocd = good.rfind(b"PK\x05\x06")
    cd = good.find(b"PK\x01\x02")
    bad = [b"", b"PK", good[:eocd], good[:eocd + 10], good[:-1],                               # the end record is cut
           good[:cd + 2] + b"xx" + good[cd + 4:],                                              # damaged central header
           good[:cd + 28] + b"\xff\xff" + good[cd + 30:],                                      # name length beyond the directory
           good[:eocd + 10] + (500).to_bytes(2, "little") + good[eocd + 12:],                  # more entries than there are
           good[:cd + 42] + (2 ** 31).to_bytes(4, "little") + good[cd + 46:],                  # local header offset beyond the file
           good[:cd + 20] + (2 ** 30).to_bytes(4, "little") + good[cd + 24:],                  # the data lie beyond the file
           good[:eocd + 16] + (2 ** 32 - 1).to_bytes(4, "little") + good[eocd + 20:],          # directory offset beyond the file
           good[:eocd + 12] + (2 ** 31).to_bytes(4, "little") + good[eocd + 16:],              # directory size beyond the file
           good[:2] + b"zz" + good[4:], bytes(100), good[eocd:]]
    texts = set()
    for k, a in enumerate(bad):
        with pytest.raises(za.ZadaError) as want:
            za.ZipInfo.load(a)
        with pytest.raises(za.ZadaError) as got:
            za.ZipInfo.load_device(_tensor(a))
        assert str(got.value) == str(want.value) and type(got.value) is type(want.value), k
        texts.add(str(want.value).split(":")[1].strip()[:20])
    assert len(texts) >= 5                                      # (the cases do raise different things)
    rng = np.random.default_rng(6)
    for _ in range(400):                                        # random damage in the directory: the same outcome either way
        b = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(cd, len(b)))] = int(rng.integers(0, 256))
        try:
            want = [tuple(getattr(e, f) for f in FIELDS) for e in za.ZipInfo.load(bytes(b)).entries]
        except za.ZadaError as ex:
            with pytest.raises(za.ZadaError) as got:
                za.ZipInfo.load_device(_tensor(b))
            assert str(got.value) == str(ex)
        else:
            assert [tuple(getattr(e, f) for f in FIELDS) for e in za.ZipInfo.load_device(_tensor(b)).entries] == want
    import torch
    for t in (torch.zeros(4, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)[::2], b"bytes"):
        with pytest.raises(za.ZadaError):
            za.ZipInfo.load_device(t)
