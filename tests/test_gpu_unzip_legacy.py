"""Archives with Shrink, Reduce and Implode entries through UnZip / CompZip / FindZip (encoder, legacy=True): PKZIP's own streams put into an
archive by ZipCreate.add_compressed, and the archives ZipCreate writes under Shrink_1 and Reduce_1 .. _4, with and without a password."""
import zlib

import numpy as np
import pytest

import _legacy as L
import _unlegacy as U
from _common import product

pytestmark = pytest.mark.gpu
PW = "legacy p\xe4ss"


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope="module")
def plain():
    row, payload = U.fixtures()[0]
    return U.host_decode(row["format"], row["flags"], payload, row["size"])[1]


@pytest.fixture(scope="module")
def pkzip_archive(encoder, plain):
    """PKZIP's seven streams and a stored entry: (archive bytes, {name: plaintext})."""
    za = product()
    zc = za.ZipCreate(encoder, za.Method.Store)
    want = {}
    for row, payload in U.fixtures():
        zc.add_compressed(row["file"], payload, int(row["crc32"], 16), row["size"], row["format"], flag_bits=row["flags"])
        want[row["file"]] = plain
    zc.add_stream("stored.txt", plain[:5000])
    want["stored.txt"] = plain[:5000]
    return zc.finish(), want


def _own_archive(encoder, password):
    """What ZipCreate writes under Shrink_1 and Reduce_1 .. _4 (entries the method does not shrink are stored): (archive bytes, {name: data})."""
    za = product()
    datas = L.zip_inputs()
    want = {}
    zc = za.ZipCreate(encoder, za.Method.Shrink_1)
    for method in (1, 2, 3, 4, 5):
        zc.method = method                                  # (Zip.Create's Set (Info, New_Method) between two entries)
        names = ["m%d/e%d.bin" % (method, i) for i in range(len(datas))]
        zc.add_streams(names, datas, password=password)
        want.update(zip(names, datas))
    return zc.finish(), want


@pytest.mark.parametrize("password", (None, PW))
def test_extract_and_extract_device(encoder, pkzip_archive, password):
    za = product()
    for arc, want in ([pkzip_archive] if password is None else []) + [_own_archive(encoder, password)]:
        info = za.ZipInfo.load(arc)
        assert {e.method for e in info.entries} >= ({0, 1, 2, 3, 4, 5, 6} if len(want) == 8 else {0, 1, 2, 3, 4, 5})
        got = za.UnZip(encoder, legacy=True).extract(info, password=password)
        assert got == want
        assert za.UnZip(encoder, legacy=True).extract(info, password=password, test_only=True) == {nm: None for nm in want}
        dinfo = za.ZipInfo.load_device(_dev(arc))
        dgot = za.UnZip(encoder, legacy=True).extract_device(dinfo, password=password)
        assert {nm: bytes(t.cpu().numpy()) for nm, t in dgot.items()} == want
        assert za.UnZip(encoder, legacy=True).extract_device(dinfo, password=password, test_only=True) == {nm: None for nm in want}
        # the knob is set around the call only
        with pytest.raises(za.ZadaError):
            tab = np.zeros(1, dtype=encoder.unzip_dtypes()[0])
            tab["method"], tab["n_in"] = 1, 4
            encoder.unzip_device(dinfo.device_data.data_ptr(), dinfo.device_data.numel(), None, 0, tab, None)
        assert b"unknown method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)" in encoder.lib.zada_last_error(encoder.ctx)


def test_wrong_password(encoder):
    za = product()
    arc, want = _own_archive(encoder, PW)
    for info, call in ((za.ZipInfo.load(arc), "extract"), (za.ZipInfo.load_device(_dev(arc)), "extract_device")):
        res = getattr(za.UnZip(encoder, legacy=True), call)(info, password="not it", errors="collect")
        bad = [nm for nm, v in res.items() if isinstance(v, za.WrongPassword)]
        assert len(bad) >= len(want) - 1, (call, len(bad))          # (one header in 256 ends in the check byte by chance)
        with pytest.raises(za.WrongPassword):
            getattr(za.UnZip(encoder, legacy=True), call)(info, password="not it")


def test_one_flipped_payload_bit_is_that_entry_alone(encoder, pkzip_archive):
    za = product()
    arc, want = pkzip_archive
    info = za.ZipInfo.load(arc)
    for e in info.entries:
        if e.method == 0:
            continue
        b = bytearray(arc)
        b[e.data_offset + e.csize // 2] ^= 0x10
        for inf, call in ((za.ZipInfo.load(bytes(b)), "extract"), (za.ZipInfo.load_device(_dev(b)), "extract_device")):
            res = getattr(za.UnZip(encoder, legacy=True), call)(inf, errors="collect")
            assert isinstance(res[e.name], (za.DataError, za.CRCError, za.SizeError)), (e.name, call, res[e.name])
            if isinstance(res[e.name], za.DataError):
                assert ("not a valid %s stream" % za.UnZip._STREAMS[e.method]) in str(res[e.name])
            for nm, v in res.items():
                if nm != e.name:
                    assert (v if call == "extract" else bytes(v.cpu().numpy())) == want[nm], (e.name, nm, call)


def test_without_the_keyword_nothing_changed(encoder, pkzip_archive):
    za = product()
    arc, want = pkzip_archive
    for info, call in ((za.ZipInfo.load(arc), "extract"), (za.ZipInfo.load_device(_dev(arc)), "extract_device")):
        res = getattr(za.UnZip(encoder), call)(info, errors="collect")
        for e in info.entries:
            if e.method == 0:
                assert (res[e.name] if call == "extract" else bytes(res[e.name].cpu().numpy())) == want[e.name]
            else:
                assert isinstance(res[e.name], za.UnsupportedMethod) and "Store, Deflate and Deflate64 only" in str(res[e.name])
        with pytest.raises(za.UnsupportedMethod, match="Shrink"):
            getattr(za.UnZip(encoder, bzip2=True, lzma=True), call)(info, what="many_formats_05_pk090.bin")
    dinfo = za.ZipInfo.load_device(_dev(arc))
    with pytest.raises(za.UnsupportedMethod):
        za.CompZip(encoder).compare_device(dinfo, dinfo)
    with pytest.raises(za.UnsupportedMethod):
        za.FindZip(encoder).find_device(dinfo, b"the")
    with pytest.raises(za.UnsupportedMethod):
        za.ReZip(encoder).rezip_device(dinfo)


def _stored_copy(encoder, want):
    za = product()
    zc = za.ZipCreate(encoder, za.Method.Store)
    for nm, d in want.items():
        zc.add_stream(nm, d)
    return zc.finish()


def test_compzip_and_findzip(encoder, pkzip_archive):
    za = product()
    arc, want = pkzip_archive
    own, own_want = _own_archive(encoder, None)
    for a, w in ((arc, want), (own, own_want)):
        stored = _stored_copy(encoder, w)
        i1, i2 = za.ZipInfo.load_device(_dev(a)), za.ZipInfo.load_device(_dev(stored))
        out = za.CompZip(encoder, legacy=True).compare_device(i1, i2)
        assert out.total_differences == 0 and out.common == len(w) and out.total_bytes == sum(len(d) for d in w.values())
        # one byte changed in the stored copy of one entry: "Difference at position p"
        name = sorted(w, key=lambda nm: -len(w[nm]))[0]
        changed = dict(w)
        p = len(w[name]) // 3
        changed[name] = w[name][:p] + bytes([w[name][p] ^ 1]) + w[name][p + 1:]
        out = za.CompZip(encoder, legacy=True).compare_device(i1, za.ZipInfo.load_device(_dev(_stored_copy(encoder, changed))))
        assert out.total_differences == 1 and out.compare_failures == 1
        assert out[name][1] == za.CZ_DIFFERENT and out[name][2] == p + 1
        # Find_Zip counts in the legacy archive what it counts in the stored copy
        text = w[name][100:108]
        f1 = za.FindZip(encoder, legacy=True).find_device(i1, text)
        f2 = za.FindZip(encoder).find_device(i2, text)
        assert f1.damaged == f2.damaged == 0 and [(e[0], e[1], e[2]) for e in f1.entries] == [(e[0], e[1], e[2]) for e in f2.entries]
        assert sum(e[1] for e in f1.entries) >= 1
