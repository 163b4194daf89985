"""GPU tests of the fifteen data-type LZMA methods (LZMA_Method'Pos 19 .. 33: their own lc, lp, pb, zip-compress-lzma_e.adb:121-143) and of
the Preselection methods in ZipCreate.  The expected payload of an entry is built from the oracle's LZMA.Encoding.Encode with the method's
parameters, transcribed below from the Ada file: the bytes 16 2 5 0 (:155-158), then the stream with an end marker and dictionary_size = the
entry's size; "inefficient" when it is not shorter than the entry (zip-compress.adb:479-486); the CRC from zlib."""
import io
import os
import zipfile
import zlib

import pytest

from _common import GOLDEN, product, silesia_mix, oracle_zip_compressed
from _lzmah import lz_inputs, oracle_lzma, oracle_lzma_encode, lzma_decode, lzma_symbols

pytestmark = pytest.mark.gpu

# zip-compress-lzma_e.adb:121-143: method'Pos -> (lc, lp, pb, level)
PARAMS = {
    19: (8, 4, 0, 2), 20: (8, 4, 0, 3),      # LZMA_2 / _3_for_Zip_in_Zip
    21: (3, 0, 0, 2), 22: (3, 0, 0, 3),      # LZMA_2 / _3_for_Source
    23: (8, 0, 0, 2),                        # LZMA_for_JPEG
    24: (8, 4, 4, 2),                        # LZMA_for_ARW
    25: (8, 0, 0, 0),                        # LZMA_for_ORF
    26: (8, 4, 4, 2), 27: (8, 4, 4, 2),      # LZMA_for_MP3 / _MP4
    28: (8, 0, 0, 0),                        # LZMA_for_PGM
    29: (4, 0, 0, 2),                        # LZMA_for_PPM
    30: (8, 0, 2, 2),                        # LZMA_for_PNG
    31: (0, 0, 0, 1),                        # LZMA_for_GIF
    32: (0, 1, 1, 2),                        # LZMA_for_WAV
    33: (0, 2, 2, 2),                        # LZMA_for_AU
}
NEW = sorted(PARAMS)


def golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def expected(data, method):
    """(rc, payload, CRC register) of Zip.Compress.LZMA_E for one of the new methods."""
    if method not in PARAMS:
        return oracle_lzma(data, method)
    lc, lp, pb, level = PARAMS[method]
    s, _ = oracle_lzma_encode(data, level, lc, lp, pb)
    z = bytes([16, 2, 5, 0]) + s
    return (1 if len(z) >= len(data) else 0), z, zlib.crc32(data) ^ 0xFFFFFFFF


def matrix(method):
    cases = {k: v for k, v in lz_inputs().items() if len(v) <= (110000 if PARAMS[method][3] >= 2 else 400000)}
    for g in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin"):
        cases[g] = golden(g)
    return cases


@pytest.fixture(scope="module")
def enc():
    Z = product()
    e = Z.Encoder(0)
    yield e
    e.close()


@pytest.mark.parametrize("method", NEW)
def test_batch_of_every_new_method_equals_the_oracle(enc, method):
    """One zada_lzma_batch per method over the parity inputs and the three golden samples: payload, rc, CRC, the props byte lc + 9 lp + 45 pb."""
    cases = matrix(method)
    names = sorted(cases)
    res = enc.lzma_batch([cases[k] for k in names], method)
    lc, lp, pb, _ = PARAMS[method]
    for name, (rc, z, crc) in zip(names, res):
        d = cases[name]
        orc, oz, ocrc = expected(d, method)
        assert (rc, crc) == (orc, ocrc), (name, method)
        assert z == oz, (name, method, len(z or b""), len(oz))
        assert z[4] == lc + 9 * lp + 45 * pb
    if method == 23:                         # near the inefficiency line: sample.jpg is 65 188 of 65 278 bytes, compressed and not stored
        rc, z, _ = res[names.index("sample.jpg")]
        assert rc == 0 and len(z) == 65188


def test_streams_of_the_new_methods_decode(enc):
    """sample.xls and 16 KiB of the mixed corpus under every new method decode to the input: the plain decoder (any lc / lp / pb) and, where
    lc + lp <= 4, liblzma."""
    datas = [golden("sample.xls"), silesia_mix(16384)]
    for method in NEW:
        lc, lp, _, _ = PARAMS[method]
        for d, (rc, z, crc) in zip(datas, enc.lzma_batch(datas, method)):
            assert z is not None
            assert lzma_symbols(z[4:])[0] == d, method
            if lc + lp <= 4:
                assert lzma_decode(z, 4) == d, method


# every (home of the literal table, level) pair of the table: PGM (HBM, 0), GIF (LDS, 1), WAV (LDS, 2), JPEG (HBM, 2), 3_for_Source (LDS, 3),
# 3_for_Zip_in_Zip (HBM, 3)
SINGLES = (28, 31, 32, 23, 22, 20)


def test_single_calls_in_bounded_launches_with_feedback_and_abort(enc):
    """zada_lzma in launches of 777 and 20 000 positions (the HBM table waits between them) and zada_lzma_device: the oracle's payload;
    feedback monotone 0 .. 100; after an abort the context codes the next stream right."""
    import torch
    Z = product()
    d = silesia_mix(60000, seed=5)
    t = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    out = torch.empty(len(d) + 4096, dtype=torch.uint8, device="cuda")
    try:
        for method in SINGLES:
            want = expected(d, method)
            for chunk in (777, 20000):
                enc.set_knob("lzma_chunk", chunk)
                seen = []
                assert enc.lzma(d, method, feedback=lambda pct: seen.append(pct) and False) == want, (method, chunk)
                assert seen[0] == 0 and seen[-1] == 100 and seen == sorted(seen) and len(seen) > 3, (method, chunk)
            rc, ln, crc = enc.lzma_device(t.data_ptr(), len(d), out.data_ptr(), out.numel(), method)
            torch.cuda.synchronize()
            assert (rc, bytes(out[:ln].cpu().numpy()), crc) == want, method
            enc.set_knob("lzma_chunk", 5000)
            with pytest.raises(Z.UserAbort):
                enc.lzma(d, method, feedback=lambda pct: pct >= 40)
            assert enc.lzma(d[:30000], method) == expected(d[:30000], method), method
    finally:
        enc.set_knob("lzma_chunk", 0)


def test_one_stream_on_four_waves_and_on_one(enc):
    """LZMA_3_for_Zip_in_Zip (HBM table: the helpers read wave 0's updates in device memory) and LZMA_3_for_Source on 256 KiB of the
    benchmark corpus, with the helper waves and without."""
    d = silesia_mix(256 * 1024, version=2)
    try:
        for method in (20, 22):
            want = expected(d, method)
            for waves in (4, 1):
                enc.set_knob("lzma_waves", waves)
                assert enc.lzma(d, method) == want, (method, waves)
    finally:
        enc.set_knob("lzma_waves", 0)


def test_a_batch_split_by_the_literal_table_knob_gives_the_same_bytes(enc):
    """lzma_lit_mib = 1: every entry of an HBM-table batch is a launch group of its own; the bytes are the default's."""
    datas = [silesia_mix(3000 + 1000 * k, seed=k) for k in range(6)]
    for method in (24, 23):
        base = enc.lzma_batch(datas, method)
        try:
            enc.set_knob("lzma_lit_mib", 1)
            assert enc.lzma_batch(datas, method) == base
        finally:
            enc.set_knob("lzma_lit_mib", 12288)
        assert base == [expected(d, method) for d in datas]


def test_export_and_import_of_the_new_methods():
    """A stopped LZMA_3_for_Source stream (table in LDS) goes on in another context; an LZMA_3 state is refused by an LZMA_3_for_Source call
    (same level, other pb); export after a stream whose table is in HBM is refused.  The contexts stay usable."""
    Z = product()
    d = silesia_mix(200000, version=2)
    want = expected(d, 22)
    a = Z.Encoder(0)
    b = Z.Encoder(0)
    try:
        for e in (a, b):
            e.set_knob("lzma_chunk", 20000)
        with pytest.raises(Z.UserAbort):
            a.lzma(d, 22, feedback=lambda pct: pct >= 40)
        state, head, pos = a.lzma_export_state(len(d) + 4096)
        assert 0 < pos < len(d)
        b.lzma_import_state(state)
        rc, z, crc = b.lzma(d, 22)
        assert (rc, head + z[len(head):], crc) == want
        # an LZMA_3 state met by an LZMA_3_for_Source call
        with pytest.raises(Z.UserAbort):
            a.lzma(d, 18, feedback=lambda pct: pct >= 40)
        state3, _, _ = a.lzma_export_state(len(d) + 4096)
        b.lzma_import_state(state3)
        with pytest.raises(Z.ZadaError, match="imported state"):
            b.lzma(d, 22)
        assert b.lzma(d, 22) == want
        # a stream whose literal table is in HBM: bounded launches and abort work, its state is not exported
        with pytest.raises(Z.UserAbort):
            a.lzma(d, 20, feedback=lambda pct: pct >= 40)
        with pytest.raises(Z.ZadaError, match="HBM"):
            a.lzma_export_state(len(d) + 4096)
        assert a.lzma(d[:50000], 20) == expected(d[:50000], 20)
        assert a.lzma(d[:50000], 22) == expected(d[:50000], 22)
    finally:
        a.close()
        b.close()


def presel_entries():
    """Names and sizes that reach every branch of Compress_Data's Preselection (zip-compress.adb:266-325)."""
    jpg, pgm, xls = golden("sample.jpg"), golden("sample_pgm_100k.bin"), golden("sample.xls")
    mix = lambda n, s: silesia_mix(n, seed=s)
    return [
        ("a.jpg", jpg), ("a_small.JPG", jpg[:2000]), ("b.PNG", mix(5000, 1)), ("c.adb", mix(12000, 2)), ("c_small.ads", mix(7000, 3)),
        ("c_big.cpp", mix(20000, 4)), ("d.htm", mix(9500, 5)), ("e.txt", mix(16000, 6)), ("e_mid.txt", mix(12000, 7)), ("e_small.txt", mix(8000, 8)),
        ("f.docx", xls), ("f_small.xlsx", xls[:900]), ("f_mid.zip", xls[:5000]), ("g.gif", mix(300, 9)), ("g2.gif", mix(400, 10)),
        ("h.wav", mix(6000, 11)), ("i.au", mix(6000, 12)), ("j.cr2", mix(4000, 13)), ("k.nef", mix(4000, 14)), ("l.mp3", mix(3000, 15)),
        ("m.mp4", mix(3000, 16)), ("n.pgm", pgm[:30000]), ("o.ppm", mix(5000, 17)), ("p.csv", mix(12000, 18)), ("p_small.json", mix(3000, 19)),
        ("q", mix(11000, 20)), ("r.bin", b""), ("s.log", mix(9500, 21)),
    ]


@pytest.mark.parametrize("presel", (34, 35))
def test_zip_create_with_preselection(enc, presel):
    """ZipCreate (Preselection_1 / _2): add_streams (grouped by method, one batch per group) == add_stream per entry == the oracle's archive of
    the expected per-entry payloads; zipfile reads back what zlib / bz2 / liblzma decode."""
    import bz2
    Z = product()
    ents = presel_entries()
    zc = Z.ZipCreate(enc, presel)
    zc.add_streams([n for n, _ in ents], [d for _, d in ents])
    many = zc.finish()
    zo = Z.ZipCreate(enc, presel)
    for n, d in ents:
        zo.add_stream(n, d)
    one = zo.finish()
    assert many == one
    want, used = [], set()
    for n, d in ents:
        m = Z.preselect(presel, Z.guess_type_from_name(n), len(d))
        used.add(m)
        if 15 <= m <= 33:
            rc, z, reg = expected(d, m)
            zt = 14
        elif 12 <= m <= 14:
            from _bzip2 import oracle_encode
            z, _ = oracle_encode(d, m - 12)
            rc, reg, zt = (1 if len(z) >= len(d) else 0), zlib.crc32(d) ^ 0xFFFFFFFF, 12
        else:
            from _common import oracle_deflate
            rc, z, reg = oracle_deflate(d, m)
            zt = 8
        if rc != 0:
            z, zt = d, 0
        want.append((n, z, reg ^ 0xFFFFFFFF, len(d), zt))
    assert many == oracle_zip_compressed(want)
    assert used == ({8, 10, 14, 17, 18, 19, 20, 21, 22} if presel == 35 else {8, 10, 17, 19, 21}) | set(range(23, 34)), sorted(used)
    zf = zipfile.ZipFile(io.BytesIO(many))
    for (n, d), info in zip(ents, zf.infolist()):
        assert info.filename == n
        if info.compress_type == zipfile.ZIP_LZMA:
            start = info.header_offset + 30 + len(n.encode())
            props = many[start + 4]
            if props % 9 + (props // 9) % 5 > 4:                  # (liblzma takes lc + lp <= 4 only: the plain decoder)
                assert lzma_symbols(many[start + 4:start + info.compress_size])[0] == d, n
                continue
        assert zf.read(info) == d, n
