"""zada_zip_device_ex with the knob "zip_legacy": Shrink_1 and Reduce_1 .. _4 from device memory into an archive in device memory.  The reference
is never the code under test: the archive is what ZipCreate (encoder, method).add_streams + finish write from host bytes (the host-pointer batch
calls, pinned to the CPU models by test_gpu_shrink.py / test_gpu_reduce.py), and every delivered stream is held against the CPU model's closed form
(tests/legacy/) directly as well."""
import io
import shutil
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

import _legacy as L
from _common import product
from _devbuf import GUARD
from _zip_legacy import NAMES, knobs, model_stream
from _zipdev import E_INVALID, CallEx, check_equal, headers_for, host_archive, names_for, same_results

pytestmark = pytest.mark.gpu
METHODS = (1, 2, 3, 4, 5)
PW = "legacy p\xe4ss"
EDGES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 5999, 6000, 6001, 8999, 9000, 9001, 16384, 65535, 65536)


_inputs = []


def inputs():
    """40 entries, none above 64 KiB: every edge size cut from text with matches and 144s in it, the named inputs of the encoders' tests, and random
    bytes (incompressible: the Store fallback) at four sizes."""
    if not _inputs:
        si, ri = L.shrink_inputs(), L.reduce_inputs()
        rb = lambda seed, n: L.rnd(seed, n, bytes(range(256)))
        _inputs.extend([L.edge_input(n) for n in EDGES])
        _inputs.extend([si["abcd_48k"], si["sym16_96k"][:40000], si["random_16k"], ri["words_24k"], ri["runs_A_90"], ri["far_repeats"], ri["abcd_12k"]])
        _inputs.extend([rb(41, 63), rb(42, 257), rb(43, 6000), rb(44, 9001)])
        _inputs.extend(L.zip_inputs())
        _inputs.extend([L.edge_input(n, seed=3) for n in (5, 300, 700, 2500, 4097)])
        assert len(_inputs) == 40 and max(len(d) for d in _inputs) == 65536
    return _inputs


def streams_are_the_models(archive, res, names, datas, method, base=0, encrypted=False):
    """every result row against the CPU model: zip type (the method's, or 0 where the stream does not beat its input), CRC, csize; the entries lie one
    behind the other; and, unencrypted, the delivered bytes are the model's.  -> how many entries are stored"""
    stored, pos, x = 0, 0, 12 if encrypted else 0
    for k, (r, nm, d) in enumerate(zip(res, names, datas)):
        rc, s, reg = model_stream(d, method)
        payload = d if rc else s
        assert int(r["crc"]) == reg ^ 0xFFFFFFFF == zlib.crc32(d), k
        assert (int(r["zip_type"]), int(r["csize"]), int(r["offset"])) == (0 if rc else method, len(payload) + x, base + pos), (k, len(d))
        at = pos + 30 + len(nm.encode("utf-8"))
        if not encrypted:
            assert archive[at:at + len(payload)] == payload, k
        pos = at + x + len(payload)
        stored += rc
    return stored


def test_knob(encoder):
    """Off: the refusal of before, nothing written.  On: taken.  Off again: refused again.  zada_zip_device refuses whatever the knob says."""
    datas = [L.edge_input(700), L.edge_input(3000), b""]
    names = names_for(datas)
    c = CallEx(encoder, names, datas)
    cap = c.bound()

    def refused(ex_text="Deflate_Fixed .. Preselection_2 (6 .. 35)"):
        for method in (1, 2, 5):
            rc, _, _, buf, said = c.run(method, cap)
            assert rc == E_INVALID and said == "zada_zip_device_ex: method %d (%s) is not one it takes: Store (0), %s" % (method, NAMES[method], ex_text)
            assert bool((buf == GUARD).all())

    refused()
    with knobs(encoder, zip_legacy=1):
        for method in (1, 2, 5):
            rc, alen, res, buf, said = c.run(method, cap)
            assert rc == 0 and alen > 0 and [int(r["zip_type"]) for r in res] == [0 if model_stream(d, method)[0] else method for d in datas], said
            rc, _, _, buf, said = c.run(method, cap, old=True)
            assert rc == E_INVALID and "zada_zip_device: method %d (%s) is not one it takes: Store (0), Deflate_Fixed .. Deflate_R (6 .. 11)" % (method, NAMES[method]) == said
            assert bool((buf == GUARD).all())
        rc, _, _, buf, said = c.run(36, cap)
        assert rc == E_INVALID and "method 36 (unknown) is not one it takes" in said and bool((buf == GUARD).all())
        # an entry of 1 GiB - 64 KiB: refused with its index before anything is read or written
        tab = c.tab.copy()
        tab[1]["d_data"], tab[1]["n"] = 1 << 20, (1 << 30) - 65536          # (an address far from the archive buffer; the checks come first)
        rc, _, _, buf, said = c.run(5, cap, tab=tab)
        assert rc == -4 and "entry 1:" in said and bool((buf == GUARD).all()), said
    refused()
    with pytest.raises(Exception):
        encoder.set_knob("zip_legacy", 2)


@pytest.mark.parametrize("method", METHODS)
def test_bytes(encoder, method):
    """40 entries at every source alignment 0 .. 15, the archive at an odd address behind an odd archive_base: the archive equals add_streams + finish
    byte for byte, the delivered streams are the CPU model's, the result rows are right; and once more in several groups (batch_mib = 1,
    reduce_group_mib = 1: two or three Reduce entries per group), the same bytes."""
    datas = inputs()
    names = names_for(datas)
    base = 77
    want, entries = host_archive(encoder, method, names, datas, base=base, key=("legacy", method))
    c = CallEx(encoder, names, datas, a_arc=3, a_in=[k % 16 for k in range(len(datas))])
    assert c.bound(base) >= len(want)
    with knobs(encoder, zip_legacy=1):
        rc, alen, res, buf, said = c.run(method, len(want), base=base)
    assert rc == 0, said
    assert alen == len(want) and buf.tobytes() == want
    same_results(res, entries, datas)
    stored = streams_are_the_models(want, res, names, datas, method, base=base)
    assert 6 <= stored <= 20, stored                               # the Store fallback is among them, and so are real streams
    with knobs(encoder, zip_legacy=1, batch_mib=1, reduce_group_mib=1):
        rc, alen, res2, buf, said = c.run(method, len(want), base=base)
        marks = dict(encoder.last_timing())
    assert rc == 0, said
    assert alen == len(want) and buf.tobytes() == want and res2.tobytes() == res.tobytes()
    assert "zip:k_zw_pack" in marks and "k_batch_crc" in marks


def test_single_path(encoder):
    """A call of one entry runs alone (zx_single: no gather, the stream written behind its local header).  So does a middle entry that no group can
    hold: with batch_mib = 1 a Shrink entry of 520 KiB, whose two slots alone pass the limit -- the one entry above 64 KiB in these tests, since no
    smaller one can be alone between two groups at the smallest value the knobs take; it is highly compressible and Shrink_1's wave takes a fifth of
    a second for it."""
    for method in (1, 5):
        for d in (L.edge_input(3000), L.rnd(50, 500, bytes(range(256))), b""):
            with knobs(encoder, zip_legacy=1):
                check_equal(encoder, method, ["one.bin"], [d], a_arc=5, too_small=bool(d))
            assert "zip:k_zw_pack" not in dict(encoder.last_timing())
    big = (L.shrink_inputs()["abcd_128k"] * 5)[:520 << 10]
    datas = [L.edge_input(5000), L.edge_input(700), big, L.edge_input(6000), L.edge_input(64)]
    with knobs(encoder, zip_legacy=1, batch_mib=1):
        want, entries, res = check_equal(encoder, 1, names_for(datas), datas, a_arc=1, too_small=False)
    assert [int(r["zip_type"]) for r in res] == [0 if model_stream(d, 1)[0] else 1 for d in datas] and int(res[2]["zip_type"]) == 1
    assert model_stream(big, 1)[1] == want[entries[2]["offset"] + 30 + len(names_for(datas)[2]):][:entries[2]["csize"]]


@pytest.mark.parametrize("method", (1, 5))
def test_capacity(encoder, method):
    """cap exact succeeds, one byte less is "archive buffer too small", in a batch and in a call of one; the guard bytes on both sides stay (CallEx)."""
    datas = [L.edge_input(2500), L.rnd(51, 800, bytes(range(256))), b"", L.edge_input(9000), b"q"]
    with knobs(encoder, zip_legacy=1):
        check_equal(encoder, method, names_for(datas), datas, a_arc=7, too_small=True)
        # a call of one whose stream alone does not fit: legacy_device_one's "output buffer too small" is the writer's text
        c = CallEx(encoder, ["x"], [datas[3]])
        rc, _, _, _, said = c.run(method, 31 + 100)
        assert rc == E_INVALID and said == "zada_zip_device_ex: archive buffer too small"


@pytest.mark.parametrize("method", (1, 5))
def test_password(encoder, method):
    datas = inputs()[:20] + [L.rnd(52, 3000, bytes(range(256)))]
    names = names_for(datas)
    hs = headers_for(len(datas))
    with knobs(encoder, zip_legacy=1):
        want, entries, res = check_equal(encoder, method, names, datas, a_arc=9, password=PW, headers=hs, too_small=False)
        check_equal(encoder, method, names[3:4], datas[3:4], password=PW, headers=hs[3:4], too_small=True)      # ... and the single path
    assert streams_are_the_models(want, res, names, datas, method, encrypted=True) >= 3
    read = 0
    with zipfile.ZipFile(io.BytesIO(want)) as z:                   # zipfile decrypts; it decodes the stored entries only
        for nm, d, info in zip(names, datas, z.infolist()):
            if info.compress_type == 0:
                assert z.read(info, pwd=PW.encode("latin-1")) == d, nm
                read += 1
    assert read >= 3
    if method == 1 and shutil.which("unzip"):                      # Info-ZIP reads Shrink
        import os
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "a.zip")
            with open(p, "wb") as f:
                f.write(want)
            r = subprocess.run(["unzip", "-t", "-P", PW.encode("latin-1"), p], capture_output=True, timeout=60)
            assert r.returncode == 0, r.stdout[-400:]


@pytest.mark.parametrize("password", (None, PW))
def test_read_back(encoder, password):
    """ZipInfo.load_device + UnZip (legacy=True).extract_device return every input, from the archive as it lies in device memory"""
    za = product()
    datas = inputs()[:24]
    names = names_for(datas)
    for method in (1, 3, 5):
        c = CallEx(encoder, names, datas)
        cap = c.bound(0, password is not None)
        with knobs(encoder, zip_legacy=1):
            rc, alen, res, buf, said = c.run(method, cap, password=password, headers=headers_for(len(datas)) if password else None)
        assert rc == 0, said
        info = za.ZipInfo.load_device(c.t_arc[c.a_arc:c.a_arc + alen])
        assert {e.method for e in info.entries} == {0, method}
        got = za.UnZip(encoder, legacy=True).extract_device(info, password=password)
        assert [bytes(got[nm].cpu().numpy()) for nm in names] == datas


def test_python(encoder):
    import torch
    za = product()
    datas = inputs()[4:16]
    names = names_for(datas)
    tensors = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() if d else torch.empty(0, dtype=torch.uint8, device="cuda") for d in datas]
    for method, password in ((1, None), (5, None), (5, PW)):
        hs = headers_for(len(datas)) if password else None
        want, entries = host_archive(encoder, method, names, datas, password=password, headers=hs)
        zc = za.ZipCreate(encoder, method)
        out = zc.write_device_ex(names, tensors, password=password, _headers=hs, legacy=True)
        assert bytes(out.cpu().numpy()) == want and zc.entries == entries
        # the knob was set around the call only: the plain call refuses as before
        with pytest.raises(za.ZadaError, match=r"method %d \(%s\) is not one it takes: Store \(0\), Deflate_Fixed \.\. Preselection_2" % (method, NAMES[method])):
            za.ZipCreate(encoder, method).write_device_ex(names, tensors, password=password, _headers=hs)
