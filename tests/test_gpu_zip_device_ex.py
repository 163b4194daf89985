"""zada_zip_device_ex (csrc/zada_zip.hip): the archive writer on device memory with BZip2, LZMA, Preselection_1 / _2 and passwords -- the C ABI at
unaligned addresses and at the exact capacity, groups with several methods, the out-of-place Encode, entries that run alone, the refusals -- and
ZipCreate.write_device_ex read back by ZipInfo.load_device / UnZip.extract_device and by zipfile.  The reference throughout is the host path on the
same encoder with the same encryption headers, ZipCreate.add_streams + finish; the entry point under test is never its own reference."""
import ctypes
import io
import zipfile

import numpy as np
import pytest

from _common import product
from _devbuf import GUARD
from _zipdev import (E_INVALID, E_TOO_LARGE, CallEx, check_equal, headers_for, host_archive, names_for, plain_list, same_results, text, zipfile_reads_back)

pytestmark = pytest.mark.gpu
MIB4 = 4 << 20
PW = "p\xe4ssword"
# BZip2_1, BZip2_3, LZMA_0, LZMA_1, LZMA_2, LZMA_3, LZMA_3_for_Source, LZMA_for_PNG (a literal table in HBM), Deflate_3
EQUAL_METHODS = (12, 14, 15, 16, 17, 18, 22, 30, 10)
LZMA_METHODS = tuple(range(15, 34))


@pytest.fixture(scope="module")
def plains():
    return plain_list()


@pytest.mark.parametrize("method", EQUAL_METHODS)
def test_archive_equality(encoder, plains, method):
    """Inputs at offsets (5 k + 3) mod 16, the archive at offsets 0, 1 and 15 mod 16, cap = archive_len exactly, guards and arena untouched (CallEx.run),
    cap - 1 refused.  100 000 bytes lie above BZip2_1's one-block limit (the single path inside a list) and below BZip2_3's (the batch)."""
    names = names_for(plains)
    for a_arc in (0, 1, 15):
        want, entries, res = check_equal(encoder, method, names, plains, a_arc=a_arc, key=("plains", method), too_small=a_arc == 1)
    zt = [int(x) for x in res["zip_type"]]
    own = 12 if method in (12, 14) else 8 if method == 10 else 14
    assert zt[0] == 0 and zt[-2] == 0, "an empty entry and 4 KiB of random bytes are stored"
    assert zt[-1] == own and zt[-3] == own
    assert [e["flag"] for e in entries] == [0x0800 | (0x0002 if t == 14 else 0) for t in zt]
    zipfile_reads_back(want, names, plains, [method] * len(plains), least=len(plains) if method != 30 else 5)


@pytest.mark.parametrize("method", LZMA_METHODS)
def test_every_lzma_method(encoder, method):
    t = text()
    datas = [b"", t[:255], t[5000:5000 + 32769], t[300000:320000]]
    check_equal(encoder, method, names_for(datas), datas, a_arc=3, too_small=False)


def presel_list():
    """Neighbours differ in method, and every branch of zada_preselect that yields another batch occurs."""
    t = text()
    rnd = np.random.default_rng(3).integers(0, 256, 5000, dtype=np.uint8).tobytes()
    ents = [("a.bin", t[:8000]), ("b.txt", t[300000:320000]), ("d.c", t[20000:32000]), ("c.bin", t[8000:19000]), ("e.gif", t[:300]), ("f.png", t[40000:45000]),
            ("g.gif", t[50000:55000]), ("h.jpg", t[60000:65000]), ("empty.txt", b""), ("i.zip", rnd), ("j.txt", t[320000:340000]), ("k.c", t[70000:82000])]
    return [e[0] for e in ents], [e[1] for e in ents]


@pytest.mark.parametrize("method", (34, 35))
def test_preselection(encoder, method):
    za = product()
    names, datas = presel_list()
    methods = [za.preselect(method, za.guess_type_from_name(nm), len(d)) for nm, d in zip(names, datas)]
    assert all(a != b for a, b in zip(methods, methods[1:])) and len(set(methods)) >= (5 if method == 35 else 4), methods
    want, entries, res = check_equal(encoder, method, names, datas, a_arc=7)
    assert [int(r) for r in res["zip_type"]] == [e["zip_type"] for e in entries]
    assert {12, 14, 8} <= {e["zip_type"] for e in entries} if method == 35 else {14, 8} <= {e["zip_type"] for e in entries}
    marks = dict(encoder.last_timing())
    assert "zip:k_zw_place (hold)" in marks, "a group with several methods keeps its streams in the holding buffer"


@pytest.mark.parametrize("method", (10, 14, 17, 0, 35))
def test_passwords(encoder, plains, method):
    """Fixed encryption headers: the bytes of the reference; zipfile and extract_device read every entry back; the random entry is stored AND encrypted
    from its own bytes with the arena unchanged (CallEx.run).  (batch_mib = 1: test_passwords_over_several_groups.)"""
    za = product()
    if method == 35:
        names, datas = presel_list()
        names, datas = names + ["rnd.bin"], datas + [plains[-2]]
    else:
        names, datas = names_for(plains), plains
    hd = headers_for(len(datas))
    want, entries, res = check_equal(encoder, method, names, datas, a_arc=9, password=PW, headers=hd, key=("pw", method))
    k = names.index("rnd.bin") if method == 35 else len(datas) - 2
    assert int(res["zip_type"][k]) == 0 and int(res["csize"][k]) == 4096 + 12
    off = int(res["offset"][k]) + 30 + len(names[k].encode()) + 12
    assert want[off:off + 4096] != datas[k]
    assert all(e["flag"] & 1 for e in entries) and [int(r) for r in res["csize"]] == [e["csize"] for e in entries]
    methods = [za.preselect(method, za.guess_type_from_name(nm), len(d)) for nm, d in zip(names, datas)]
    zipfile_reads_back(want, names, datas, methods, pwd=PW.encode("latin-1"), least=len(datas) - 2)
    import torch
    info = za.ZipInfo.load_device(torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).cuda())
    got = za.UnZip(encoder, bzip2=True, lzma=True).extract_device(info, password=PW)
    assert [bytes(got[nm].cpu().numpy()) for nm in names] == datas


def plan_groups(encoder, tab, methods, limit):
    """The groups zada_zip_device_ex makes of the table, from the plan's own zw_groups_ex (tests/zip/libzip_plan_ex_host.so): (g1, kind) pairs."""
    import os
    from _common import ROOT
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "zip", "libzip_plan_ex_host.so"))
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.zpx_groups.argtypes = [vp, i32, vp, vp, u64, u64, u64, vp, i32]
    encoder.lib.zada_lzma_lit_table_bytes.restype = u64
    m = np.array(methods, np.int32)
    lit = np.array([encoder.lib.zada_lzma_lit_table_bytes(int(x)) for x in methods], np.uint64)
    g = np.zeros((len(tab) + 1, 2), np.int32)
    k = L.zpx_groups(tab.ctypes.data, len(tab), m.ctypes.data, lit.ctypes.data, limit, 256 << 20, 12288 << 20, g.ctypes.data, len(tab) + 1)
    return [(int(a), int(b)) for a, b in g[:k]]


@pytest.mark.parametrize("method", (35, 10, 14, 17))
def test_passwords_over_several_groups(encoder, method):
    """batch_mib = 1 on a list whose slots take 1.5 MiB: two batch groups in one call -- asserted from the plan's own groups --, for Preselection_2 both
    with several methods, so the second one uses the holding buffer again and indexes its verdicts and keys from g0 > 0.  The bytes of the reference."""
    za = product()
    names, datas = presel_list()
    names, datas = ["r%d/%s" % (r, nm) for r in range(4) for nm in names], [d[r:] for r in range(4) for d in datas]
    methods = [za.preselect(method, za.guess_type_from_name(nm), len(d)) for nm, d in zip(names, datas)]
    hd = headers_for(len(datas), seed=60)
    want, entries = host_archive(encoder, method, names, datas, password=PW, headers=hd)
    c = CallEx(encoder, names, datas, a_arc=2)
    groups = plan_groups(encoder, c.tab, methods, 1 << 20)
    assert groups == [(32, 0), (48, 0)], groups
    if method == 35:
        assert len(set(methods[:32])) > 3 and len(set(methods[32:])) > 3
    assert plan_groups(encoder, c.tab, methods, 512 << 20) == [(48, 0)]
    try:
        encoder.set_knob("batch_mib", 1)
        rc, alen, res, buf, said = c.run(method, len(want), password=PW, headers=hd)
        assert rc == 0 and alen == len(want) and buf.tobytes() == want, said
        same_results(res, entries, datas)
        marks = dict(encoder.last_timing())
        assert "zip:k_zc_place" in marks and ("zip:k_zw_place (hold)" in marks) == (method == 35) and (method not in (17, 35) or "lzma:end" in marks)
    finally:
        encoder.set_knob("batch_mib", 512)
    rc, alen, res, buf, said = c.run(method, len(want), password=PW, headers=hd)      # ... and as one group
    assert rc == 0 and buf.tobytes() == want, said


def test_large_entries_placed_alone(encoder):
    """An entry of ZW_ENTRY_MAX + 1 bytes for Deflate_1 and one of 1 MiB (above the one-block limit) for BZip2_3, each among small neighbours, with a
    password: written to their place behind the encryption header and encoded there."""
    t = text()
    small = [t[3000 * k:3000 * k + 5000] for k in range(4)]
    for method, big in ((8, (t * 8)[:MIB4 + 1]), (14, (t * 2)[:1 << 20])):
        datas = small[:2] + [big] + small[2:]
        names = names_for(datas)
        hd = headers_for(len(datas), seed=40)
        want, entries, res = check_equal(encoder, method, names, datas, a_arc=5, password=PW, headers=hd, too_small=False)
        assert int(res["zip_type"][2]) == (8 if method == 8 else 12)
        check_equal(encoder, method, names, datas, a_arc=6, too_small=False)
        with zipfile.ZipFile(io.BytesIO(want)) as z:
            assert z.read(names[2], pwd=PW.encode("latin-1")) == big


def test_refusals(encoder, plains):
    """Refused by name; a password without random11; every per-entry refusal of the old call with its index; nothing is written; count = 0."""
    names = names_for(plains)
    c = CallEx(encoder, names, plains)
    cap = c.bound()

    def untouched(buf):
        return bool((buf == GUARD).all())

    for method, nm in ((1, "Shrink_1"), (2, "Reduce_1"), (5, "Reduce_4"), (99, "unknown"), (-1, "unknown")):
        rc, _, _, buf, said = c.run(method, cap)
        assert rc == E_INVALID and "method %d (%s) is not one it takes" % (method, nm) in said and untouched(buf), said
    pw = ctypes.create_string_buffer(b"secret", 6)
    rc, _, _, buf, said = c.run(10, cap, crypt=(ctypes.addressof(pw), 6, 0))
    assert rc == E_INVALID and "random11" in said and untouched(buf)
    h = ctypes.create_string_buffer(bytes(11 * len(plains)), 11 * len(plains))
    rc, _, _, buf, said = c.run(10, cap, crypt=(0, 6, ctypes.addressof(h)))
    assert rc == E_INVALID and untouched(buf), said
    for k, (field, value, rcw, why) in enumerate((("d_data", 0, E_INVALID, "null d_data with n > 0"), ("name_len", 65536, E_INVALID, "a name longer than 65 535 bytes"),
                                                  ("n", 1 << 40, E_TOO_LARGE, "an entry of 1 TiB or more"))):
        for method in (14, 17, 35):
            tab = c.tab.copy()
            tab[3 + k][field] = value
            rc, _, _, buf, said = c.run(method, cap, tab=tab)
            assert rc == rcw and "entry %d: %s" % (3 + k, why) in said and untouched(buf), said
    # with a password, an entry whose compressed size with the 12 header bytes has no place in its local header (nothing is read: the checks come first)
    tab = c.tab.copy()
    tab[6]["d_data"], tab[6]["n"] = 1 << 20, 0xFFFFFFFF - 5
    rc, _, _, buf, said = c.run(14, cap, tab=tab, password=PW, headers=headers_for(len(tab)))
    assert rc == E_INVALID and "entry 6: an encrypted entry of 4 GiB - 11 .. 4 GiB - 1 bytes" in said and untouched(buf), said
    # an input that overlaps the archive buffer: the buffer of the next run lies where this one's did only by chance, so point an entry into it afterwards
    import torch
    t_arc = torch.full((cap + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    tab = c.tab.copy()
    tab[5]["d_data"] = t_arc.data_ptr() + 64 + 10
    res = np.zeros(len(tab), dtype=product().Encoder.zip_dtypes()[1])
    alen = ctypes.c_uint64(0)
    rc = encoder.lib.zada_zip_device_ex(encoder.ctx, 14, len(tab), tab.ctypes.data, t_arc.data_ptr() + 64, cap, 0, None, ctypes.byref(alen), res.ctypes.data)
    assert rc == E_INVALID and "entry 5: its input overlaps the archive buffer" in encoder.lib.zada_last_error(encoder.ctx).decode()
    assert bool((t_arc == 0xA5).all())
    # count = 0: the 22-byte end record
    e = CallEx(encoder, [], [])
    for method, kw in ((35, {}), (14, dict(password=PW, headers=[]))):
        rc, alen, _, buf, said = e.run(method, 22, **kw)
        assert rc == 0 and alen == 22 and buf.tobytes() == host_archive(encoder, method, [], [])[0], said
    rc, _, _, _, said = e.run(35, 21)
    assert rc == E_INVALID and "archive buffer too small" in said


def test_write_device_ex_round_trip(encoder):
    import torch
    za = product()
    names, datas = presel_list()
    names = ["sub\\" + nm for nm in names]
    tensors = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() if d else torch.empty(0, dtype=torch.uint8) for d in datas]
    hd = headers_for(len(datas), seed=70)
    for pw in (None, PW):
        for kw in (dict(), dict(file_time=0x5A215A21, unicode_name=False)):
            ref = za.ZipCreate(encoder, za.Method.Preselection_2, _offset_bias=77)
            ref.add_streams(names, datas, password=pw, _headers=hd if pw else None, **kw)
            want = ref.finish()
            zc = za.ZipCreate(encoder, za.Method.Preselection_2, _offset_bias=77)
            arc = zc.write_device_ex(names, tensors, password=pw, _headers=hd if pw else None, **kw)
            assert bytes(arc.cpu().numpy()) == want and zc.entries == ref.entries
            with pytest.raises(ValueError):
                zc.write_device_ex(names, tensors)
    for pw in (None, PW):
        zc = za.ZipCreate(encoder, za.Method.Preselection_2)
        arc = zc.write_device_ex(names, tensors, password=pw)                       # (headers from os.urandom)
        info = za.ZipInfo.load_device(arc)
        got = za.UnZip(encoder, bzip2=True, lzma=True).extract_device(info, password=pw)
        assert [bytes(got[nm.replace("\\", "/")].cpu().numpy()) for nm in names] == datas
        methods = [za.preselect(za.Method.Preselection_2, za.guess_type_from_name(nm), len(d)) for nm, d in zip(names, datas)]
        zipfile_reads_back(bytes(arc.cpu().numpy()), names, datas, methods, pwd=pw.encode("latin-1") if pw else None, least=len(datas) - 2)
    with pytest.raises(za.ZadaError):
        za.ZipCreate(encoder, za.Method.Preselection_2).write_device_ex(["x"], [torch.zeros(4, dtype=torch.uint8)])
    with pytest.raises(za.ZadaError):
        za.ZipCreate(encoder, 1).write_device_ex(names, tensors)


def test_order_independence(encoder, plains):
    """A zada_zip_device_ex call (Preselection_2, with a password) between two equal batch calls of every compressor on one context leaves their
    results equal; so does the old zada_zip_device around it."""
    za = product()
    names, datas = presel_list()
    hd = headers_for(len(datas), seed=90)
    small = [d for d in plains if len(d) <= 70000]
    c = CallEx(encoder, names, datas)
    cap = c.bound(0, True)
    old = CallEx(encoder, names_for(small), small)

    def ex():
        rc, alen, res, buf, said = c.run(35, cap, password=PW, headers=hd)
        assert rc == 0, said
        return buf[:alen].tobytes()

    def old_call():
        rc, alen, res, buf, said = old.run(10, old.bound(), old=True)
        assert rc == 0, said
        return buf[:alen].tobytes()

    first = ex()
    for call in (lambda: encoder.bzip2_batch(small, 14), lambda: encoder.lzma_batch(small, 17), lambda: encoder.lzma_batch(small[:8], 18),
                 lambda: encoder.deflate_batch(small, 10), old_call):
        before = call()
        assert ex() == first
        assert call() == before
    assert first == host_archive(encoder, 35, names, datas, password=PW, headers=hd)[0]
