"""ReZip on the device (include/zada.h "an archive in device memory recompressed into device memory").  The reference is never the code under test:
per entry and approach the size and the stream come from ZipCreate (enc, method).add_streams on host bytes (pinned to the oracle elsewhere), the
choice from the approach loop restated from the Ada text and the archive bytes from the header model, both in tests/_rezip.py."""
import ctypes
import io
import zipfile
import zlib

import numpy as np
import pytest

import _rezip
from _common import product
from _devbuf import GUARD, guard_damage
from _zipdev import text, zipfile_reads_back

pytestmark = pytest.mark.gpu
E_INVALID, E_TOO_LARGE, E_DATA = -1, -4, -7
G = 64
COMMENT = b"the source's comment"
SRC_METHODS = (0, 8, 14, 18)                             # Store, Deflate_1, BZip2_3, LZMA_3: the source's entries take turns, but for these:
SRC_FIXED = {"m\\back.txt": 8, "dir/b.ads": 8, "w.html": 8, "z.bin": 0, "lz.bin": 18, "dir/": 0}


def source_list():
    """About a dozen entries cut from the text, names not in order, one with a backslash, an empty one, 4 KiB of random bytes (a Store fallback under
    every method), 30 000 zero bytes (Deflate_3's turn to win), 100 000 bytes (above BZip2_1's one block) and a directory entry."""
    t = text()
    rnd = np.random.default_rng(3).integers(0, 256, 4096, dtype=np.uint8).tobytes()
    cut = lambda k, n: t[7000 * k:7000 * k + n]
    return [("zeta.txt", cut(0, 20000)), ("dir/", b""), ("alpha.c", cut(1, 3000)), ("m\\back.txt", cut(2, 300)), ("empty", b""), ("random.bin", rnd),
            ("big.dat", t[300000:400000]), ("dir/b.ads", cut(3, 9000)), ("Alpha.txt", cut(4, 17)), ("one", b"x"), ("pic.pgm", cut(5, 12000)),
            ("lz.bin", cut(8, 5000) * 4), ("w.html", cut(7, 33000)), ("z.bin", bytes(30000))]


_cache = {}


def host_streams(enc, method, datas):
    """[(zip type, stream)] of ZipCreate (enc, method).add_streams on host bytes; kept per (method, data)"""
    za = product()
    todo = [d for d in dict.fromkeys(datas) if (method, d) not in _cache]
    if todo:
        zc = za.ZipCreate(enc, method)
        zc.add_streams(["e%d" % k for k in range(len(todo))], todo)
        arc = zc.finish()
        for d, e in zip(todo, za.ZipInfo.load(arc).entries):
            _cache[(method, d)] = (e.method, arc[e.data_offset:e.data_offset + e.csize])
    return [_cache[(method, d)] for d in datas]


def source_archive(enc):
    """The source, written on the host entry by entry with the methods of SRC_METHODS in turn (lz.bin, four copies of 5 000 bytes: LZMA_3, which nothing beats there), flag
    bit 1 set in the LZMA entries' headers and bit 3 in one local header, and a comment."""
    if "src" in _cache:
        return _cache["src"]
    za = product()
    src = source_list()
    zc = za.ZipCreate(enc, 0)
    for k, (nm, d) in enumerate(src):
        m = SRC_FIXED.get(nm, SRC_METHODS[k % 4])
        zt, stream = host_streams(enc, m, [d])[0] if m else (0, d)
        zc.add_compressed(nm, stream, zlib.crc32(d), len(d), zt)
    arc = bytearray(zc.finish().replace(b"m/back.txt", b"m\\back.txt"))      # (add_compressed turns the backslash into a slash: put it back)
    e = za.ZipInfo.load(bytes(arc))["alpha.c"]
    arc[e.header_offset + 6] |= 8                              # flag bit 3 in one local header (the sizes are in the directory)
    arc[-2:] = len(COMMENT).to_bytes(2, "little")
    arc += COMMENT
    _cache["src"] = bytes(arc)
    return _cache["src"]


def model(enc, arc, approaches=0x0FE7, formats=0x1F, base=0, comment=COMMENT, lower=False, touch=None):
    """What zada_rezip_device must write for the source `arc`: -> (archive bytes, results [(approach, zip type, csize, offset)], sizes matrix, names)"""
    za = product()
    info = za.ZipInfo.load(arc)
    order = za.zip_load_order(info)
    consider = _rezip.consider_a_priori(approaches, formats)
    rows, results, sizes = [], [], []
    by_method = {}
    kept = [(key, e) for key, e in order if key and key[-1:] not in (b"/", b"\\")]
    plain = dict((nm.replace("\\", "/").encode(), d) for nm, d in source_list())
    for key, e in kept:
        d = plain[key]
        for a in range(1, 12):
            if consider[a]:
                m = _rezip.METHOD[a] if _rezip.METHOD[a] < 34 else za.preselect(_rezip.METHOD[a], za.guess_type_from_name(key.decode("latin-1")), len(d))
                by_method.setdefault(m, []).append((key, a))
    got = {}
    for m, users in sorted(by_method.items()):
        keys = list(dict.fromkeys(k for k, _ in users))
        for k, r in zip(keys, host_streams(enc, m, [plain[k] for k in keys])):
            got[(k, m)] = r
    for key, e in order:
        if not key or key[-1:] in (b"/", b"\\"):
            results.append(None)
            sizes.append([_rezip.NOT_TRIED] * 12)
            continue
        d = plain[key]
        size, stream = [None] * 12, [None] * 12
        size[0], stream[0] = e.csize, (e.method, arc[e.data_offset:e.data_offset + e.csize], e.method == 14 and bool(e.local_flags & 2))
        for a in range(1, 12):
            if consider[a]:
                m = _rezip.METHOD[a] if _rezip.METHOD[a] < 34 else za.preselect(_rezip.METHOD[a], za.guess_type_from_name(key.decode("latin-1")), len(d))
                zt, s = got[(key, m)]
                size[a], stream[a] = len(s), (zt, s, zt == 14)
        choice = _rezip.try_all_approaches(consider, [x if x is not None else 0 for x in size], bool((formats >> _rezip.FORMAT_BIT[e.method]) & 1))
        zt, s, eos = stream[choice]
        name = key.decode("latin-1").lower().encode("latin-1") if lower else key
        rows.append(dict(name=name, version=e.local_version, flags=e.local_flags, time=e.local_time if touch is None else touch, crc=e.crc, usize=e.usize,
                         csize=len(s), zip_type=zt, eos=eos, payload=s))
        results.append((choice, zt, len(s)))
        sizes.append([_rezip.NOT_TRIED if x is None else x for x in size])
    body, tail, offs, total = _rezip.rezip_archive(rows, base, comment)
    it = iter(offs)
    results = [None if r is None else r + (next(it),) for r in results]
    return body + tail, results, sizes, [key for key, _ in order]


class Call:
    """One zada_rezip_device call: the source at offset 3 modulo 16 of its tensor, the output at G + a_out of a tensor of GUARD; run () asserts that no
    guard byte and no byte of the source changed."""

    def __init__(self, enc, arc, a_out=0, lower=False, touch=None):
        import torch
        za = product()
        self.enc, self.arc = enc, arc
        self.h_src = np.full(3 + len(arc), GUARD, dtype=np.uint8)
        self.h_src[3:] = np.frombuffer(arc, dtype=np.uint8)
        self.t_src = torch.from_numpy(self.h_src).cuda()
        order = za.zip_load_order(za.ZipInfo.load(arc))
        self.names = [(k.decode("latin-1").lower().encode("latin-1") if lower else k) for k, _ in order]
        self.blob = np.frombuffer(b"".join(self.names) + b"\0", dtype=np.uint8)
        self.tab = np.zeros(len(order), dtype=za.Encoder.rezip_dtypes()[0])
        at = 0
        for k, (key, e) in enumerate(order):
            self.tab[k] = (e.data_offset, e.csize, e.usize, e.crc, e.local_time if touch is None else touch, e.method, e.local_flags, e.local_version, 0,
                           len(self.names[k]), 0, self.blob.ctypes.data + at)
            at += len(self.names[k])
        self.a_out = G + a_out

    def run(self, cap, approaches=0x0FE7, formats=0x1F, base=0, comment=COMMENT, tab=None, out_ptr=None):
        import torch
        za = product()
        tab = self.tab if tab is None else tab
        t_out = torch.full((self.a_out + cap + G,), GUARD, dtype=torch.uint8, device="cuda")
        res = np.zeros(len(tab), dtype=za.Encoder.rezip_dtypes()[1])
        sizes = np.zeros((len(tab), 12), dtype=np.uint64)
        alen = ctypes.c_uint64(0)
        keep = ctypes.create_string_buffer(comment, max(len(comment), 1))
        torch.cuda.synchronize()
        rc = self.enc.lib.zada_rezip_device(self.enc.ctx, self.t_src.data_ptr() + 3, len(self.arc), len(tab), tab.ctypes.data, approaches, formats,
                                            t_out.data_ptr() + self.a_out if out_ptr is None else out_ptr, cap, base, ctypes.addressof(keep) if comment else None,
                                            len(comment), ctypes.byref(alen), res.ctypes.data, sizes.ctypes.data)
        said = self.enc.lib.zada_last_error(self.enc.ctx).decode()
        torch.cuda.synchronize()
        host = t_out.cpu().numpy()
        bad = guard_damage(host, self.a_out, cap)
        assert not bad, "bytes outside the archive buffer were written: %r" % bad[:8]
        assert np.array_equal(self.t_src.cpu().numpy(), self.h_src), "the source was written"
        return rc, alen.value, res, sizes, host[self.a_out:self.a_out + cap].tobytes(), said


def check(enc, arc, a_out=0, too_small=False, **kw):
    want, results, sizes, _ = model(enc, arc, **kw)
    c = Call(enc, arc, a_out, lower=kw.get("lower", False), touch=kw.get("touch"))
    kw = {k: v for k, v in kw.items() if k not in ("lower", "touch")}
    assert enc.rezip_bound(c.tab, len(kw.get("comment", COMMENT))) >= len(want)
    if too_small:
        rc, _, _, _, _, said = c.run(len(want) - 1, **kw)
        assert rc == E_INVALID and "archive buffer too small" in said, (rc, said)
    rc, alen, res, sz, buf, said = c.run(len(want), **kw)
    assert rc == 0, said
    assert alen == len(want)
    assert buf == want, "first difference at byte %d of %d" % (next(i for i, (x, y) in enumerate(zip(buf, want)) if x != y), len(want))
    for k, r in enumerate(results):
        if r is None:
            assert int(res["flags"][k]) & 1
        else:
            assert (int(res["approach"][k]), int(res["zip_type"][k]), int(res["csize"][k]), int(res["offset"][k])) == r, k
    assert [[int(x) for x in row] for row in sz] == sizes
    return want, results, sizes


@pytest.mark.parametrize("a_out", (0, 1, 15))
def test_equality(encoder, a_out):
    """Archive bytes, results and the sizes matrix equal the model, cap = archive_len exactly, cap - 1 refused, guards and source untouched.  A
    condition on the list: the winners comprise original and at least three other approaches and a Store fallback (the tie of the entry that is LZMA_3
    already: test_format_sets_and_masks)."""
    arc = source_archive(encoder)
    want, results, sizes = check(encoder, arc, a_out, too_small=a_out == 0)
    wins = {r[0] for r in results if r}
    assert 0 in wins and len(wins - {0}) >= 3, wins
    names = product().zip_load_order(product().ZipInfo.load(arc))
    rnd = [k for k, (key, _) in enumerate(names) if key == b"random.bin"][0]
    assert sizes[rnd][5] == sizes[rnd][7] == sizes[rnd][10] == 4096 and results[rnd][1] == 0, "no Store fallback"
    lz = [k for k, (key, _) in enumerate(names) if key == b"lz.bin"][0]
    assert sizes[lz][10] == sizes[lz][0], "the LZMA_3 approach does not reproduce the source's LZMA_3 stream"
    # a tie goes to the earlier approach under the default mask too: on the empty entry and on the entry of one byte every approach falls back to
    # Store at the source's own size, and the winner is original
    for nm in (b"empty", b"one"):
        k = [i for i, (key, _) in enumerate(names) if key == nm][0]
        assert results[k][0] == 0 and len({x for x in sizes[k] if x != _rezip.NOT_TRIED}) == 1, (nm, results[k], sizes[k])
    assert zipfile.ZipFile(io.BytesIO(want)).comment == COMMENT


def test_format_sets_and_masks(encoder):
    arc = source_archive(encoder)
    _, results, sizes = check(encoder, arc, formats=_rezip.DEFLATE_OR_STORE)
    assert all(r is None or r[1] in (0, 8) for r in results) and all(row[1] == row[2] == _rezip.NOT_TRIED for row in sizes)
    assert any(r and sizes[k][r[0]] > sizes[k][0] for k, r in enumerate(results)), "no original was forced out at a larger size"
    _, results, _ = check(encoder, arc, formats=_rezip.FAST_DECOMPRESSION)
    assert all(r is None or r[1] != 12 for r in results)
    check(encoder, arc, approaches=(1 << 0) | (1 << 5))
    # the entry that is LZMA_3 already stays original against lzma_3: a tie goes to the earlier approach.  (Under the default mask LZMA_2 is 14 bytes
    # shorter than LZMA_3 on this entry -- 2 468 against 2 482 --, so the tie is shown under the mask of the two.)
    _, results, sizes = check(encoder, arc, approaches=(1 << 0) | (1 << 10))
    lz = [k for k, (key, _) in enumerate(product().zip_load_order(product().ZipInfo.load(arc))) if key == b"lz.bin"][0]
    assert results[lz][0] == 0 and sizes[lz][10] == sizes[lz][0]
    _, results, _ = check(encoder, arc, approaches=1, comment=b"", lower=True, touch=0x5A21_8C40, base=1000)
    assert all(r is None or r[0] == 0 for r in results)
    c = Call(encoder, arc)
    for bit, name in ((3, "Shrink_1"), (4, "Reduce_4")):
        rc, _, _, _, _, said = c.run(1 << 20, approaches=0x0FE7 | (1 << bit))
        assert rc == E_INVALID and name in said


def test_groups(encoder):
    """batch_mib = 1: the same bytes from several groups; last_timing shows the extraction, the encoders and the placement."""
    arc = source_archive(encoder)
    encoder.set_knob("batch_mib", 1)
    try:
        check(encoder, arc, approaches=(1 << 0) | (1 << 5) | (1 << 7) | (1 << 11))
        marks = [nm for nm, _ in encoder.last_timing()]
    finally:
        encoder.set_knob("batch_mib", 512)
    assert "rezip:k_zw_place" in marks and "zip:k_zw_pack" in marks and any(nm.startswith("unzip:") for nm in marks), marks


def test_read_back_and_compare(encoder):
    """ZipInfo.load_device + extract_device return every input; zipfile reads what it can; CompZip.compare_device of the source against the
    rezipped archive reports the directory entry as missing and nothing else."""
    import torch
    za = product()
    arc = source_archive(encoder)
    t = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).cuda()
    out, rep = za.ReZip(encoder).rezip_device(za.ZipInfo.load_device(t), report=True)
    want, results, sizes, _ = model(encoder, arc)
    assert out.cpu().numpy().tobytes() == want
    plain = dict((nm.replace("\\", "/"), d) for nm, d in source_list() if not nm.endswith("/"))
    back = za.UnZip(encoder, bzip2=True, lzma=True).extract_device(za.ZipInfo.load_device(out))
    assert {nm: v.cpu().numpy().tobytes() for nm, v in back.items()} == plain
    info = za.ZipInfo.load(want)
    zipfile_reads_back(want, [e.name for e in info.entries], [plain[e.name] for e in info.entries], [19 if e.method == 14 else 0 for e in info.entries], least=3)
    r = za.CompZip(encoder).compare_device(za.ZipInfo.load_device(t), za.ZipInfo.load_device(out))
    assert (r.size_failures, r.compare_failures, r.damaged, r.missing_1_in_2, r.just_a_directory, r.missing_2_in_1) == (0, 0, 0, 1, 1, 0)
    assert r.total_bytes == sum(len(d) for d in plain.values())
    assert sum(v["count"] for v in rep["totals"].values()) == len(plain) and rep["totals"]["original"]["saved"] == 0
    assert sum(v["saved"] for v in rep["totals"].values()) == sum(e.csize for e in za.ZipInfo.load(arc).entries) - sum(e.csize for e in info.entries)
    assert za.ReZip(encoder).rezip(arc) == want


def test_a_large_entry(encoder):
    """One stored entry of 4 MiB + 1 with {original, deflate_3, bzip2_3}: it runs alone through the single-stream paths.  The other approaches are
    left out: a single LZMA_3 stream of this size runs at a quarter of a megabyte per second."""
    za = product()
    d = (text() * 8)[:(4 << 20) + 1]
    zc = za.ZipCreate(encoder, 0)
    zc.add_compressed("large.bin", d, zlib.crc32(d), len(d), 0)
    arc = zc.finish()
    mask = (1 << 0) | (1 << 5) | (1 << 7)
    c = Call(encoder, arc)
    rc, alen, res, sizes, buf, said = c.run(encoder.rezip_bound(c.tab, 0), approaches=mask, comment=b"")
    assert rc == 0, said
    want = {5: host_streams(encoder, 10, [d])[0], 7: host_streams(encoder, 14, [d])[0]}
    assert [int(x) for x in sizes[0]][5] == len(want[5][1]) and int(sizes[0][7]) == len(want[7][1]) and int(sizes[0][0]) == len(d)
    a = int(res["approach"][0])
    assert a == min((5, 7), key=lambda x: (len(want[x][1]), x)) and int(res["csize"][0]) == len(want[a][1])
    info = za.ZipInfo.load(buf[:alen])
    e = info.entries[0]
    assert buf[e.data_offset:e.data_offset + e.csize] == want[a][1] and e.crc == zlib.crc32(d)


def test_refusals_and_failures(encoder):
    """Each with its index in the text, and the guards intact (Call.run)."""
    za = product()
    arc = source_archive(encoder)
    c = Call(encoder, arc)
    cap = encoder.rezip_bound(c.tab, len(COMMENT))

    def refused(rc_want, text_want, **change):
        tab = c.tab.copy()
        at = change.pop("at", 2)
        for f, v in change.items():
            tab[f][at] = v
        rc, _, _, _, _, said = c.run(cap, tab=tab)
        assert rc == rc_want and text_want in said, (rc, said)
    refused(E_INVALID, "entry 2: encrypted", flags=1)
    refused(E_INVALID, "entry 2: unknown source method", method=1)
    refused(E_INVALID, "entry 3: the same name as an earlier entry", at=3, name=int(c.tab["name"][2]), name_len=int(c.tab["name_len"][2]))
    refused(E_INVALID, "entry 2: its data lie beyond the source archive", in_off=len(arc))
    refused(E_DATA, "CRC-32", crc=int(c.tab["crc"][2]) ^ 1)
    rc, _, _, _, _, said = c.run(cap, out_ptr=c.t_src.data_ptr() + 100)
    assert rc == E_INVALID and "overlaps the source" in said
    info = za.ZipInfo.load(arc)
    e = next(x for x in info.entries if x.method == 8 and x.csize > 100)
    bad = bytearray(arc)
    bad[e.data_offset + e.csize // 2] ^= 0x10
    c2 = Call(encoder, bytes(bad))
    rc, _, _, _, _, said = c2.run(cap)
    k = [i for i, (key, x) in enumerate(za.zip_load_order(info)) if x is e][0]
    assert rc == E_DATA and ("entry %d:" % k) in said, (rc, said)


def test_a_refused_lzma_3_entry_loses_that_approach(encoder):
    """With the reference's dictionary_size of 5 000 (knob "lzma_dict") the coder refuses the committed defect input (ZADA_E_REFERENCE,
    test_gpu_lzma.py::test_reference_defect_is_refused_not_written): the method's call is repeated entry by entry, the refused entry's lzma_3 is
    marked not tried and flagged, its neighbour keeps its LZMA_3 stream, and the archive is the model's for these sizes."""
    from _lzmah import lz_inputs
    za = product()
    x, y = bytes(lz_inputs()["mix_256k"][:12000]), text()[91000:94000]
    zc = za.ZipCreate(encoder, 0)
    for nm, d in (("x.bin", x), ("y.bin", y)):
        zc.add_compressed(nm, d, zlib.crc32(d), len(d), 0)
    arc = zc.finish()
    mask = (1 << 0) | (1 << 5) | (1 << 10)
    c = Call(encoder, arc)
    encoder.set_knob("lzma_dict", 5000)
    try:
        (rx, px, _), (ry, py, _) = encoder.lzma_batch([x, y], 18)          # the host path's batch: x refused, y coded
        assert rx == -6 and px is None and ry == 0
        y_lzma = (14, py)
        rc, alen, res, sizes, buf, said = c.run(encoder.rezip_bound(c.tab, 0), approaches=mask, comment=b"")
    finally:
        encoder.set_knob("lzma_dict", 0)
    assert rc == 0, said
    dx, dy = host_streams(encoder, 10, [x, y])
    NT = _rezip.NOT_TRIED
    assert [int(v) for v in sizes[0]] == [12000, NT, NT, NT, NT, len(dx[1]), NT, NT, NT, NT, NT, NT] and int(res["flags"][0]) & 2
    assert [int(v) for v in sizes[1]] == [3000, NT, NT, NT, NT, len(dy[1]), NT, NT, NT, NT, len(y_lzma[1]), NT] and not int(res["flags"][1]) & 2
    info = za.ZipInfo.load(arc)
    rows = []
    for ent, cands in ((info["x.bin"], [(0, 0, x), (5,) + dx]), (info["y.bin"], [(0, 0, y), (5,) + dy, (10,) + y_lzma])):
        consider = [a in [cd[0] for cd in cands] for a in range(12)]
        size = [0] * 12
        for a, zt, st in cands:
            size[a] = len(st)
        a, zt, st = next(cd for cd in cands if cd[0] == _rezip.try_all_approaches(consider, size, True))
        rows.append(dict(name=ent.raw_name, version=ent.local_version, flags=ent.local_flags, time=ent.local_time, crc=ent.crc, usize=ent.usize, csize=len(st), zip_type=zt,
                         eos=zt == 14, payload=st))
    body, tail, _, total = _rezip.rezip_archive(rows, 0, b"")
    assert alen == total and buf[:alen] == body + tail


def test_a_fresh_context(encoder):
    """The first call on a new Encoder is rezip_device, then compare_device."""
    import torch
    za = product()
    arc = source_archive(encoder)
    want, _, _, _ = model(encoder, arc, approaches=0x21)
    enc = za.Encoder(0)
    try:
        t = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).cuda()
        out = za.ReZip(enc).rezip_device(za.ZipInfo.load_device(t), approaches=("original", "deflate_3"))
        assert out.cpu().numpy().tobytes() == want
        assert za.CompZip(enc).compare_device(za.ZipInfo.load_device(t), za.ZipInfo.load_device(out)).total_differences == 1
    finally:
        enc.close()
