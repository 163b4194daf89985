"""Comp_Zip on the device (include/zada.h "two archives that lie in device memory, compared entry by entry"): zada_compare_device at every
alignment and around every piece boundary, against numpy; CompZip.compare_device and zada_compzip_device against the literal restatement of
tools/comp_zip_prc.adb in tests/_rezip.py, on archives written on the host by zipfile (all four of its methods, which the reader decodes) and by
ZipCreate.write_device_ex with a password.  The reference is never the code under test."""
import io
import zipfile

import numpy as np
import pytest

import _rezip
from _common import product
from _devbuf import GUARD
from _zipdev import headers_for, text

pytestmark = pytest.mark.gpu
PIECE = 16384
PW = "p\xe4ssword"


# ---- zada_compare_device ----
_rng = np.random.default_rng(11)
_base = _rng.integers(0, 256, 2 * PIECE + 64, dtype=np.uint8)


def compare(enc, n, al_a, al_b, flips=(), outside=False):
    """The first n bytes of the shared random text at offsets 16 + al_a and 16 + al_b of two tensors with 32 bytes and more around them; side b's bytes at
    `flips` are changed; outside: the bytes directly in front of both buffers and at their ends differ too.  -> first_diff"""
    import torch
    a = np.full(16 + al_a + n + 32, GUARD, dtype=np.uint8)
    b = np.full(16 + al_b + n + 32, GUARD, dtype=np.uint8)
    a[16 + al_a:16 + al_a + n] = _base[:n]
    b[16 + al_b:16 + al_b + n] = _base[:n]
    for f in flips:
        b[16 + al_b + f] ^= 0x40
    if outside:                                                # the 16 bytes in front of each buffer and the 16 bytes behind it
        for buf, al, v in ((a, al_a, 0x22), (b, al_b, 0x11)):
            buf[al:16 + al] = v
            buf[16 + al + n:32 + al + n] = v
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    got = enc.compare_device(ta.data_ptr() + 16 + al_a, tb.data_ptr() + 16 + al_b, n)
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b), "a buffer was written"
    return got


LENGTHS = (0, 1, 15, 16, 17, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 3)
ALIGNS = [(x, y) for x in (0, 1, 15) for y in (0, 1, 15)]


@pytest.mark.parametrize("al", ALIGNS, ids=lambda al: "a%d_b%d" % al)
def test_compare_device(encoder, al):
    """Every length of the list at this pair of alignments: equal buffers give n, with differing bytes directly in front of both buffers and behind
    them; a difference at byte 0, at the last byte, at the last byte of a piece and at the first byte of the next one is found where it is; of two
    differences in different pieces -- and of two in one 16-byte word -- the earlier one is reported."""
    for n in LENGTHS:
        assert compare(encoder, n, *al, outside=True) == n, n
        spots = {0, n - 1, n // 2, PIECE - 1, PIECE, 2 * PIECE - 1, 2 * PIECE, 17, 1023, 1024}
        for f in sorted(s for s in spots if 0 <= s < n):
            assert compare(encoder, n, *al, flips=(f,), outside=True) == f, (n, f)
    n = 2 * PIECE + 3
    assert compare(encoder, n, *al, flips=(PIECE - 1, PIECE)) == PIECE - 1
    assert compare(encoder, n, *al, flips=(5000, 2 * PIECE + 2)) == 5000
    assert compare(encoder, n, *al, flips=(2 * PIECE + 1, 100, PIECE + 7)) == 100
    assert compare(encoder, n, *al, flips=(4001, 4003)) == 4001
    assert compare(encoder, 40, *al, flips=(39, 3)) == 3


def test_compare_device_beyond_4_gib(encoder):
    """Offsets that need more than 32 bits: 4 GiB + two pieces + 5 bytes at alignments 1 and 2 (uninitialised memory, copied, so equal): n; then a
    difference in the last byte, and one three bytes behind 4 GiB in front of it, each found where it is."""
    import torch
    n = (1 << 32) + 2 * PIECE + 5
    a = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    b = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    b[2:2 + n].copy_(a[1:1 + n])
    torch.cuda.synchronize()
    pa, pb = a.data_ptr() + 1, b.data_ptr() + 2
    assert encoder.compare_device(pa, pb, n) == n
    b[2 + n - 1] ^= 0x80
    torch.cuda.synchronize()
    assert encoder.compare_device(pa, pb, n) == n - 1
    assert encoder.compare_device(pa, pb, n - 1) == n - 1
    b[2 + (1 << 32) + 3] ^= 1
    torch.cuda.synchronize()
    assert encoder.compare_device(pa, pb, n) == (1 << 32) + 3


def test_compare_device_refusals(encoder):
    import torch
    za = product()
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(za.ZadaError, match="null argument"):
        encoder.compare_device(None, t.data_ptr(), 5)
    with pytest.raises(za.ZadaError, match="1 TiB"):
        encoder.compare_device(t.data_ptr(), t.data_ptr(), 1 << 40)
    assert encoder.compare_device(None, None, 0) == 0
    assert encoder.compare_device(t.data_ptr() + 1, t.data_ptr() + 9, 50) == 50
    assert any(nm == "compare:k_cz_compare" for nm, _ in encoder.last_timing())


# ---- CompZip.compare_device ----
def source_list():
    """(raw name, bytes) in an order that is not the traversal's: texts of several sizes on both sides of a piece, an empty entry, random bytes, one
    entry above two pieces, a directory entry and a name with a backslash."""
    t = text()
    rnd = np.random.default_rng(3).integers(0, 256, 4096, dtype=np.uint8).tobytes()
    return [("zeta.txt", t[:PIECE + 1]), ("dir/", b""), ("alpha.txt", t[1000:1000 + PIECE - 1]), ("m\\back.txt", t[5000:5300]), ("empty", b""),
            ("random.bin", rnd), ("big.dat", t[20000:20000 + 100000]), ("dir/b.c", t[300000:300000 + PIECE]), ("Alpha.txt", t[7:24]), ("one", b"x")]


METHODS = (zipfile.ZIP_DEFLATED, zipfile.ZIP_BZIP2, zipfile.ZIP_LZMA, zipfile.ZIP_STORED)


def archive(entries, shift=0, comment=b""):
    """An archive written by zipfile, entry k with method (k + shift) mod 4."""
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as z:
        for k, (nm, d) in enumerate(entries):
            zi = zipfile.ZipInfo(nm)
            zi.filename = nm                                   # (zipfile turns os.sep into '/': keep a backslash as given wherever the test runs)
            z.writestr(zi, d, compress_type=zipfile.ZIP_STORED if nm.endswith("/") else METHODS[(k + shift) % 4])
        z.comment = comment
    return b.getvalue()


def on_device(data, offset):
    import torch
    h = np.full(offset + len(data), GUARD, dtype=np.uint8)
    h[offset:] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(h).cuda()[offset:], h


def run(enc, arc1, arc2, password=None, off1=3, off2=0):
    """CompZip.compare_device on the two archives at the given offsets modulo 16 of their tensors; asserts that neither tensor was written."""
    za = product()
    t1, h1 = on_device(arc1, off1)
    t2, h2 = on_device(arc2, off2)
    out = za.CompZip(enc).compare_device(za.ZipInfo.load_device(t1), za.ZipInfo.load_device(t2), password=password)
    assert np.array_equal(t1.cpu().numpy(), h1[off1:]) and np.array_equal(t2.cpu().numpy(), h2[off2:]), "an archive was written"
    return out


def same(out, z1, z2, damaged=0):
    c, entries = _rezip.comp_zip([(nm.encode(), d) for nm, d in z1], [(nm.encode(), d) for nm, d in z2])
    for nm, v in c.items():
        if nm == "total_differences":
            v += damaged
        assert getattr(out, nm) == v, (nm, getattr(out, nm), v, out)
    assert [(e[5], e[1], e[2]) for e in out.entries] == entries
    return c


def test_equal_archives_under_other_methods(encoder):
    """Every entry under another method in archive 2, which lacks the directory entry -- what the reference reports after a ReZip: one missing
    name, a directory, and nothing else."""
    src = source_list()
    out = run(encoder, archive(src, comment=b"first"), archive([e for e in src if e[0] != "dir/"], shift=1))
    c = same(out, src, [e for e in src if e[0] != "dir/"])
    assert out.size_failures == out.compare_failures == out.damaged == 0 and out.missing_1_in_2 == out.just_a_directory == 1
    assert out.total_bytes == sum(len(d) for _, d in src) and out.total_differences == 1 and c["total_1"] == len(src)
    assert [e[0] for e in out.entries][:3] == ["Alpha.txt", "alpha.txt", "big.dat"]
    assert out["big.dat"][1:4] == (_rezip.OK, 0, 100000)


def tampered(src):
    """(label, archive 2's list): an entry removed, one added, bytes changed at the first and last position, on both sides of a piece boundary and in
    two pieces at once, an entry one byte shorter and one byte longer, and several of these together."""
    d = dict(src)
    flip = lambda x, *at: bytes(b ^ (0x20 if i in at else 0) for i, b in enumerate(x))
    put = lambda **kw: [(nm, kw.get(nm.replace(".", "_").replace("/", "_"), x)) for nm, x in src]
    yield "removed", [e for e in src if e[0] != "random.bin"]
    yield "added", src + [("new.txt", b"hello")]
    yield "first byte", put(big_dat=flip(d["big.dat"], 0))
    yield "last byte", put(big_dat=flip(d["big.dat"], 99999))
    yield "end of a piece", put(big_dat=flip(d["big.dat"], 3 * PIECE - 1))
    yield "start of a piece", put(big_dat=flip(d["big.dat"], 3 * PIECE))
    yield "two pieces", put(big_dat=flip(d["big.dat"], 5 * PIECE + 9, 2 * PIECE + 100))
    yield "shorter", put(zeta_txt=d["zeta.txt"][:-1])
    yield "longer", put(alpha_txt=d["alpha.txt"] + b"!")
    yield "shorter with a difference", put(dir_b_c=flip(d["dir/b.c"], 77)[:-1])
    yield "emptied", put(one=b"")
    yield "filled", put(empty=b"y")
    yield "several", put(one=b"y", zeta_txt=flip(d["zeta.txt"], PIECE), empty=b"z", random_bin=d["random.bin"][:-1])[:-3] + [("q", b"")]


def test_tampered_copies(encoder):
    src = source_list()
    arc1 = archive(src)
    seen = set()
    for label, z2 in tampered(src):
        out = run(encoder, arc1, archive(z2, shift=2))
        c = same(out, src, z2)
        assert out.total_differences == c["total_differences"] >= 1, label
        seen |= {e[1] for e in out.entries}
    assert seen == {_rezip.OK, _rezip.DIFFERENT, _rezip.SHORTER, _rezip.LONGER, _rezip.MISSING}


def test_groups_give_the_same_verdicts(encoder):
    """batch_mib = 1: the 100 000 bytes of big.dat fill their group's two arenas with few neighbours, so the call takes several groups; every verdict is
    the one group's."""
    src = source_list() + [("more%d" % k, text()[k * 1000:k * 1000 + 150000]) for k in range(4)]
    z2 = [(nm, d if nm != "more2" else d[:149999] + b"#") for nm, d in src]
    encoder.set_knob("batch_mib", 1)
    try:
        out = run(encoder, archive(src), archive(z2, shift=3))
    finally:
        encoder.set_knob("batch_mib", 512)
    same(out, src, z2)
    assert out["more2"][1:3] == (_rezip.DIFFERENT, 150000)


def test_a_damaged_entry_on_either_side(encoder):
    """One payload byte of a Deflate entry flipped in archive 1, then in archive 2: that pair is CZ_DAMAGED with the reader's exception, every other
    verdict stands, and the call does not fail."""
    za = product()
    src = source_list()
    good = archive(src)
    info = za.ZipInfo.load(good)
    e = info["zeta.txt"]
    assert e.method == 8
    bad = bytearray(good)
    bad[e.data_offset + e.csize // 2] ^= 0x10
    for arcs in ((bytes(bad), good), (good, bytes(bad))):
        out = run(encoder, *arcs)
        assert out.damaged == 1 and out.total_differences == 1 and out.size_failures == out.compare_failures == 0
        name, v, pos, cmpd, err, key = out[b"zeta.txt"]
        assert v == _rezip.DAMAGED and isinstance(err, (za.DataError, za.CRCError, za.SizeError))
        assert sum(1 for x in out.entries if x[1] == _rezip.OK) == len(src) - 1
        assert out.total_bytes == sum(len(d) for nm, d in src if nm != "zeta.txt")


def test_with_a_password(encoder):
    """Archive 1 written by write_device_ex with a password, archive 2 by zipfile without: equal; the wrong password damages every encrypted pair;
    no password raises."""
    import torch
    za = product()
    src = [(nm, d) for nm, d in source_list() if not nm.endswith("/")]
    tens = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() if d else torch.empty(0, dtype=torch.uint8, device="cuda") for _, d in src]
    arc1 = za.ZipCreate(encoder, za.Method.Deflate_1).write_device_ex([nm for nm, _ in src], tens, password=PW, _headers=headers_for(len(src)))
    arc1 = arc1.cpu().numpy().tobytes()
    arc2 = archive(src)
    out = run(encoder, arc1, arc2, password=PW)
    same(out, src, src)
    assert out.total_differences == 0 and out.total_bytes == sum(len(d) for _, d in src)
    out = run(encoder, arc1, arc2, password="wrong")
    # (a wrong password passes an entry's check byte once in 256 times; the headers are fixed, so what happens here happens every time)
    assert out.damaged >= len(src) - 1 and sum(isinstance(e[4], za.WrongPassword) for e in out.entries) >= len(src) - 1
    with pytest.raises(za.WrongPassword):
        run(encoder, arc1, arc2)


def test_refusals_and_a_fresh_context(encoder):
    """The first call on a new Encoder is compare_device, then compzip_device; an unknown method raises in UnZip's words, a duplicate name as Zip.Load
    does, and the C entry point names the pair and the archive of a range beyond the archive."""
    import torch
    za = product()
    enc = za.Encoder(0)
    try:
        t = torch.from_numpy(_base.copy()).cuda()
        assert enc.compare_device(t.data_ptr() + 1, t.data_ptr() + 1, 1000) == 1000
        src = source_list()
        out = run(enc, archive(src), archive(src, shift=1))
        assert out.total_differences == 0 and out.common == len(src)
    finally:
        enc.close()
    src = source_list()
    arc = archive(src)
    info = za.ZipInfo.load(arc)
    bad = bytearray(arc)
    at = arc.rfind(b"PK\x01\x02" , 0, arc.rfind(b"one"))             # the central header of the last entry: its method field
    bad[at + 10] = 1
    with pytest.raises(za.UnsupportedMethod, match="Shrink"):
        run(encoder, bytes(bad), arc)
    with pytest.raises(za.UnsupportedMethod, match="Shrink"):          # ... also where archive 2 has no entry of that name
        run(encoder, bytes(bad), archive([x for x in src if x[0] != "one"]))
    with pytest.raises(za.ZadaError, match="appears twice"):
        run(encoder, archive(src + [("m/back.txt", b"dup")]), arc)
    t1, _ = on_device(arc, 0)
    dt = za.Encoder.unzip_dtypes()[0]
    ra, rb = np.zeros(2, dtype=dt), np.zeros(2, dtype=dt)
    e = info["one"]
    for tab in (ra, rb):
        tab["in_off"], tab["n_in"], tab["cap"], tab["method"] = e.data_offset, e.csize, e.usize, e.method
    rb["in_off"][1] = len(arc)
    with pytest.raises(za.ZadaError, match="pair 1, archive 2: its data lie beyond the archive"):
        encoder.compzip_device(t1.data_ptr(), len(arc), t1.data_ptr(), len(arc), ra, rb)
    rb["in_off"][1] = e.data_offset
    rb["flags"][0] = za.CZ_ABSENT
    r = encoder.compzip_device(t1.data_ptr(), len(arc), t1.data_ptr(), len(arc), ra, rb)
    assert [int(v) for v in r["verdict"]] == [za.CZ_MISSING, za.CZ_OK] and int(r["compared"][1]) == 1 and int(r["len_a"][0]) == 0
