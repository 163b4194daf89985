"""Find_Zip on the device (include/zada.h "a string searched in every entry of an archive that lies in device memory"): zada_find_device at every
alignment, text length and string length of the lists in tests/_findzip.py, with planted occurrences around every piece boundary and with bytes
around the buffer that would complete an occurrence if they were read; FindZip.find_device and zada_findzip_device on archives written on the host
by zipfile (all four of its methods, which the reader decodes) and by ZipCreate.write_device_ex with a password.  The reference is always the literal
restatement of tools/find_zip.adb in tests/_findzip.py, never the code under test."""
import io
import zipfile

import numpy as np
import pytest

import _findzip
from _common import product
from _devbuf import GUARD
from _zipdev import headers_for, text

pytestmark = pytest.mark.gpu
PIECE = _findzip.PIECE
PW = "p\xe4ssword"
ROOM = 1040                                                    # bytes in front of and behind the buffer in its tensor (a multiple of 16, above max)


# ---- zada_find_device ----
def find(enc, x, s, al, ignore_case=True, front=None, behind=None):
    """The entry x at offset ROOM + al of a tensor.  By default the bytes directly in front of it are the string itself as the search would need it
    (behind exclamation marks) -- its own head where an occurrence would begin in front of the buffer, and no spaces where the virtual ones are
    unless the string has them --, and the bytes behind it the string's tail, over and over.  -> (occurrences, first); asserts that the tensor was
    not written."""
    import torch
    given, s = s, s.encode("latin-1") if isinstance(s, str) else bytes(s)
    if front is None:
        front = b"!" * ROOM + s
    if behind is None:
        behind = (s[1:] or s) * ROOM
    h = np.full(ROOM + al + len(x) + ROOM, GUARD, dtype=np.uint8)
    h[al:ROOM + al] = np.frombuffer(front[-ROOM:].rjust(ROOM, b"!"), dtype=np.uint8)
    h[ROOM + al:ROOM + al + len(x)] = np.frombuffer(x, dtype=np.uint8)
    h[ROOM + al + len(x):ROOM + al + len(x) + ROOM - al] = np.frombuffer(behind[:ROOM - al], dtype=np.uint8)
    t = torch.from_numpy(h).cuda()
    torch.cuda.synchronize()
    got = enc.find_device(t.data_ptr() + ROOM + al, len(x), given, ignore_case)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), h), "the buffer was written"
    return got


@pytest.mark.parametrize("al", (0, 1, 15))
def test_find_device_every_text_and_string_length(encoder, al):
    """Every text length against every string length at this alignment, with the planted occurrences of _findzip.grid_cases: counts and first as the
    literal loop gives them."""
    hits = 0
    for x, s in _findzip.grid_cases():
        want = _findzip.reference(x, s)
        assert find(encoder, x, s, al) == want, (len(x), len(s), al)
        hits += want[0] > 0
    assert hits > 100
    assert {(len(x), len(s)) for x, s in _findzip.grid_cases()} >= {(n, k) for n in _findzip.TEXT_LENGTHS for k in _findzip.STRING_LENGTHS}


@pytest.mark.parametrize("al", (0, 1, 15))
def test_planted_occurrences_around_the_pieces(encoder, al):
    """One occurrence alone in a text of dots: at the first byte (its head are the virtual spaces), ending at the last byte, at PIECE - 1, at PIECE, at
    PIECE + stl - 2, and 1024 bytes around 2 PIECE -- found where it is, once."""
    n = 2 * PIECE + 700
    for stl in (1, 4, 5, 17, 64, 1024):
        body = bytes(0x41 + (i * 7 + i // 26) % 26 for i in range(stl - 1)) + b"#"
        for end in (stl - 1, n - 1, PIECE - 1, PIECE, PIECE + stl - 2, 2 * PIECE + 500):
            x = bytearray(b"." * n)
            x[end + 1 - stl:end + 1] = body
            assert find(encoder, bytes(x), body, al) == (1, end) == _findzip.reference(bytes(x), body), (stl, end)
        x = bytearray(b"." * n)
        x[0] = 0x23
        assert find(encoder, bytes(x), b" " * (stl - 1) + b"#", al) == (1, 0), stl


@pytest.mark.parametrize("al", (0, 1, 15))
def test_bytes_around_the_buffer_do_not_count(encoder, al):
    """Non-space bytes directly in front where the virtual spaces are expected; the string's own head directly in front where a real match would need
    it; the string's tail directly behind.  Neither counts."""
    assert find(encoder, b"ab...", b"  ab", al, front=b"#" * ROOM) == (1, 1)
    assert find(encoder, b"ab...", b"  ab", al, front=b"ab" * 520) == (1, 1)
    assert find(encoder, b"q ab", b"  ab", al, front=b" " * ROOM) == (0, 4)
    assert find(encoder, b"cd...", b"abcd", al, front=b"#" * (ROOM - 2) + b"ab") == (0, 5)
    assert find(encoder, b"..ab", b"abcd", al, behind=b"cd" * 520) == (0, 4)
    for stl in (5, 17, 300, 1024):
        s = bytes(0x61 + i % 23 for i in range(stl))
        for cut in (1, 4, stl // 2, stl - 1):                  # the string lies across the buffer's first byte, then across its end
            assert find(encoder, s[cut:] + b"....", s, al, front=b"!" * ROOM + s[:cut]) == (0, stl - cut + 4), (stl, cut)
            assert find(encoder, b"...." + s[:cut], s, al, behind=s[cut:] + b"!" * ROOM) == (0, cut + 4), (stl, cut)
        x = b"." * PIECE + s + b"."
        assert find(encoder, x, s, al) == (1, PIECE + stl - 1)


def test_virtual_spaces_overlaps_dense_candidates_and_case(encoder):
    """The named cases of _findzip.named_cases at alignments 0 and 5: "  ab" at position 1; 1024 spaces on five spaces give 5 with first = 0, and 0
    when the first byte is no space; "aaa" in 2 PIECE + 3 bytes of a; "b" + 40 "a" there: every position survives the filter, none is an occurrence;
    " " in all spaces: n; mixed-case ASCII and Latin-1 letters with ignore_case, 0xF7 / 0xD7 and 0xFF / 0xDF apart, exact bytes without."""
    seen = {}
    for x, s, fold in _findzip.named_cases():
        want = _findzip.reference(x, s, fold)
        for al in (0, 5):
            assert find(encoder, x, s, al, fold) == want, (len(x), s[:12], fold, al)
        seen[(len(x), s[:12], fold)] = want
    n = 2 * PIECE + 3
    assert seen[(42, b"  ab", True)] == (1, 1) and seen[(5, b" " * 12, True)] in ((5, 0), (0, 5))
    assert seen[(n, b"aaa", True)] == (n - 2, 2) and seen[(n, b"b" + b"a" * 11, True)] == (0, n) and seen[(n, b" ", True)] == (n, 0)
    assert seen[(36, b"\xf7", True)] == seen[(36, b"\xff", True)][:1] + (1,) == (9, 1) and seen[(36, b"\xd7", True)] == (9, 0)
    assert find(encoder, b"x    ", b" " * 1024, 3) == (0, 5) and find(encoder, b"     ", b" " * 1024, 3) == (5, 0)
    assert find(encoder, b"Stra\xdfe \xc4\xe4 stra\xdfe", "STRA\xdfE \xe4\xc4", 2) == (1, 8)
    assert find(encoder, b"abc ABC aBc", b"aBc", 2, ignore_case=False) == (1, 10) and find(encoder, b"abc ABC aBc", b"aBc", 2) == (3, 2)


def test_find_device_beyond_4_gib(encoder):
    """Offsets that need more than 32 bits: one tensor of 4 GiB + two pieces + 5 bytes at alignment 1.  All spaces with " ": every byte is an
    occurrence.  Zeros with one x three bytes behind 4 GiB: found there, once -- by the filter alone and through the confirmation."""
    import torch
    n = (1 << 32) + 2 * PIECE + 5
    t = torch.full((n + 16,), 0x20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert encoder.find_device(t.data_ptr() + 1, n, b" ") == (n, 0)
    t.zero_()
    t[1 + (1 << 32) + 3] = 0x78
    torch.cuda.synchronize()
    assert encoder.find_device(t.data_ptr() + 1, n, b"x") == (1, (1 << 32) + 3)
    assert encoder.find_device(t.data_ptr() + 1, n, b"\0" * 11 + b"x") == (1, (1 << 32) + 3)
    assert encoder.find_device(t.data_ptr() + 1, n, b"y") == (0, n)
    assert int(t[1 + (1 << 32) + 3]) == 0x78 and int(t[1 + (1 << 32) + 2]) == 0


def test_find_device_refusals(encoder):
    import torch
    za = product()
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(za.ZadaError, match="null argument"):
        encoder.find_device(None, 5, b"a")
    with pytest.raises(za.ZadaError, match="1 TiB"):
        encoder.find_device(t.data_ptr(), 1 << 40, b"a")
    with pytest.raises(za.ZadaError, match="a search string of 0 bytes"):
        encoder.find_device(t.data_ptr(), 64, b"")
    with pytest.raises(za.ZadaError, match="a search string of 1025 bytes"):
        encoder.find_device(t.data_ptr(), 64, b"a" * 1025)
    assert encoder.find_device(None, 0, b"a") == (0, 0)
    assert encoder.find_device(t.data_ptr() + 1, 50, b"\0") == (50, 0)
    assert any(nm == "find:k_fz_search" for nm, _ in encoder.last_timing())


# ---- FindZip.find_device ----
def source_list():
    """(raw name, bytes) in an order that is not the traversal's (test_gpu_rezip.py's list): texts of several sizes on both sides of a piece, an empty
    entry, random bytes, one entry above two pieces, a directory entry and a name with a backslash."""
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


def run(enc, arc, s, off=0, **kw):
    """FindZip.find_device on the archive at the given offset of its tensor; asserts that the tensor was not written."""
    za = product()
    t, h = on_device(arc, off)
    out = za.FindZip(enc).find_device(za.ZipInfo.load_device(t), s, **kw)
    assert np.array_equal(t.cpu().numpy(), h[off:]), "the archive was written"
    return out


_refs = {}


def same(out, src, s, skip=()):
    """Counts, first, in_names and lines () against _findzip.find_zip on the source list (computed once per string); skip: keys left out of the
    contents (damaged entries)."""
    s = s.encode("latin-1") if isinstance(s, str) else s
    if s not in _refs:
        _refs[s] = _findzip.find_zip([(nm.encode("latin-1"), d) for nm, d in src], s)
    contents, names, lines = _refs[s]
    contents = [c for c in contents if c[0] not in skip]
    assert [(e[4], e[1], e[2]) for e in out.entries if e[1] > 0] == contents
    assert out.in_contents == [(c[0], c[1]) for c in contents] and out.in_names == names
    if not skip:
        assert out.lines() == lines
        lens = {nm.encode("latin-1").replace(b"\\", b"/"): len(d) for nm, d in src}
        assert all(e[2] == lens[e[4]] for e in out.entries if e[1] == 0)           # first = the entry's length where nothing was found
    return contents, names


def strings(src):
    d = dict(src)
    several = d["big.dat"][40000:40006]                        # six bytes of the generators' text
    return several, b"no such string \xa4\x01 anywhere", "ALPHA", b" x"


@pytest.mark.parametrize("off", (0, 3))
def test_findzip_against_the_literal_tool(encoder, off):
    """A string present in several entries, one absent from all, one found only in names, and one with a leading space that hits an entry's first
    byte -- the archive at this offset of its tensor."""
    src = source_list()
    arc = archive(src, comment=b"find")
    several, absent, only_name, spaced = strings(src)
    outs = {}
    for s in (several, absent, only_name, spaced):
        outs[s] = run(encoder, arc, s, off)
        same(outs[s], src, s)
        assert outs[s].damaged == 0 and len(outs[s].entries) == len(src)
    assert len(outs[several].in_contents) >= 3
    assert outs[absent].in_contents == [] and outs[absent].in_names == [] and outs[absent].lines() == []
    assert outs[only_name].in_names == [b"Alpha.txt", b"alpha.txt"] and outs[only_name].lines()[-1] == " Found in [alpha.txt]'s entry name"
    assert (b"one", 1) in outs[spaced].in_contents and outs[spaced][b"one"][1:3] == (1, 0)
    assert [e[0] for e in outs[several].entries][:3] == ["Alpha.txt", "alpha.txt", "big.dat"] and outs[several]["m\\back.txt"][4] == b"m/back.txt"
    assert any(nm == "findzip:k_fz_search" for nm, _ in encoder.last_timing())


def test_groups_give_the_same_result(encoder):
    """batch_mib = 1: three more entries of 330 000 bytes, so the call takes several groups; every count is the one group's, and the literal tool's."""
    src = source_list() + [("more%d" % k, text()[k * 1000:k * 1000 + 330000]) for k in range(3)]
    arc = archive(src, shift=1)
    several = strings(src)[0]
    one = run(encoder, arc, several, 3)
    encoder.set_knob("batch_mib", 1)
    try:
        grouped = run(encoder, arc, several, 3)
    finally:
        encoder.set_knob("batch_mib", 512)
    assert grouped.entries == one.entries and grouped.lines() == one.lines()
    contents, names, lines = _findzip.find_zip([(nm.encode("latin-1"), d) for nm, d in src], several)
    assert [(e[4], e[1], e[2]) for e in grouped.entries if e[1] > 0] == contents and grouped.lines() == lines and len(contents) >= 5


def test_case_and_names(encoder):
    """ignore_case = False finds exact bytes only, in contents and in names; a str is taken as Latin-1; the names come out in Latin-1 lower case."""
    src = [("Strasse.TXT", b"Gro\xdfe STRA\xdfE, stra\xdfe \xc4\xe4"), ("b\\Q.txt", b"\xe4 \xc4"), ("c", b"")]
    arc = archive(src)
    for s, fold in (("stra\xdfe", True), ("stra\xdfe", False), ("\xe4", True), ("\xe4", False), (".txt", True), (".txt", False), ("/q", True), ("\\Q", False)):
        out = run(encoder, arc, s, 1, ignore_case=fold)
        contents, names, lines = _findzip.find_zip([(nm.encode("latin-1"), d) for nm, d in src], s.encode("latin-1"), fold)
        assert [(e[4], e[1], e[2]) for e in out.entries if e[1] > 0] == contents and out.in_names == names and out.lines() == lines, (s, fold)
    assert run(encoder, arc, "\xe4", 1).lines() == ["    2 in [strasse.txt]'s contents", "    2 in [b/q.txt]'s contents"]
    assert run(encoder, arc, ".TXT", 1, ignore_case=False).lines() == [" Found in [strasse.txt]'s entry name"]


def test_a_damaged_entry(encoder):
    """One payload byte of a Deflate entry flipped: that entry is damaged with the reader's exception, every other count stands, and the call does not
    fail."""
    za = product()
    src = source_list()
    good = archive(src)
    info = za.ZipInfo.load(good)
    e = info["zeta.txt"]
    assert e.method == 8
    bad = bytearray(good)
    bad[e.data_offset + e.csize // 2] ^= 0x10
    several = dict(src)["zeta.txt"][200:205]
    ref = run(encoder, good, several)
    assert ref[b"zeta.txt"][1] > 0
    out = run(encoder, bytes(bad), several, 3)
    name, occ, first, err, key = out[b"zeta.txt"]
    assert (occ, first) == (0, 0) and isinstance(err, (za.DataError, za.CRCError, za.SizeError)) and out.damaged == 1
    assert [x for x in out.entries if x[4] != b"zeta.txt"] == [x for x in ref.entries if x[4] != b"zeta.txt"]
    same(out, src, several, skip=(b"zeta.txt",))


def test_with_a_password(encoder):
    """An archive written by write_device_ex with a password: found with the password, the wrong one damages the encrypted entries, none raises."""
    import torch
    za = product()
    src = [(nm, d) for nm, d in source_list() if not nm.endswith("/")]
    tens = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() if d else torch.empty(0, dtype=torch.uint8, device="cuda") for _, d in src]
    arc = za.ZipCreate(encoder, za.Method.Deflate_1).write_device_ex([nm for nm, _ in src], tens, password=PW, _headers=headers_for(len(src)))
    arc = arc.cpu().numpy().tobytes()
    several = strings(src)[0]
    out = run(encoder, arc, several, 3, password=PW)
    same(out, src, several)
    assert out.damaged == 0 and len(out.in_contents) >= 3
    out = run(encoder, arc, several, password="wrong")
    # (a wrong password passes an entry's check byte once in 256 times; the headers are fixed, so what happens here happens every time)
    assert out.damaged >= len(src) - 1 and sum(isinstance(x[3], za.WrongPassword) for x in out.entries) >= len(src) - 1
    with pytest.raises(za.WrongPassword):
        run(encoder, arc, several)


def test_refusals_and_a_fresh_context(encoder):
    """The first call on a new Encoder is find_device, then findzip_device; a string of 0 and of 1025 bytes is a ValueError, an unknown method raises
    in UnZip's words, a duplicate name as Zip.Load does, and the C entry point names the row of a range beyond the archive."""
    import torch
    za = product()
    src = source_list()
    arc = archive(src)
    several = strings(src)[0]
    enc = za.Encoder(0)
    try:
        t = torch.from_numpy(np.frombuffer(b"." * 999 + b"q", dtype=np.uint8).copy()).cuda()
        assert enc.find_device(t.data_ptr() + 1, 999, b"....Q") == (1, 998)
        out = run(enc, arc, several, 3)
        assert enc.find_device(t.data_ptr(), 1000, b".") == (999, 0)
    finally:
        enc.close()
    same(out, src, several)
    assert za.FindZip(encoder).find(arc, several).entries == out.entries
    for bad_text in (b"", "", b"a" * 1025):
        with pytest.raises(ValueError, match="1 .. 1024"):
            run(encoder, arc, bad_text)
    bad = bytearray(arc)
    at = arc.rfind(b"PK\x01\x02", 0, arc.rfind(b"one"))             # the central header of the last entry: its method field
    bad[at + 10] = 1
    with pytest.raises(za.UnsupportedMethod, match="Shrink"):
        run(encoder, bytes(bad), several)
    with pytest.raises(za.ZadaError, match="appears twice"):
        run(encoder, archive(src + [("m/back.txt", b"dup")]), several)
    with pytest.raises(za.ZadaError, match="not made by ZipInfo.load_device"):
        za.FindZip(encoder).find_device(za.ZipInfo.load(arc), several)
    info = za.ZipInfo.load(arc)
    t1, _ = on_device(arc, 0)
    rows = np.zeros(2, dtype=za.Encoder.unzip_dtypes()[0])
    e = info["one"]
    rows["in_off"], rows["n_in"], rows["cap"], rows["method"] = e.data_offset, e.csize, e.usize, e.method
    rows["in_off"][1] = len(arc)
    with pytest.raises(za.ZadaError, match="entry 1: its data lie beyond the archive"):
        encoder.findzip_device(t1.data_ptr(), len(arc), rows, b"x")
    rows["in_off"][1] = e.data_offset
    rows["flags"][1] = 1
    with pytest.raises(za.ZadaError, match="entry 1: encrypted, and no keys were given"):
        encoder.findzip_device(t1.data_ptr(), len(arc), rows, b"x")
    rows["flags"][1] = 0
    rows["out_off"] = 1 << 50                                        # ignored
    r = encoder.findzip_device(t1.data_ptr(), len(arc), rows, b" x")
    assert [int(v) for v in r["occurrences"]] == [1, 1] and [int(v) for v in r["first"]] == [0, 0] and [int(v) for v in r["rc"]] == [0, 0]
    with pytest.raises(za.ZadaError, match="a search string of 1025 bytes"):
        encoder.findzip_device(t1.data_ptr(), len(arc), rows, b"a" * 1025)
    assert len(encoder.findzip_device(t1.data_ptr(), len(arc), rows[:0], b"a")) == 0
