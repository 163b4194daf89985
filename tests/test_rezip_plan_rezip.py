"""The host plan of zada_rezip_device (zip-ada_amd/csrc/zada_rezip_plan.h: the considered approaches, the choice as a closed form, the methods to
run, ReZip's headers, argument checks, bound and groups) through tests/rezip/rezip_plan_host.cpp, against the approach loop and the header writing
restated from the Ada text in tests/_rezip.py; the choices once more through a program of its own built with -fsanitize=address,undefined.  No GPU."""
import ctypes
import io
import itertools
import os
import subprocess
import zipfile

import numpy as np
import pytest

import _rezip
from _common import product

E_INVALID, E_TOO_LARGE = -1, -4
NT = _rezip.NOT_TRIED
GIB4 = 1 << 32


@pytest.fixture(scope="module")
def plan():
    return _rezip.load_plan()


def dtype():
    return product().Encoder.rezip_dtypes()[0]


def choose(plan, size, allowed):
    arr = (ctypes.c_uint64 * 12)(*size)
    return plan.rp_choose(arr, 1 if allowed else 0)


def test_choice_against_the_literal_loop(plan):
    """Sizes in {0, 1, 2, 3} for original and four other approaches, every subset of the four considered, original's format allowed or not:
    4 ** 5 * 16 * 2 tables.  The four sit at ranks 1, 5, 7 and 10."""
    ranks = (1, 5, 7, 10)
    cases = 0
    for sizes in itertools.product(range(4), repeat=5):
        for subset in range(16):
            consider = [a == 0 or (a in ranks and (subset >> ranks.index(a)) & 1) for a in range(12)]
            size = [NT] * 12
            size[0] = sizes[0]
            for j, a in enumerate(ranks):
                if consider[a]:
                    size[a] = sizes[j + 1]
            for allowed in (True, False):
                want = _rezip.try_all_approaches(consider, [0 if x == NT else x for x in size], allowed)
                assert choose(plan, size, allowed) == want, (size, allowed)
                cases += 1
    assert cases == 4 ** 5 * 16 * 2


def test_named_format_sets_over_the_source_formats(plan):
    for formats in (_rezip.ALL_FORMATS, _rezip.DEFLATE_OR_STORE, _rezip.FAST_DECOMPRESSION):
        consider = _rezip.consider_a_priori(0x0FE7, formats)
        assert plan.rp_considered(0x0FE7, formats) == sum(1 << a for a in range(12) if consider[a])
        assert plan.rp_considered(0x0FE7 & ~1, formats) & 1                    # bit 0 is always taken as set
        for zt in (0, 8, 9, 12, 14):
            allowed = bool((formats >> _rezip.FORMAT_BIT[zt]) & 1)
            for sizes in ((5, 5), (5, 9), (9, 5)):
                size = [sizes[1] if consider[a] else NT for a in range(12)]
                size[0] = sizes[0]
                assert choose(plan, size, allowed) == _rezip.try_all_approaches(consider, [0 if x == NT else x for x in size], allowed)
    assert plan.rp_considered(0x0FE7, _rezip.DEFLATE_OR_STORE) == 1 | 1 << 5 | 1 << 6
    assert plan.rp_considered(0x0FE7, _rezip.FAST_DECOMPRESSION) == 1 | 1 << 5 | 1 << 6 | 1 << 10 | 1 << 11


def presel_names():
    return ["a.txt", "b.JPG", "c.orf", "d.zip", "e.adb", "f.pgm", "g.png", "h.mp3", "i.wav", "j.bin", "k.arw", "l.gif", "m.mp4", "n.au", "o.ppm", "p.jar", "noext"]


def test_methods_to_run(plan):
    """Against preselect / guess_type_from_name, on names of every content type and sizes on both sides of every threshold zada_preselect has."""
    za = product()
    out = (ctypes.c_int * 12)()
    seen = set()
    for nm in presel_names():
        for n in (0, 1, 4999, 5000, 5001, 8999, 9000, 9001, 15999, 16000, 16001, 1 << 20):
            p2 = za.preselect(35, za.guess_type_from_name(nm), n)
            p1 = za.preselect(34, za.guess_type_from_name(nm), n)
            for approaches, formats in ((0x0FE7, 0x1F), (0x27, 0x1F), (0x0FE7, 0x03), (0x0C06, 0x1F)):
                consider = _rezip.consider_a_priori(approaches, formats)
                want = sorted({p2 if a == 1 else p1 if a == 2 else _rezip.METHOD[a] for a in range(1, 12) if consider[a]})
                k = plan.rp_methods(plan.rp_considered(approaches, formats), p2, p1, out)
                assert list(out[:k]) == want
                seen.add(len(want))
    assert len(seen) >= 3


def table(rows):
    """rows: (name bytes, in_off, n_in, usize, method, flags) -> (structured array, the names' buffer to keep alive)"""
    tab = np.zeros(len(rows), dtype=dtype())
    blob = np.frombuffer(b"".join(r[0] for r in rows) + b"\0", dtype=np.uint8)
    at = 0
    for k, (nm, in_off, n_in, usize, method, flags) in enumerate(rows):
        tab[k] = (in_off, n_in, usize, 0x1234 + k, 0x5A210000 + k, method, flags, 20 + k % 3, 0, len(nm), 0, blob.ctypes.data + at)
        at += len(nm)
    return tab, blob


def archive(plan, rows, winners, base=0, comment=b""):
    """-> (the plan's header bytes, offsets, archive length) and the model's, for winners (csize, zip type, eos) per row"""
    tab, blob = table(rows)
    n = len(rows)
    cs = np.array([w[0] for w in winners], dtype=np.uint64)
    zt = np.array([w[1] for w in winners], dtype=np.uint16)
    eos = np.array([w[2] for w in winners], dtype=np.uint8)
    cap = 200 * n + sum(2 * len(r[0]) for r in rows) + len(comment) + 200
    out = np.zeros(cap, dtype=np.uint8)
    offs = np.zeros(n + 1, dtype=np.uint64)
    alen = ctypes.c_uint64(0)
    used = plan.rp_rz_archive(tab.ctypes.data, n, cs.ctypes.data, zt.ctypes.data, eos.ctypes.data, base, comment, len(comment), out.ctypes.data, cap, offs.ctypes.data,
                              ctypes.byref(alen))
    assert used <= cap
    kept = [(r, w, t) for r, w, t in zip(rows, winners, tab) if r[0] and r[0][-1:] not in (b"/", b"\\")]
    model = [dict(name=r[0], version=int(t["version"]), flags=r[5], time=int(t["time"]), crc=int(t["crc"]), usize=r[3], csize=w[0], zip_type=w[1], eos=w[2], payload=None)
             for r, w, t in kept]
    body, tail, moffs, total = _rezip.rezip_archive(model, base, comment)
    assert out[:used].tobytes() == body + tail
    assert [int(x) for x in offs[:len(kept)]] == moffs and alen.value == total
    if all(w[0] <= max(r[2], r[3]) for r, w in zip(rows, winners)):          # (a winner is never longer than the source's stream or the Store fallback)
        assert plan.rp_rz_bound(n, tab.ctypes.data, len(comment)) >= total
    return model, body, tail, total


def test_archive_bytes_against_the_model(plan):
    """Made-up winners, payloads as lengths only: sizes and bases on both sides of 4 GiB (the local short extension, the central long one, the end
    records with and without Zip64), the comment kept and deleted, dropped directory entries, flag bits 1 and 3 set in the source."""
    rows = [(b"a.txt", 0, 10, 100, 8, 0x0808), (b"dir/", 0, 0, 0, 0, 0), (b"b\\", 0, 0, 0, 0, 0), (b"l.bin", 0, 50, 70, 14, 0x0802), (b"", 0, 0, 0, 0, 0), (b"s", 0, 5, 5, 0, 0x000A)]
    win = [(9, 8, 0), (0, 0, 0), (0, 0, 0), (50, 14, 1), (0, 0, 0), (5, 0, 0)]
    for base in (0, 77, GIB4 - 60, GIB4 - 1, GIB4, GIB4 + 5):
        for comment in (b"", b"kept comment"):
            model, body, tail, _ = archive(plan, rows, win, base, comment)
            assert len(model) == 3
            assert (b"PK\x06\x06" in tail) == (base + 129 >= GIB4 - 1)          # the last entry's offset: two headers of 35 bytes, 9 + 50 of payload
    for big in (GIB4 - 2, GIB4 - 1, GIB4, GIB4 + 7):
        for which in ("csize", "usize"):
            r = [(b"x", 0, 10, big if which == "usize" else 100, 8, 0), (b"y", 0, 10, 20, 8, 0)]
            w = [(big if which == "csize" else 9, 8, 0), (15, 8, 0)]
            model, body, tail, _ = archive(plan, r, w)
            assert (b"PK\x06\x07" in tail) == (big >= GIB4 - 1 or which == "csize")      # (behind such a stream the next entry's offset asks for it)
    # flag bits: 1 and 3 cleared, bit 1 set again for a winner that ends on a marker, the others kept
    model, body, _, _ = archive(plan, rows, win)
    flags = [int.from_bytes(body[at + 6:at + 8], "little") for at in (0, 35, 70)]       # (headers of 30 + 5, 30 + 5 and 30 + 1 bytes, no payloads)
    assert flags == [0x0800, 0x0802, 0x0000]


def test_zipfile_opens_the_small_model_archives(plan):
    rows = [(b"a.txt", 0, 4, 4, 0, 0), (b"sub/b.bin", 0, 0, 0, 0, 0), (b"dir/", 0, 0, 0, 0, 0), (b"c", 0, 11, 11, 0, 8)]
    pay = {b"a.txt": b"abcd", b"sub/b.bin": b"", b"c": b"hello world"}
    win = [(len(pay.get(r[0], b"")), 0, 0) for r in rows]
    tab, blob = table(rows)
    import zlib
    model = [dict(name=r[0], version=20, flags=r[5], time=0x5A210000, crc=zlib.crc32(pay[r[0]]), usize=r[3], csize=r[3], zip_type=0, eos=0, payload=pay[r[0]])
             for r in rows if r[0] != b"dir/"]
    body, tail, _, total = _rezip.rezip_archive(model, 0, b"note")
    assert len(body + tail) == total
    with zipfile.ZipFile(io.BytesIO(body + tail)) as z:
        assert [(i.filename, i.file_size, i.compress_type) for i in z.infolist()] == [("a.txt", 4, 0), ("sub/b.bin", 0, 0), ("c", 11, 0)]
        assert z.read("c") == b"hello world" and z.comment == b"note" and z.testzip() is None


def rz_check(plan, rows, src_len=1000, d_src=1 << 20, d_archive=1 << 50, cap=1 << 20):
    tab, blob = table(rows)
    bad, why = ctypes.c_int(9), ctypes.c_int(9)
    rc = plan.rp_rz_check(tab.ctypes.data, len(rows), d_src, src_len, d_archive, cap, ctypes.byref(bad), ctypes.byref(why))
    return rc, bad.value, plan.rp_rz_why_text(why.value).decode()


def test_every_argument_check_with_its_text_and_index(plan):
    good = [(b"a", 0, 10, 20, 8, 0), (b"b", 10, 10, 20, 0, 0), (b"c/", 0, 0, 0, 0, 0), (b"d", 990, 10, 5, 14, 2)]
    assert rz_check(plan, good) == (0, -1, "")
    for at in (0, 3):
        def with_(row):
            r = list(good)
            r[at] = row
            return r
        assert rz_check(plan, with_((b"q", 991, 10, 5, 8, 0))) == (E_INVALID, at, "its data lie beyond the source archive")
        assert rz_check(plan, with_((b"q", 1001, 0, 5, 8, 0)))[:2] == (E_INVALID, at)
        assert rz_check(plan, with_((b"q", 0, 10, 5, 1, 0))) == (E_INVALID, at, "unknown source method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)")
        assert rz_check(plan, with_((b"q", 0, 10, 5, 8, 0x0801))) == (E_INVALID, at, "encrypted (ReZip reads without a password)")
        assert rz_check(plan, with_((b"q", 0, 1 << 40, 5, 8, 0)), src_len=1 << 41) == (E_TOO_LARGE, at, "a stream or an entry of 1 TiB or more")
        assert rz_check(plan, with_((b"q", 0, 10, 1 << 40, 8, 0))) == (E_TOO_LARGE, at, "a stream or an entry of 1 TiB or more")
    assert rz_check(plan, good + [(b"b", 0, 1, 1, 0, 0)]) == (E_INVALID, 4, "the same name as an earlier entry")
    assert rz_check(plan, [good[0], (b"c/", 0, 0, 0, 0, 0)] + good[1:]) == (E_INVALID, 3, "the same name as an earlier entry")
    for d_archive, cap, hit in ((1 << 20, 1, True), ((1 << 20) + 999, 5, True), ((1 << 20) + 1000, 5, False), ((1 << 20) - 5, 5, False), ((1 << 20) - 5, 6, True)):
        assert (rz_check(plan, good, d_archive=d_archive, cap=cap) == (E_INVALID, -1, "the archive buffer overlaps the source archive")) == hit


def test_entry_limit_bound_and_groups(plan):
    """65 534 kept entries pass, 65 535 are refused; dropped ones do not count.  Groups: consecutive kept entries within the limit, an entry above
    4 MiB alone."""
    names = [b"%05x" % k for k in range(65535)]
    rows = [(nm, 0, 0, 0, 0, 0) for nm in names]
    assert rz_check(plan, rows[:65534] + [(b"d/", 0, 0, 0, 0, 0)])[0] == 0
    rc, bad, text = rz_check(plan, rows)
    assert (rc, bad) == (E_TOO_LARGE, -1) and "65 534" in text
    MIB4 = 4 << 20
    rows = [(b"a", 0, 1, 300, 8, 0), (b"b", 0, 1, 256, 8, 0), (b"d/", 0, 0, 0, 0, 0), (b"c", 0, 1, MIB4 + 1, 8, 0), (b"e", 0, 1, MIB4, 8, 0), (b"f", 0, 1, 1, 8, 0)]
    tab, blob = table(rows)
    ends = (ctypes.c_int * 8)()

    def groups(limit):
        return list(ends[:plan.rp_rz_groups(tab.ctypes.data, len(rows), limit, ends, 8)])
    assert groups(1 << 30) == [3, 4, 6]
    assert groups(512) == [1, 3, 4, 5, 6]
    assert groups(768) == [3, 4, 5, 6]
    assert plan.rp_rz_bound(len(rows), tab.ctypes.data, 7) == 56 + 20 + 22 + 7 + sum(124 + 2 + max(r[2], r[3]) for r in rows if r[0] != b"d/")


ARCHIVE_ROWS = [(b"a.txt", 0, 10, 100, 8, 0x0808), (b"dir/", 0, 0, 0, 0, 0), (b"b\\", 0, 0, 0, 0, 0), (b"l.bin", 0, 50, 70, 14, 0x0802), (b"", 0, 0, 0, 0, 0), (b"s", 0, 5, 5, 0, 0x000A)]
ARCHIVE_WIN = [(9, 8, 0), (0, 0, 0), (0, 0, 0), (50, 14, 1), (0, 0, 0), (5, 0, 0)]


def archive_lists():
    """The lists of test_archive_bytes_against_the_model: (rows, winners, base, comment)"""
    out = [(ARCHIVE_ROWS, ARCHIVE_WIN, base, comment) for base in (0, 77, GIB4 - 60, GIB4 - 1, GIB4, GIB4 + 5) for comment in (b"", b"kept comment")]
    for big in (GIB4 - 2, GIB4 - 1, GIB4, GIB4 + 7):
        for which in ("csize", "usize"):
            out.append(([(b"x", 0, 10, big if which == "usize" else 100, 8, 0), (b"y", 0, 10, 20, 8, 0)], [(big if which == "csize" else 9, 8, 0), (15, 8, 0)], 0, b""))
    return out


def check_lists():
    """The tables of test_every_argument_check_with_its_text_and_index and test_entry_limit_bound_and_groups: (rows, src_len, d_archive, cap, limit)"""
    good = [(b"a", 0, 10, 20, 8, 0), (b"b", 10, 10, 20, 0, 0), (b"c/", 0, 0, 0, 0, 0), (b"d", 990, 10, 5, 14, 2)]
    out = [(good, 1000, 1 << 50, 1 << 20, 1 << 30), ([], 0, 1 << 50, 0, 1), ([(b"", 0, 0, 0, 0, 0), (b"", 0, 0, 0, 0, 0)], 10, 1 << 50, 5, 1)]
    for at in (0, 3):
        for row, src_len in (((b"q", 991, 10, 5, 8, 0), 1000), ((b"q", 1001, 0, 5, 8, 0), 1000), ((b"q", 0, 10, 5, 1, 0), 1000), ((b"q", 0, 10, 5, 8, 0x0801), 1000),
                             ((b"q", 0, 1 << 40, 5, 8, 0), 1 << 41), ((b"q", 0, 10, 1 << 40, 8, 0), 1000)):
            r = list(good)
            r[at] = row
            out.append((r, src_len, 1 << 50, 1 << 20, 1 << 30))
    out.append((good + [(b"b", 0, 1, 1, 0, 0)], 1000, 1 << 50, 1 << 20, 1 << 30))
    out.append(([good[0], (b"c/", 0, 0, 0, 0, 0)] + good[1:], 1000, 1 << 50, 1 << 20, 1 << 30))
    for d_archive, cap in ((1 << 20, 1), ((1 << 20) + 999, 5), ((1 << 20) + 1000, 5), ((1 << 20) - 5, 5), ((1 << 20) - 5, 6)):
        out.append((good, 1000, d_archive, cap, 1 << 30))
    names = [(b"%05x" % k, 0, 0, 0, 0, 0) for k in range(65535)]
    out.append((names[:65534] + [(b"d/", 0, 0, 0, 0, 0)], 1000, 1 << 50, 1 << 20, 1 << 30))
    out.append((names, 1000, 1 << 50, 1 << 20, 1 << 30))
    MIB4 = 4 << 20
    g = [(b"a", 0, 1, 300, 8, 0), (b"b", 0, 1, 256, 8, 0), (b"d/", 0, 0, 0, 0, 0), (b"c", 0, 1, MIB4 + 1, 8, 0), (b"e", 0, 1, MIB4, 8, 0), (b"f", 0, 1, 1, 8, 0)]
    out += [(g, 1000, 1 << 50, 1 << 20, limit) for limit in (1 << 30, 512, 768)]
    return out


def fnv1a64(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_plan_under_the_sanitizers(plan, tmp_path):
    """A program of its own (its own main, -fsanitize=address,undefined), run as a child process, every name an exact-size heap block: the entry tables
    of the check and group tests (against the library loaded here, which those tests hold to their expectations), the archives of made-up winners
    (length, header bytes and their FNV-1a hash, offsets: against the Python model) and the methods to run (against preselect)."""
    za = product()
    exe = str(tmp_path / "rezip_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DREZIP_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe, _rezip.SRC],
                   check=True)
    hx = lambda b: b.hex() if b else "-"
    lines, want = [], []
    D_SRC = 1 << 20
    for rows, src_len, d_archive, cap, limit in check_lists():
        lines.append("e %d %d %d %d %d %d 7" % (len(rows), src_len, D_SRC, d_archive, cap, limit))
        lines += ["%s %d %d %d %d %d" % ((hx(r[0]),) + tuple(r[1:])) for r in rows]
        tab, blob = table(rows)
        bad, why = ctypes.c_int(9), ctypes.c_int(9)
        rc = plan.rp_rz_check(tab.ctypes.data if len(rows) else None, len(rows), D_SRC, src_len, d_archive, cap, ctypes.byref(bad), ctypes.byref(why))
        ends = (ctypes.c_int * (len(rows) + 1))()
        ng = plan.rp_rz_groups(tab.ctypes.data if len(rows) else None, len(rows), limit, ends, len(rows) + 1)
        want.append("%d %d %d | %d | groups:%s" % (rc, bad.value, why.value, plan.rp_rz_bound(len(rows), tab.ctypes.data if len(rows) else None, 7),
                                                  "".join(" %d" % e for e in ends[:ng])))
    for rows, win, base, comment in archive_lists():
        tab, blob = table(rows)
        lines.append("a %d %d %s" % (len(rows), base, hx(comment)))
        lines += ["%s %d %d %d %d %d %d %d %d" % (hx(r[0]), r[3], r[5], int(t["version"]), int(t["time"]), int(t["crc"]), w[0], w[1], w[2]) for r, w, t in zip(rows, win, tab)]
        kept = [(r, w, t) for r, w, t in zip(rows, win, tab) if r[0] and r[0][-1:] not in (b"/", b"\\")]
        model = [dict(name=r[0], version=int(t["version"]), flags=r[5], time=int(t["time"]), crc=int(t["crc"]), usize=r[3], csize=w[0], zip_type=w[1], eos=w[2], payload=None)
                 for r, w, t in kept]
        body, tail, offs, total = _rezip.rezip_archive(model, base, comment)
        want.append("%d %d %d |%s" % (total, len(body + tail), fnv1a64(body + tail), "".join(" %d" % o for o in offs)))
    for nm in presel_names():
        for n in (0, 4999, 5001, 9001, 16001, 1 << 20):
            p2, p1 = za.preselect(35, za.guess_type_from_name(nm), n), za.preselect(34, za.guess_type_from_name(nm), n)
            for approaches, formats in ((0x0FE7, 0x1F), (0x27, 0x1F), (0x0FE7, 0x03), (0x0C06, 0x1F)):
                consider = _rezip.consider_a_priori(approaches, formats)
                lines.append("m %d %d %d %d" % (approaches, formats, p2, p1))
                want.append("".join("%d " % m for m in sorted({p2 if a == 1 else p1 if a == 2 else _rezip.METHOD[a] for a in range(1, 12) if consider[a]})))
    src = tmp_path / "lists.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert got[-1] == "plan ok" and len(got) - 1 == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.rstrip() == w.rstrip(), (k, lines[:0], g, w)


def test_the_choices_under_the_sanitizers(plan, tmp_path):
    """A program of its own (its own main, -fsanitize=address,undefined), run as a child process on a third of the tables of the first test."""
    exe = str(tmp_path / "rezip_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DREZIP_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe, _rezip.SRC],
                   check=True)
    ranks = (1, 5, 7, 10)
    lines, want = [], []
    for k, sizes in enumerate(itertools.product(range(4), repeat=5)):
        if k % 3:
            continue
        for subset in range(16):
            consider = [a == 0 or (a in ranks and (subset >> ranks.index(a)) & 1) for a in range(12)]
            size = [NT] * 12
            size[0] = sizes[0]
            for j, a in enumerate(ranks):
                if consider[a]:
                    size[a] = sizes[j + 1]
            for allowed in (1, 0):
                lines.append("c %d %s" % (allowed, " ".join(str(x) for x in size)))
                want.append(str(_rezip.try_all_approaches(consider, [0 if x == NT else x for x in size], bool(allowed))))
    src = tmp_path / "choices.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert got[-1] == "plan ok" and got[:-1] == want
