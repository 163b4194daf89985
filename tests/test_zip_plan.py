"""The host plan of zada_zip_device (zip-ada_amd/csrc/zada_zip_plan.h: argument checks, groups, every header byte, the copy jobs) through
tests/zip/zip_plan_host.cpp, against ZipCreate.add_compressed + finish -- Python only, pinned to the oracle by test_oracle.py -- and a restatement of
the groups in Python; the same lists once more through a program of its own built with -fsanitize=address,undefined.  No GPU, and nothing is loaded
into this interpreter with a sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _common import ROOT, plan_library, product

E_INVALID, E_TOO_LARGE = -1, -4
W_NULL, W_NAME, W_TOO_LARGE, W_OVERLAP = 1, 2, 3, 4
G_BATCH, G_SINGLE, G_STORE = 0, 1, 2
K_BLOB, K_STREAM, K_DATA = 0, 1, 2
TIB, MIB4, M64 = 1 << 40, 4 << 20, (1 << 64) - 1
DT = np.dtype([("d_data", "<u8"), ("n", "<u8"), ("name", "<u8"), ("name_len", "<u4"), ("time", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
DT_RES = np.dtype([("rc", "<i4"), ("zip_type", "<u2"), ("pad", "<u2"), ("crc", "<u4"), ("pad2", "<u4"), ("csize", "<u8"), ("offset", "<u8")])
SRC = os.path.join(ROOT, "tests", "zip", "zip_plan_host.cpp")
MARGIN = 22 + 56 + 20 + 2 ** 16 + 10


@pytest.fixture(scope="module")
def plan():
    L = ctypes.CDLL(plan_library("zip", "zip_plan_host", "zada_zip_plan.h", "zada_legacy_plan.h"))
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.zp_method_name.restype = ctypes.c_char_p
    L.zp_why_text.restype = ctypes.c_char_p
    L.zp_check.argtypes = [vp, i32, u64, u64, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.zp_bound.restype = u64
    L.zp_bound.argtypes = [i32, vp, u64]
    L.zp_groups.argtypes = [vp, i32, i32, u64, vp, vp, i32]
    L.zp_headers.restype = u64
    L.zp_headers.argtypes = [vp, i32, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp]
    L.zp_archive.restype = u64
    L.zp_archive.argtypes = [vp, i32, i32, u64, u64, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp]
    return L


def name_of(i, n):
    """Byte j of entry i's name is 'a' + (7 * i + j) % 26, as the stand-alone program makes it."""
    return ((np.arange(n, dtype=np.uint32) + 7 * i) % 26 + 97).astype(np.uint8).tobytes()


def table(rows):
    """rows: (d_data, n, name_len, time, flags).  -> (the table, what keeps the names alive)"""
    t = np.zeros(len(rows), dtype=DT)
    names = [np.frombuffer(name_of(i, r[2] if r[2] <= 65535 else 0) + b"\0", dtype=np.uint8) for i, r in enumerate(rows)]
    for i, r in enumerate(rows):
        t[i] = (r[0], r[1], names[i].ctypes.data, r[2], r[3], r[4], 0)
    return t, names


# ---- ZipCreate on sizes no buffer holds: the payloads are lengths, the buffer keeps the headers ----
class Payload:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __radd__(self, head):
        return (bytes(head), self.n)


class HeaderBuf:
    """What ZipCreate appends to, without the payloads' bytes: .chunks holds the header of every entry, .tail what finish adds."""

    def __init__(self):
        self.size, self.chunks, self.tail = 0, [], bytearray()

    def __len__(self):
        return self.size

    def __iadd__(self, x):
        if isinstance(x, tuple):
            self.chunks.append(x[0])
            self.size += len(x[0]) + x[1]
        else:
            self.tail += x
            self.size += len(x)
        return self

    def __bytes__(self):
        return bytes(self.tail)


def py_archive(entries, base):
    """entries: (name bytes, crc, csize, usize, zip_type, time, unicode).  -> (local headers, offsets, tail, archive length) by ZipCreate."""
    zc = product().ZipCreate(None, 0, _offset_bias=base)
    zc.buf = HeaderBuf()
    for nm, crc, csize, usize, zt, tm, uni in entries:
        zc.add_compressed(nm.decode("ascii"), Payload(csize), crc, usize, zt, tm, bool(uni))
    tail = zc.finish()
    return zc.buf.chunks, [e["offset"] for e in zc.entries], tail, len(zc.buf)


def py_groups(ns, method, limit):
    out, g0, b = [], 0, 0

    def flush(g1):
        nonlocal g0, b
        if g1 > g0:
            out.append((g1, G_STORE if method == 0 else G_SINGLE if g1 - g0 == 1 else G_BATCH))
        g0, b = g1, 0
    for i, n in enumerate(ns):
        if method == 0:
            p = (n + 16383) // 16384 + 1
            if b + p > 1 << 22:
                flush(i)
            b += p
        elif n > MIB4:
            flush(i)
            flush(i + 1)
        else:
            slot = (max(n, 1) + 32767) & ~32767
            if b + slot > limit:
                flush(i)
            b += slot
    flush(len(ns))
    return out


def py_check(rows, d_archive, cap):
    for i, (a, n, nl, _, _) in enumerate(rows):
        w = 0
        if n and not a:
            w = W_NULL
        elif nl > 65535:
            w = W_NAME
        elif n >= TIB:
            w = W_TOO_LARGE
        elif n and cap and a < d_archive + cap and d_archive < a + n:
            w = W_OVERLAP
        if w:
            return (E_TOO_LARGE if w == W_TOO_LARGE else E_INVALID), i, w
    return 0, -1, 0


SIZES = (0, 0, 1, 2, 100, 4095, 32768, 32769, MIB4, MIB4 + 1, 0xFFFFFFFE, 0xFFFFFFFF, 0x100000000, 2 ** 32 - MARGIN - 1, 2 ** 32 - MARGIN)
BASES = (0, 0, 0, 0, 7, 2 ** 32 - MARGIN - 40, 2 ** 32 - MARGIN - 1, 2 ** 32 - MARGIN, 2 ** 32 - MARGIN + 1, 0xFFFFFFFF - 31, 0xFFFFFFFE, 0xFFFFFFFF, 0x100000000,
         2 ** 32 - 100)
ARCHIVE_AT, ARCHIVE_CAP = 1 << 50, 1 << 43               # (where the lists' pretended archive buffer lies; the inputs lie below it)


def random_lists(count=2000, seed=23):
    """(rows, method, base, limit, verdicts): rows of (d_data, n, name_len, time, flags), verdicts of (bytes, wbase, reg) per entry.  The lists the
    issue names are among them: no entries; 65 534, 65 535 and 65 536 entries; empty names and names of 65 535 bytes; every size and base of
    SIZES / BASES."""
    rng = np.random.default_rng(seed)
    pick = lambda values: values[int(rng.integers(0, len(values)))]
    out = []
    for t in range(count):
        ne = 0 if t == 0 else (65534, 65535, 65536)[t - 1] if t <= 3 else int(rng.integers(0, 12))
        big = t <= 3
        if t in (4, 5):
            ne = max(ne, 2)
        rows, ver = [], []
        for i in range(ne):
            n = 0 if big and i % 5 else pick(SIZES) if rng.integers(0, 3) == 0 else int(rng.integers(0, 70000))
            nl = i % 3 if big else 65535 if (t in (4, 5) and i == 1) else pick((0, 1, 8, 30, int(rng.integers(0, 300))))
            a = (1 << 30) + (i << 41 if n >= 1 << 32 else i << 33) + int(rng.integers(0, 16)) if n else pick((0, 5))
            rows.append((a, n, nl, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 4))))
            by = int(rng.integers(0, max(1, n))) if rng.integers(0, 3) else n + int(rng.integers(0, 9))
            ver.append((by, int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1 << 32))))
        base = 0 if big and t != 2 else pick(BASES)
        if not rows:
            base = min(base, 0xFFFFFFFF)          # (Finish promotes an archive to Zip64 only when it has entries: an empty one further back has no end record)
        out.append((rows, pick((0, 6, 8, 10, 11)), base, pick((1 << 15, 1 << 20, 512 << 20)), ver))
    return out


def c_headers(L, rows, base, crc, csize, zt):
    t, keep = table(rows)
    n = len(rows)
    crc, csize, zt = np.array(crc, np.uint32), np.array(csize, np.uint64), np.array(zt, np.uint16)
    lcap = sum(50 + min(r[2], 65535) for r in rows) + 1
    tcap = sum(74 + min(r[2], 65535) for r in rows) + 98
    locals_, tail = np.zeros(lcap, np.uint8), np.zeros(tcap, np.uint8)
    at, off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    ln, tn = ctypes.c_uint64(0), ctypes.c_uint64(0)
    alen = L.zp_headers(t.ctypes.data, n, base, crc.ctypes.data, csize.ctypes.data, zt.ctypes.data, locals_.ctypes.data, lcap, ctypes.byref(ln), at.ctypes.data, off.ctypes.data,
                        tail.ctypes.data, tcap, ctypes.byref(tn))
    assert ln.value <= lcap and tn.value <= tcap
    lb = locals_.tobytes()
    return [lb[int(at[i]):int(at[i + 1])] for i in range(n)], [int(x) for x in off[:n]], tail[:tn.value].tobytes(), alen, int(L.zp_bound(n, t.ctypes.data, base))


def c_archive(L, rows, method, base, limit, ver):
    t, keep = table(rows)
    n = len(rows)
    by, wb, rg = np.array([v[0] for v in ver], np.uint64), np.array([v[1] for v in ver], np.uint32), np.array([v[2] for v in ver], np.uint32)
    lcap = sum(50 + r[2] for r in rows) + 1
    tcap = sum(74 + r[2] for r in rows) + 98
    locals_, tail = np.zeros(lcap, np.uint8), np.zeros(tcap, np.uint8)
    jobs = np.zeros((2 * n + 1, 5), np.uint64)
    res = np.zeros(n + 1, DT_RES)
    nj, ln, tn = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    alen = L.zp_archive(t.ctypes.data, n, method, base, limit, by.ctypes.data, wb.ctypes.data, rg.ctypes.data, jobs.ctypes.data, 2 * n, ctypes.byref(nj), res.ctypes.data,
                        locals_.ctypes.data, lcap, ctypes.byref(ln), tail.ctypes.data, tcap, ctypes.byref(tn))
    assert nj.value <= 2 * n and ln.value <= lcap and tn.value <= tcap
    return alen, [tuple(int(x) for x in j) for j in jobs[:nj.value]], res[:n], locals_[:ln.value].tobytes(), tail[:tn.value].tobytes()


def c_groups(L, rows, method, limit):
    t, keep = table(rows)
    g1, kind = np.zeros(len(rows) + 1, np.int32), np.zeros(len(rows) + 1, np.int32)
    k = L.zp_groups(t.ctypes.data, len(rows), method, limit, g1.ctypes.data, kind.ctypes.data, len(rows) + 1)
    return [(int(a), int(b)) for a, b in zip(g1[:k], kind[:k])]


def verdict_entries(rows, method, ver):
    """What the plan must make of the verdicts: Compress_Data's fallback, the final CRC."""
    out = []
    for i, ((a, n, nl, tm, fl), (by, wb, rg)) in enumerate(zip(rows, ver)):
        stored = method == 0 or by >= n
        out.append((name_of(i, nl), rg ^ 0xFFFFFFFF, n if stored else by, n, 0 if stored else 8, tm, fl & 1))
    return out


def test_headers_equal_zipcreate_on_random_lists(plan):
    """add_compressed + finish from given (name, crc, csize, usize, zip_type, time, unicode): every local header, the directory and the end records, the
    offsets, the archive's length; and the bound."""
    rng = np.random.default_rng(5)
    seen64, seen_plain, counts = 0, 0, set()
    for rows, method, base, limit, ver in random_lists():
        rows = [r for r in rows if r[2] <= 65535]
        ents = []
        for i, (a, n, nl, tm, fl) in enumerate(rows):
            zt = int(rng.integers(0, 2)) * 8
            ents.append((name_of(i, nl), int(rng.integers(0, 1 << 32)), n if zt == 0 else int(rng.integers(0, n + 1)), n, zt, tm, fl & 1))
        want = py_archive(ents, base)
        got = c_headers(plan, rows, base, [e[1] for e in ents], [e[2] for e in ents], [e[4] for e in ents])
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3], (base, rows[:4])
        assert got[4] >= want[3], (got[4], want[3], base)
        seen64 += b"PK\x06\x06" in want[2]
        seen_plain += b"PK\x06\x06" not in want[2]
        counts.add(len(rows))
    assert seen64 > 100 and seen_plain > 100 and {0, 65534, 65535, 65536} <= counts


def test_plan_from_verdicts_on_random_lists(plan):
    """The plan as zada_zip_device walks it: groups, Store fallbacks, results, headers; the copy jobs tile [0, archive_len) exactly once, minus the
    directory."""
    kinds = set()
    for rows, method, base, limit, ver in random_lists():
        if any(r[2] > 65535 for r in rows):
            continue
        groups = c_groups(plan, rows, method, limit)
        assert groups == py_groups([r[1] for r in rows], method, limit)
        ents = verdict_entries(rows, method, ver)
        want = py_archive(ents, base)
        alen, jobs, res, locals_, tail = c_archive(plan, rows, method, base, limit, ver)
        assert alen == want[3] and tail == want[2] and locals_ == b"".join(want[0])
        assert [int(x) for x in res["offset"]] == want[1]
        assert [(int(r["rc"]), int(r["zip_type"]), int(r["crc"]), int(r["csize"])) for r in res] == [(0, e[4], e[1], e[2]) for e in ents]
        t, keep = table(rows)
        assert plan.zp_bound(len(rows), t.ctypes.data, base) >= alen
        # the jobs: in archive order, one behind the other from 0 to where the directory begins; the headers one behind the other in the blob
        pos = blob = 0
        single = {g1 - 1 for g1, kind in groups if kind == G_SINGLE}
        for kind, entry, src, dst, ln in jobs:
            assert dst == pos and ln > 0
            pos += ln
            kinds.add(kind)
            if kind == K_BLOB:
                assert src == blob and ln == len(want[0][entry]) and dst == want[1][entry] - base
                blob += ln
            else:
                assert ln == ents[entry][2] and dst == want[1][entry] - base + len(want[0][entry])
                assert kind == (K_DATA if ents[entry][4] == 0 else K_STREAM)
                assert src == (ver[entry][1] if kind == K_STREAM and entry not in single else 0)
        assert pos == alen - len(tail) and blob == len(locals_)
        assert sorted({j[1] for j in jobs if j[0] == K_BLOB}) == list(range(len(rows)))
    assert kinds == {K_BLOB, K_STREAM, K_DATA}


def test_group_cuts(plan):
    row = lambda n: (1 << 30, n, 1, 0, 0)
    small = [row(16384)] * 100
    for m in (6, 8, 11):
        assert c_groups(plan, small, m, 1 << 20) == [(32, G_BATCH), (64, G_BATCH), (96, G_BATCH), (100, G_BATCH)]        # 32 slots of 32 KiB per MiB
        assert c_groups(plan, small, m, 512 << 20) == [(100, G_BATCH)]
        assert c_groups(plan, small[:33], m, 1 << 20) == [(32, G_BATCH), (33, G_SINGLE)]
        assert c_groups(plan, [row(32768)] * 3 + [row(32769)] * 2, m, 131072) == [(3, G_BATCH), (5, G_BATCH)]        # 3 x 32 KiB + 64 KiB is over, 2 x 64 KiB fits
        # around an entry of 4 MiB + 1: it ends the group before it and runs alone; 4 MiB itself is a small entry
        assert c_groups(plan, [row(5), row(7), row(MIB4 + 1), row(9), row(11)], m, 512 << 20) == [(2, G_BATCH), (3, G_SINGLE), (5, G_BATCH)]
        assert c_groups(plan, [row(5), row(MIB4 + 1), row(9)], m, 512 << 20) == [(1, G_SINGLE), (2, G_SINGLE), (3, G_SINGLE)]
        assert c_groups(plan, [row(5), row(MIB4), row(9)], m, 512 << 20) == [(3, G_BATCH)]
        assert c_groups(plan, [row(MIB4 + 1)] * 2, m, 512 << 20) == [(1, G_SINGLE), (2, G_SINGLE)]
        assert c_groups(plan, [row(0)], m, 512 << 20) == [(1, G_SINGLE)]
        assert c_groups(plan, [row(MIB4)] * 3, m, 1 << 20) == [(1, G_SINGLE), (2, G_SINGLE), (3, G_SINGLE)]       # an entry beyond the bound: alone
    assert c_groups(plan, small + [row(1 << 36)], 0, 1 << 20) == [(100, G_STORE), (101, G_STORE)]              # Store: by pieces, whatever batch_mib says
    assert c_groups(plan, [row(0)] * 65535, 0, 1 << 20) == [(65535, G_STORE)]
    assert c_groups(plan, [], 8, 1 << 20) == []


def test_every_refusal_with_its_index(plan):
    def check(rows, d_archive=ARCHIVE_AT, cap=ARCHIVE_CAP):
        t, keep = table(rows)
        bad, why = ctypes.c_int(99), ctypes.c_int(99)
        rc = plan.zp_check(t.ctypes.data if len(t) else None, len(t), d_archive, cap, ctypes.byref(bad), ctypes.byref(why))
        assert (rc, bad.value, why.value) == py_check(rows, d_archive, cap)
        return rc, bad.value, why.value
    ok = [(4096, 100, 3, 0, 1), (16384, 0, 0, 0, 0), (8192, 5, 65535, 0, 0)]
    assert check(ok) == (0, -1, 0) and check([]) == (0, -1, 0)
    for i in range(3):
        for change, want in ((dict(a=0, n=1), (E_INVALID, W_NULL)), (dict(nl=65536), (E_INVALID, W_NAME)), (dict(nl=0xFFFFFFFF), (E_INVALID, W_NAME)),
                             (dict(n=TIB), (E_TOO_LARGE, W_TOO_LARGE)), (dict(n=TIB - 1), (0, 0)), (dict(a=5000, n=(1 << 63) + 5), (E_TOO_LARGE, W_TOO_LARGE))):
            rows = [list(r) for r in ok]
            for k, v in change.items():
                rows[i][{"a": 0, "n": 1, "nl": 2}[k]] = v
            rc, bad, why = check([tuple(r) for r in rows])
            assert (rc, why) == want and bad == (i if rc else -1), (i, change)
    # overlap with [d_archive, d_archive + cap): every way of touching it, and ranges that only touch
    for a, n, hit in ((1000, 24, False), (1000, 25, True), (1023, 1, False), (1024, 1, True), (2047, 1, True), (2048, 1, False), (16, 4096, True), (1500, 0, False),
                      (1100, 10, True)):
        rc, bad, why = check([ok[0], (a, n, 1, 0, 0)], 1024, 1024)
        assert (rc, bad, why) == ((E_INVALID, 1, W_OVERLAP) if hit else (0, -1, 0)), (a, n)
    assert check([(1024, 10, 1, 0, 0)], 1024, 0) == (0, -1, 0)                    # an empty buffer overlaps nothing (and takes no archive)
    # the first bad entry is the one named
    assert check([ok[0], (0, 1, 0, 0, 0), (0, 1, 70000, 0, 0)]) == (E_INVALID, 1, W_NULL)
    for why in (W_NULL, W_NAME, W_TOO_LARGE, W_OVERLAP):
        assert plan.zp_why_text(why)
    # methods: Store and the six Deflate methods; every other one has a name for the refusal
    assert [m for m in range(-1, 40) if plan.zp_method_ok(m)] == [0, 6, 7, 8, 9, 10, 11]
    za = product()
    names = {v: k for k, v in vars(za.Method).items() if isinstance(v, int)}
    assert len(names) == 36
    for m, nm in names.items():
        assert plan.zp_method_name(m).decode() == nm
    assert plan.zp_method_name(36) == plan.zp_method_name(-1) == b"unknown"


def test_the_same_lists_under_the_sanitizers(tmp_path):
    """A program of its own (its own main, -fsanitize=address,undefined), run as a child process on the lists of the tests above -- those with a name
    that is refused too: it ends clean and prints what ZipCreate and the restatement give."""
    exe = str(tmp_path / "zip_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DZIP_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe, SRC], check=True)
    lines, want = [], []
    lists = random_lists()
    lists.append(([(4096, 5, 65536, 1, 1), (4096, 5, 3, 1, 1)], 8, 0, 1 << 20, [(1, 0, 0), (1, 0, 0)]))        # a refused name
    lists.append(([(ARCHIVE_AT + 5, 5, 3, 1, 1)], 8, 0, 1 << 20, [(1, 0, 0)]))                               # an overlap
    for rows, method, base, limit, ver in lists:
        lines.append("%d %d %d %d %d %d" % (len(rows), method, base, limit, ARCHIVE_AT, ARCHIVE_CAP))
        lines += ["%d %d %d %d %d %d %d %d" % (r + v) for r, v in zip(rows, ver)]
        rc, bad, why = py_check(rows, ARCHIVE_AT, ARCHIVE_CAP)
        z = lambda n, off: n >= 0xFFFFFFFF or off >= 0xFFFFFFFF
        local = central = 0
        for a, n, nl, _, _ in rows:
            z64 = z(n, base + local)
            local += 30 + nl + 20 * z64 + n
            central += 46 + nl + 28 * z64
        line = "%d %d %d | %d | groups:%s" % (rc, bad, why, (local + central + 98) & M64, "".join(" %d/%d" % g for g in py_groups([r[1] for r in rows], method, limit)))
        if rc == 0:
            ents = verdict_entries(rows, method, ver)
            heads, offs, tail, alen = py_archive(ents, base)
            b = np.frombuffer(b"".join(heads) + tail, dtype=np.uint8).astype(np.uint64)
            wsum = int((b * np.arange(1, len(b) + 1, dtype=np.uint64)).sum(dtype=np.uint64)) if len(b) else 0
            single = {g1 - 1 for g1, kind in py_groups([r[1] for r in rows], method, limit) if kind == G_SINGLE}
            nj = s = blob = 0
            for i, e in enumerate(ents):
                dst = offs[i] - base
                s += K_BLOB + 3 * i + 5 * blob + 7 * dst + 11 * len(heads[i])
                blob += len(heads[i])
                nj += 1
                if e[2]:
                    kind = K_DATA if e[4] == 0 else K_STREAM
                    s += kind + 3 * i + 5 * (ver[i][1] if kind == K_STREAM and i not in single else 0) + 7 * (dst + len(heads[i])) + 11 * e[2]
                    nj += 1
            line += " | %d | %d | jobs: %d %d" % (alen, wsum, nj, s & M64)
        want.append(line)
    src = tmp_path / "lists.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    got = r.stdout.splitlines()
    assert got[-1] == "plan ok" and len(got) == len(want) + 1
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
