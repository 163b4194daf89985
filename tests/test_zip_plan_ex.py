"""The host plan of zada_zip_device_ex (zip-ada_amd/csrc/zada_zip_plan.h: a method per entry, groups with several methods, the flag bits of zip type
14 and of an encrypted entry, the 12 bytes of an encryption header in csize, Zip64 on the provisional sizes) through tests/zip/zip_plan_ex_host.cpp,
against ZipCreate.add_compressed + finish -- Python only -- and a restatement of the groups in Python; the same lists once more through a program of
its own built with -fsanitize=address,undefined.  No GPU, and nothing is loaded into this interpreter with a sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _common import ROOT, plan_library, product

G_BATCH, G_SINGLE, G_STORE = 0, 1, 2
K_BLOB, K_STREAM, K_DATA = 0, 1, 2
MIB4, M64, M32 = 4 << 20, (1 << 64) - 1, 0xFFFFFFFF
DT = np.dtype([("d_data", "<u8"), ("n", "<u8"), ("name", "<u8"), ("name_len", "<u4"), ("time", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
DT_RES = np.dtype([("rc", "<i4"), ("zip_type", "<u2"), ("pad", "<u2"), ("crc", "<u4"), ("pad2", "<u4"), ("csize", "<u8"), ("offset", "<u8")])
SRC = os.path.join(ROOT, "tests", "zip", "zip_plan_ex_host.cpp")
MARGIN = 22 + 56 + 20 + 2 ** 16 + 10
SIZES = (0, 1, 79987, 79988, 319987, 719987, 719988, MIB4, MIB4 + 1, M32 - 12, M32 - 11, M32 - 1, M32, M32 + 1, (1 << 32) - MARGIN - 1, (1 << 32) - MARGIN, 1 << 33)
BASES = (0, 77, M32 - 1000, M32 - 30, M32, (1 << 32) - MARGIN - 100, 1 << 33)


@pytest.fixture(scope="module")
def plan():
    L = ctypes.CDLL(plan_library("zip", "zip_plan_ex_host", "zada_zip_plan.h", "zada_legacy_plan.h"))
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.zpx_one_block.restype = u64
    L.zpx_bound.restype = u64
    L.zpx_bound.argtypes = [i32, vp, u64, i32]
    L.zpx_check.argtypes = [vp, i32, u64, u64, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.zpx_why_text.restype = ctypes.c_char_p
    L.zpx_groups.argtypes = [vp, i32, vp, vp, u64, u64, u64, vp, i32]
    L.zpx_archive.restype = u64
    L.zpx_archive.argtypes = [vp, i32, i32, vp, vp, u64, u64, u64, u64, vp, vp, vp, vp, vp, vp, i32, vp, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp]
    return L


def name_of(i, n):
    """Byte j of entry i's name is 'a' + (7 * i + j) % 26, as the stand-alone program makes it."""
    return ((np.arange(n, dtype=np.uint32) + 7 * i) % 26 + 97).astype(np.uint8).tobytes()


def hdr_of(i):
    return bytes((3 * i + 5 * j) % 256 for j in range(12))


def zip_type(m):
    return 0 if m == 0 else 8 if m <= 11 else 12 if m <= 14 else 14


def one_block(m):
    return ({12: 100000, 13: 400000, 14: 900000}[m] - 16) * 4 // 5


LIT = {19: 6 << 20, 20: 6 << 20, 23: 384 << 10, 24: 6 << 20, 25: 384 << 10, 26: 6 << 20, 27: 6 << 20, 28: 384 << 10, 29: 24 << 10, 30: 384 << 10}      # zada_lzma_lit_table_bytes


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


def py_archive(entries, base, enc):
    """entries: (name bytes, crc, payload bytes, usize, zip_type, time, unicode).  -> (local headers, entries, tail, archive length) by ZipCreate."""
    zc = product().ZipCreate(None, 0, _offset_bias=base)
    zc.buf = HeaderBuf()
    for nm, crc, pay, usize, zt, tm, uni in entries:
        zc.add_compressed(nm.decode("ascii"), Payload(pay + (12 if enc else 0)), crc, usize, zt, tm, bool(uni), password=b"x" if enc else None)
    tail = zc.finish()
    return zc.buf.chunks, zc.entries, tail, len(zc.buf)


def py_groups(rows, store, limit, bz_limit, lit_limit):
    """The groups of zada_zip_device_ex, restated: (g1, kind) pairs."""
    out, g0, acc = [], 0, [0, 0, 0]

    def flush(g1):
        nonlocal g0, acc
        if g1 > g0:
            out.append((g1, G_STORE if store else G_SINGLE if g1 - g0 == 1 else G_BATCH))
        g0, acc = g1, [0, 0, 0]

    for i, r in enumerate(rows):
        n, m, lit = r[1], r[5], r[6]
        if store:
            p = (n + 16383) // 16384 + 1
            if acc[0] + p > 1 << 22:
                flush(i)
            acc[0] += p
            continue
        slot = ((n or 1) + 32767) & ~32767
        b = slot if 12 <= m <= 14 else 0
        if n > MIB4 or (b and n > one_block(m)):
            flush(i)
            flush(i + 1)
            continue
        if acc[0] + slot > limit or acc[1] + b > bz_limit or acc[2] + lit > lit_limit:
            flush(i)
        acc = [acc[0] + slot, acc[1] + b, acc[2] + lit]
    flush(len(rows))
    return out


def random_lists(count=700, seed=31):
    """(rows, store, enc, base, limits): rows of (d_data, n, name_len, time, flags, method, lit, src, bytes, reg).  The method of an entry is what
    Preselection_1 / _2 make of a random content hint and the size, or one single method for all; Zip64 sizes and bases are among them, and a list
    of 65 535 entries."""
    za = product()
    rng = np.random.default_rng(seed)
    pick = lambda values: values[int(rng.integers(0, len(values)))]
    out = []
    for t in range(count):
        ne = 0 if t == 0 else 65535 if t == 1 else int(rng.integers(0, 14))
        single = pick((0, 6, 10, 11, 12, 13, 14, 15, 17, 18, 22, 30, 34, 35, 34, 35))
        store = single == 0
        rows = []
        for i in range(ne):
            n = 0 if t == 1 and i % 5 else pick(SIZES) if rng.integers(0, 4) == 0 else int(rng.integers(0, 90000))
            m = za.preselect(single, int(rng.integers(0, 16)), n) if single >= 34 else single
            nl = i % 3 if t == 1 else pick((0, 1, 8, 30, int(rng.integers(0, 300))))
            a = (1 << 30) + (i << 41) + int(rng.integers(0, 16)) if n else 0
            by = int(rng.integers(0, max(1, n))) if rng.integers(0, 3) else n + int(rng.integers(0, 9))
            rows.append((a, n, nl, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 4)), m, LIT.get(m, 0), (1 << 50) + int(rng.integers(0, 1 << 40)), by, int(rng.integers(0, 1 << 32))))
        base = 0 if t == 1 else pick(BASES)
        if not rows:
            base = min(base, M32)
        enc = bool(rng.integers(0, 2))
        if enc:           # (an encrypted entry of 4 GiB - 11 .. 4 GiB - 1 bytes is refused by zw_check_ex, and add_compressed cannot pack it: the test of its own below)
            rows = [r[:1] + (M32 - 12,) + r[2:8] + (min(r[8], M32 - 12),) + r[9:] if M32 - 12 < r[1] < M32 else r for r in rows]
        out.append((rows, store, enc, base, (pick((1 << 15, 1 << 17, 1 << 30)), pick((1 << 15, 1 << 28)), pick((1 << 21, 8 << 20, 12 << 30)))))
    return out


def c_archive(L, rows, store, enc, base, limits):
    n = len(rows)
    t = np.zeros(n, dtype=DT)
    names = [np.frombuffer(name_of(i, r[2]) + b"\0", dtype=np.uint8) for i, r in enumerate(rows)]
    for i, r in enumerate(rows):
        t[i] = (r[0], r[1], names[i].ctypes.data, r[2], r[3], r[4], 0)
    col = lambda k, dt: np.array([r[k] for r in rows], dt)
    m, lit, src, by, rg = col(5, np.int32), col(6, np.uint64), col(7, np.uint64), col(8, np.uint64), col(9, np.uint32)
    zt = np.array([zip_type(r[5]) for r in rows], np.uint16)
    h12 = np.frombuffer(b"".join(hdr_of(i) for i in range(n)) + b"\0", dtype=np.uint8)
    lcap, tcap = sum(62 + r[2] for r in rows) + 1, sum(74 + r[2] for r in rows) + 98
    locals_, tail = np.zeros(lcap, np.uint8), np.zeros(tcap, np.uint8)
    jobs, groups, res = np.zeros((2 * n + 1, 5), np.uint64), np.zeros((n + 1, 2), np.int32), np.zeros(n + 1, DT_RES)
    ng, nj, ln, tn = ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    alen = L.zpx_archive(t.ctypes.data, n, int(store), m.ctypes.data, lit.ctypes.data, base, limits[0], limits[1], limits[2], src.ctypes.data, by.ctypes.data, rg.ctypes.data,
                         zt.ctypes.data, h12.ctypes.data if enc else None, groups.ctypes.data, n + 1, ctypes.byref(ng), jobs.ctypes.data, 2 * n, ctypes.byref(nj), res.ctypes.data,
                         locals_.ctypes.data, lcap, ctypes.byref(ln), tail.ctypes.data, tcap, ctypes.byref(tn))
    assert ng.value <= n + 1 and nj.value <= 2 * n and ln.value <= lcap and tn.value <= tcap
    return (alen, [tuple(int(x) for x in g) for g in groups[:ng.value]], [tuple(int(x) for x in j) for j in jobs[:nj.value]], res[:n], locals_[:ln.value].tobytes(),
            tail[:tn.value].tobytes(), int(L.zpx_bound(n, t.ctypes.data, base, int(enc))))


def test_plan_from_verdicts_on_random_lists(plan):
    """Groups, Store fallbacks, flag bits, the 12 bytes, results, headers and the bound against add_compressed + finish; the jobs tile [0, archive_len)
    exactly once, minus the directory."""
    assert [plan.zpx_method_ok(m) for m in (-1, 0, 1, 5, 6, 35, 36, 99)] == [0, 1, 0, 0, 1, 1, 0, 0]
    assert [plan.zpx_zip_type(m) for m in (0, 6, 11, 12, 14, 15, 33)] == [0, 8, 8, 12, 12, 14, 14] and [plan.zpx_one_block(m) for m in (12, 13, 14)] == [79987, 319987, 719987]
    seen = dict(z64=0, plain=0, enc=0, eos=0, multi=0, stored=0)
    for rows, store, enc, base, limits in random_lists():
        alen, groups, jobs, res, locals_, tail, bound = c_archive(plan, rows, store, enc, base, limits)
        assert groups == py_groups(rows, store, *limits)
        ents = []
        for i, r in enumerate(rows):
            n, m, by, rg = r[1], r[5], r[8], r[9]
            stored = m == 0 or by >= n
            ents.append((name_of(i, r[2]), rg ^ M32, n if stored else by, n, 0 if stored else zip_type(m), r[3], r[4] & 1))
        chunks, entries, want_tail, want_len = py_archive(ents, base, enc)
        assert alen == want_len and tail == want_tail and bound >= want_len, (base, rows[:3])
        assert locals_ == b"".join(c + (hdr_of(i) if enc else b"") for i, c in enumerate(chunks))
        for i, (e, r) in enumerate(zip(entries, res)):
            assert (int(r["rc"]), int(r["zip_type"]), int(r["crc"]), int(r["csize"]), int(r["offset"])) == (0, e["zip_type"], e["crc"], e["csize"], e["offset"])
            assert e["flag"] == (0x0800 if rows[i][4] & 1 else 0) | (2 if e["zip_type"] == 14 else 0) | (1 if enc else 0)
        # the jobs: a header (with its 12 bytes) and, unless empty, a payload per entry, one behind the other from 0 to the directory
        pos, at, k = 0, 0, 0
        for i, e in enumerate(ents):
            hl = len(chunks[i]) + (12 if enc else 0)
            assert jobs[k] == (K_BLOB, i, at, pos, hl)
            pos, at, k = pos + hl, at + hl, k + 1
            if e[2]:
                stored = e[4] == 0
                assert jobs[k] == (K_DATA if stored else K_STREAM, i, 0 if stored else rows[i][7], pos, e[2])
                pos, k = pos + e[2], k + 1
        assert k == len(jobs) and pos + len(tail) == alen
        seen["z64"] += b"PK\x06\x06" in tail
        seen["plain"] += b"PK\x06\x06" not in tail
        seen["enc"] += enc and bool(rows)
        seen["eos"] += any(e["zip_type"] == 14 for e in entries)
        seen["stored"] += any(e["zip_type"] == 0 and rows[i][5] != 0 for i, e in enumerate(entries))
        g0 = 0
        for g1, kind in groups:
            seen["multi"] += kind == G_BATCH and len({r[5] for r in rows[g0:g1]}) > 1
            g0 = g1
    assert min(seen.values()) > 20, seen


def test_group_cuts(plan):
    """The cuts one by one: a BZip2 entry of one block and one byte more; ZW_ENTRY_MAX and one byte more; the three limits."""
    def groups(rows, limits=(1 << 30, 1 << 28, 12 << 30)):
        return c_archive(plan, rows, False, False, 0, limits)[1]

    row = lambda n, m: (1 << 30, n, 3, 0, 0, m, LIT.get(m, 0), 1 << 50, 0, 0)
    assert groups([row(10, 10), row(79987, 12), row(10, 17)]) == [(3, G_BATCH)]
    assert groups([row(10, 10), row(79988, 12), row(10, 17)]) == [(1, G_SINGLE), (2, G_SINGLE), (3, G_SINGLE)]
    assert groups([row(10, 10), row(10, 10), row(79988, 10), row(MIB4, 17), row(MIB4 + 1, 17), row(1, 14), row(719987, 14)]) == [(4, G_BATCH), (5, G_SINGLE), (7, G_BATCH)]
    assert groups([row(32768, 10)] * 5, (1 << 16, 1 << 28, 12 << 30)) == [(2, G_BATCH), (4, G_BATCH), (5, G_SINGLE)]
    assert groups([row(32768, 10), row(32768, 14), row(1, 14), row(1, 10), row(1, 10)], (1 << 30, 1 << 15, 12 << 30)) == [(2, G_BATCH), (5, G_BATCH)]
    assert groups([row(1, 19)] * 5, (1 << 30, 1 << 28, 13 << 20)) == [(2, G_BATCH), (4, G_BATCH), (5, G_SINGLE)]
    assert groups([row(1, 0)] * 3) == [(3, G_BATCH)] and c_archive(plan, [row(1, 0)] * 3, True, False, 0, (0, 0, 0))[1] == [(3, G_STORE)]


def test_an_encrypted_entry_whose_size_does_not_fit_is_refused(plan):
    """With a password an entry of 4 GiB - 11 .. 4 GiB - 1 bytes is refused with its index (add_compressed cannot pack it either: struct.error); without
    one, and at 4 GiB - 12 and 4 GiB - 1 + 1, it is taken.  An earlier refusal of the old checks comes first, a later one does not."""
    def check(sizes, enc, null_at=None):
        t = np.zeros(len(sizes), dtype=DT)
        nm = np.frombuffer(b"abc\0", dtype=np.uint8)
        for i, n in enumerate(sizes):
            t[i] = (0 if i == null_at else (1 << 20) + (i << 41), n, nm.ctypes.data, 3, 0, 0, 0)
        bad, why = ctypes.c_int(0), ctypes.c_int(0)
        rc = plan.zpx_check(t.ctypes.data, len(sizes), 1 << 60, 1 << 20, int(enc), ctypes.byref(bad), ctypes.byref(why))
        return rc, bad.value, plan.zpx_why_text(why.value).decode()

    for n in (M32 - 11, M32 - 5, M32 - 1):
        rc, bad, text = check([10, n, 10], True)
        assert rc == -1 and bad == 1 and text.startswith("an encrypted entry of 4 GiB - 11 .. 4 GiB - 1 bytes")
        assert check([10, n, 10], False)[0] == 0
        with pytest.raises(Exception):
            py_archive([(b"abc", 0, n, n, 0, 0, 1)], 0, True)
    for n in (M32 - 12, M32, M32 + 1):
        assert check([10, n, 10], True)[0] == 0
        py_archive([(b"abc", 0, n, n, 0, 0, 1)], 0, True)
    assert check([10, 5, M32 - 5], True, null_at=1)[1:] == (1, "null d_data with n > 0")
    assert check([10, M32 - 5, 5], True, null_at=2)[1] == 1


def test_the_same_lists_under_the_sanitizers(plan, tmp_path):
    """A program of its own (its own main, -fsanitize=address,undefined), run as a child process on the lists of the test above: its lines against
    what the library loaded here says."""
    exe = str(tmp_path / "zip_plan_ex_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DZIP_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe, SRC], check=True)
    lists = [L for L in random_lists(count=300) if len(L[0]) < 1000]
    src = tmp_path / "lists.txt"
    want = []
    with open(src, "w") as f:
        for rows, store, enc, base, limits in lists:
            f.write("%d %d %d %d %d %d %d\n" % (len(rows), store, enc, base, limits[0], limits[1], limits[2]))
            for r in rows:
                f.write("%d %d %d %d %d %d %d %d %d %d %d\n" % (r + (zip_type(r[5]),)))
            alen, groups, jobs, res, locals_, tail, bound = c_archive(plan, rows, store, enc, base, limits)
            w = sum((k + 1) * b for k, b in enumerate(locals_ + tail)) & M64
            js = sum(j[0] + 3 * j[1] + 5 * j[2] + 7 * j[3] + 11 * j[4] for j in jobs) & M64
            rs = sum(int(r["zip_type"]) + 3 * int(r["crc"]) + 5 * int(r["csize"]) + 7 * int(r["offset"]) for r in res) & M64
            want.append("%d | groups:%s | %d | %d | jobs: %d %d | results: %d" % (bound, "".join(" %d/%d" % g for g in groups), alen, w, len(jobs), js, rs))
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.splitlines() == want + ["plan ok"]
