"""The host plan of zada_unzip_device (zip-ada_amd/csrc/zada_unzip_plan.h: argument checks, overlap test, piece table, groups) through
tests/unzip/unzip_plan_host.cpp, against a restatement in Python; the same lists once more through a program of its own built with
-fsanitize=address,undefined.  No GPU, and nothing is loaded into this interpreter with a sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _common import ROOT, plan_library

E_INVALID, E_TOO_LARGE = -1, -4
W_METHOD, W_TOO_LARGE, W_IN, W_OUT, W_KEYS, W_OVERLAP = 1, 2, 3, 4, 5, 6
TIB = 1 << 40
DT = np.dtype([("in_off", "<u8"), ("n_in", "<u8"), ("out_off", "<u8"), ("cap", "<u8"), ("method", "<u2"), ("flags", "u1"), ("check", "u1"), ("pad", "<u4")])
SRC = os.path.join(ROOT, "tests", "unzip", "unzip_plan_host.cpp")


@pytest.fixture(scope="module")
def plan():
    L = ctypes.CDLL(plan_library("unzip", "unzip_plan_host", "zada_unzip_plan.h"))
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.up_check.argtypes = [vp, i32, u64, u64, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.up_payload.restype = u64
    L.up_payload.argtypes = [vp]
    L.up_pieces.restype = u64
    L.up_pieces.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, u64, vp]
    L.up_groups.argtypes = [vp, i32, u64, vp, i32]
    return L


def table(rows):
    t = np.zeros(len(rows), dtype=DT)
    for i, r in enumerate(rows):
        t[i] = tuple(r) + (0, 0)
    return t


# ---- the restatement ----
def py_payload(r):
    return (r[1] - 12 if r[1] >= 12 else 0) if r[5] & 1 else r[1]


def py_check(rows, archive_len, out_bytes, have_out, have_keys):
    for i, (in_off, n_in, out_off, cap, method, flags) in enumerate(rows):
        w = 0
        if method not in (0, 8, 9, 12, 14):
            w = W_METHOD
        elif n_in >= TIB or cap >= TIB:
            w = W_TOO_LARGE
        elif in_off + n_in > archive_len:
            w = W_IN
        elif have_out and out_off + cap > out_bytes:
            w = W_OUT
        elif flags & 1 and not have_keys:
            w = W_KEYS
        if w:
            return (E_TOO_LARGE if w == W_TOO_LARGE else E_INVALID), i, w
    if have_out:
        end = 0
        for out_off, i in sorted((r[2], i) for i, r in enumerate(rows) if r[3]):
            if out_off < end:
                return E_INVALID, i, W_OVERLAP
            end = out_off + rows[i][3]
    return 0, -1, 0


def py_pieces(lens, plog):
    P, out, first = 1 << plog, [], []
    for k, ln in enumerate(lens):
        first.append(len(out))
        out += [(o, k, min(P, ln - o)) for o in range(0, ln, P)]
    return out, first + [len(out)]


def py_groups(rows, limit):
    ends, g0 = [], 0
    while g0 < len(rows):
        g1, b = g0, 0
        while g1 < len(rows) and (g1 == g0 or b + ((rows[g1][3] + 255) & ~255) <= limit):
            b += (rows[g1][3] + 255) & ~255
            g1 += 1
        ends.append(g1)
        g0 = g1
    return ends


# ---- the library's answers ----
def c_check(L, rows, archive_len, out_bytes, have_out, have_keys):
    t = table(rows)
    bad, why = ctypes.c_int(99), ctypes.c_int(99)
    rc = L.up_check(t.ctypes.data if len(t) else None, len(t), archive_len, out_bytes, have_out, have_keys, ctypes.byref(bad), ctypes.byref(why))
    return rc, bad.value, why.value


def c_pieces(L, lens, plog):
    a = np.array(lens, dtype=np.uint64)
    first = np.zeros(len(lens) + 1, np.uint64)
    cap = sum((x + (1 << plog) - 1) >> plog for x in lens)
    off, ent, ln = np.zeros(cap + 1, np.uint64), np.zeros(cap + 1, np.uint32), np.zeros(cap + 1, np.uint32)
    n = L.up_pieces(a.ctypes.data, len(lens), plog, off.ctypes.data, ent.ctypes.data, ln.ctypes.data, cap, first.ctypes.data)
    assert n == cap
    return [(int(o), int(e), int(x)) for o, e, x in zip(off[:n], ent[:n], ln[:n])], [int(x) for x in first]


def c_groups(L, rows, limit):
    t = table(rows)
    ends = np.zeros(len(rows) + 1, np.int32)
    n = L.up_groups(t.ctypes.data if len(t) else None, len(t), limit, ends.ctypes.data, len(ends))
    return [int(x) for x in ends[:n]]


def random_lists(count=2000, seed=20):
    """(rows, archive_len, out_bytes, have_out, have_keys, limit, plog): mostly valid disjoint layouts, with every kind of mistake mixed in."""
    rng = np.random.default_rng(seed)
    pick = lambda values: values[int(rng.integers(0, len(values)))]          # (not rng.choice: it would make floats of the values near 2 ** 64)
    out = []
    for t in range(count):
        n = int(rng.integers(0, 40))
        archive_len = int(rng.integers(0, 1 << 22))
        rows, o = [], int(rng.integers(0, 64))
        for _ in range(n):
            n_in = int(rng.integers(0, 70000)) if archive_len else 0
            in_off = int(rng.integers(0, max(1, archive_len - min(n_in, archive_len) + 1)))
            n_in = min(n_in, archive_len - in_off)
            cap = int(rng.choice([0, 1, 255, 256, 257, int(rng.integers(0, 100000))]))
            rows.append([in_off, n_in, o, cap, int(rng.choice([0, 0, 8, 9, 12, 14])), int(rng.integers(0, 4))])
            o += cap + int(rng.choice([0, 0, 16, 256, 5]))
        out_bytes = o + int(rng.integers(0, 3))
        kind = int(rng.integers(0, 12)) if n else 0
        k = int(rng.integers(0, n)) if n else 0
        if kind == 1:
            rows[k][4] = int(rng.choice([1, 6, 10, 13, 99, 65535]))
        elif kind == 2:
            rows[k][int(rng.choice([1, 3]))] = TIB + int(rng.integers(0, 5)) * (1 << 50)
        elif kind == 3:
            rows[k][0] = pick([archive_len + 1, (1 << 64) - 1, archive_len - rows[k][1] + 1])
        elif kind == 4:
            rows[k][2] = pick([out_bytes + 1, (1 << 64) - 8, out_bytes - rows[k][3] + 1])
        elif kind == 5 and n >= 2:                            # an overlap, or an empty range inside another: only the first counts
            j = (k + 1) % n
            if rows[j][3]:
                rows[k][2] = rows[j][2] + int(rng.integers(0, rows[j][3]))
                rows[k][3] = int(rng.choice([0, 1, rows[k][3]]))
        have_keys = int(rng.integers(0, 4) != 0)
        out.append((rows, archive_len, out_bytes, int(rng.integers(0, 5) != 0), have_keys, int(rng.choice([1, 4096, 1 << 16, 1 << 20])), int(rng.choice([8, 11, 14]))))
    return out


def test_check_groups_and_pieces_equal_the_restatement(plan):
    kinds = set()
    for rows, alen, obytes, have_out, have_keys, limit, plog in random_lists():
        want = py_check(rows, alen, obytes, have_out, have_keys)
        assert c_check(plan, rows, alen, obytes, have_out, have_keys) == want, rows
        kinds.add(want[2])
        ends = c_groups(plan, rows, limit)
        assert ends == py_groups(rows, limit)
        g0 = 0
        for g1 in ends:                                       # no group over its bound, unless it holds a single entry
            assert g1 > g0 and (g1 - g0 == 1 or sum((r[3] + 255) & ~255 for r in rows[g0:g1]) <= limit)
            g0 = g1
        assert g0 == len(rows)
        lens = [py_payload(r) & 0xFFFFF for r in rows if r[4] == 0]
        assert c_pieces(plan, lens, plog) == py_pieces(lens, plog)
        t = table(rows)
        for i, r in enumerate(rows):
            assert plan.up_payload(t[i:i + 1].ctypes.data) == py_payload(r)
    assert kinds == {0, W_METHOD, W_TOO_LARGE, W_IN, W_OUT, W_KEYS, W_OVERLAP}


def test_overlap(plan):
    base = [[0, 10, 100, 50, 8, 0], [10, 10, 150, 50, 0, 0], [20, 10, 0, 100, 12, 0], [30, 10, 200, 1, 14, 0]]
    assert c_check(plan, base, 40, 201, 1, 0) == (0, -1, 0)                   # ranges that only touch
    for k, (off, cap, bad) in enumerate(((149, 50, 1), (99, 2, 0), (100, 1, 0), (199, 2, 3), (0, 201, 0), (200, 1, 3))):
        rows = [list(r) for r in base] + [[0, 0, off, cap, 0, 0]]
        rc, i, why = c_check(plan, rows, 40, 201, 1, 0)
        assert (rc, why) == (E_INVALID, W_OVERLAP) and i in (bad, 4), (k, i)
        assert (rc, i, why) == py_check(rows, 40, 201, 1, 0)
        assert c_check(plan, rows, 40, 201, 0, 0) == (0, -1, 0)               # the test-only form has no output ranges
        rows[4][3] = 0                                                       # an empty range inside another's does not count
        assert c_check(plan, rows, 40, 201, 1, 0) == (0, -1, 0)
    same = [[0, 1, 64, 16, 0, 0], [0, 1, 64, 16, 0, 0]]
    assert c_check(plan, same, 1, 80, 1, 0) == (E_INVALID, 1, W_OVERLAP)


def test_every_range_is_refused_with_its_index(plan):
    ok = [[5, 10, 0, 16, 8, 0], [15, 12, 16, 16, 0, 1], [27, 3, 32, 8, 14, 2]]
    assert c_check(plan, ok, 30, 40, 1, 1) == (0, -1, 0)
    assert c_check(plan, ok, 30, 40, 1, 0) == (E_INVALID, 1, W_KEYS)
    assert c_check(plan, ok, 29, 40, 1, 1) == (E_INVALID, 2, W_IN)
    assert c_check(plan, ok, 30, 39, 1, 1) == (E_INVALID, 2, W_OUT)
    assert c_check(plan, ok, 30, 0, 0, 1) == (0, -1, 0)
    for i in range(3):
        for col, why in ((0, W_IN), (1, W_IN), (2, W_OUT), (3, W_OUT)):
            for v in (1 << 63, (1 << 64) - 1, 31 if col < 2 else 41):
                rows = [list(r) for r in ok]
                rows[i][col] = v
                rc, bad, w = c_check(plan, rows, 30, 40, 1, 1)
                assert bad == i and (rc, w) == ((E_TOO_LARGE, W_TOO_LARGE) if col in (1, 3) and v >= TIB else (E_INVALID, why)), (i, col, v)
        rows = [list(r) for r in ok]
        rows[i][4] = 7
        assert c_check(plan, rows, 30, 40, 1, 1) == (E_INVALID, i, W_METHOD)
    assert c_check(plan, [], 0, 0, 1, 0) == (0, -1, 0)


@pytest.mark.parametrize("plog", (8, 14))
def test_piece_tables(plan, plog):
    lens = [0, 1]
    for k in range(plog - 1, plog + 8):
        lens += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    got, first = c_pieces(plan, lens, plog)
    assert (got, first) == py_pieces(lens, plog)
    P = 1 << plog
    for k, ln in enumerate(lens):
        mine = got[first[k]:first[k + 1]]
        assert len(mine) == (ln + P - 1) // P and sum(x[2] for x in mine) == ln
        assert all(e == k and o == j * P and 1 <= x <= P for j, (o, e, x) in enumerate(mine))
        assert all(x == P for _, _, x in mine[:-1])


def test_the_same_lists_under_the_sanitizers(tmp_path):
    """A program of its own (its own main, -fsanitize=address,undefined), run as a child process on the lists of the first test: it ends clean and
    prints what the restatement gives."""
    exe = str(tmp_path / "unzip_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DUNZIP_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe, SRC], check=True)
    lines, want = [], []
    for rows, alen, obytes, have_out, have_keys, limit, plog in random_lists():
        lines.append("%d %d %d %d %d %d %d" % (len(rows), alen, obytes, have_out, have_keys, limit, plog))
        lines += ["%d %d %d %d %d %d" % tuple(r) for r in rows]
        pieces, _ = py_pieces([py_payload(r) & 0xFFFFF for r in rows if r[4] == 0], plog)
        ids = [i for i, r in enumerate(rows) if r[4] == 0]
        s = sum(o + 3 * ids[e] + 7 * x for o, e, x in pieces) & ((1 << 64) - 1)
        want.append("%d %d %d | groups:%s | pieces: %d %d" % (py_check(rows, alen, obytes, have_out, have_keys) + ("".join(" %d" % e for e in py_groups(rows, limit)), len(pieces), s)))
    src = tmp_path / "lists.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    got = r.stdout.splitlines()
    assert got[-1] == "plan ok" and got[:-1] == want
