"""The host plan of zada_compzip_device (zip-ada_amd/csrc/zada_rezip_plan.h: Comp_Zip's verdict as a closed form, the argument checks, the groups
of pairs) through tests/rezip/rezip_plan_host.cpp, against the literal restatement of the Ada loop in tests/_rezip.py and a restatement of the
groups in Python; the same lists once more through a program of its own built with -fsanitize=address,undefined.  No GPU, and nothing is loaded
into this interpreter with a sanitizer."""
import ctypes
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import _rezip

DT = np.dtype([("in_off", "<u8"), ("n_in", "<u8"), ("out_off", "<u8"), ("cap", "<u8"), ("method", "<u2"), ("flags", "u1"), ("check", "u1"), ("pad", "<u4")])
E_INVALID, E_TOO_LARGE = -1, -4
TIB = 1 << 40
W_METHOD, W_TOO_LARGE, W_IN_RANGE, W_OUT_RANGE, W_NO_KEYS = 1, 2, 3, 4, 5


@pytest.fixture(scope="module")
def plan():
    return _rezip.load_plan()


def verdict(plan, la, lb, d):
    pos, cmpd = ctypes.c_uint64(99), ctypes.c_uint64(99)
    v = plan.rp_verdict(la, lb, d, ctypes.byref(pos), ctypes.byref(cmpd))
    return v, pos.value, cmpd.value


def first_diff(f1, f2):
    m = min(len(f1), len(f2))
    return next((i for i in range(m) if f1[i] != f2[i]), m)


def strings(max_len=3):
    for n in range(max_len + 1):
        for t in itertools.product(b"ab", repeat=n):
            yield bytes(t)


def test_verdict_against_the_literal_loop(plan):
    """Every pair of strings over two letters of lengths 0 .. 3: all length pairs, every position of a first difference, and differences behind
    the first one and behind the shorter string's end, which must not count."""
    seen = set()
    for f1 in strings():
        for f2 in strings():
            v, pos, nbytes = _rezip.compare_1_file(f1, f2)
            d = first_diff(f1, f2)
            got = verdict(plan, len(f1), len(f2), d)
            assert got[0] == v, (f1, f2)
            if v in (_rezip.DIFFERENT, _rezip.SHORTER):
                assert got[1] == pos, (f1, f2)
            if v == _rezip.OK:
                assert got[2] == nbytes == len(f1)
            assert got[2] == d                                 # the equal bytes in front of the verdict
            seen.add((len(f1), len(f2), d, v))
    assert {s[3] for s in seen} == {_rezip.OK, _rezip.DIFFERENT, _rezip.SHORTER, _rezip.LONGER}
    assert len({s[:2] for s in seen}) == 16


def test_verdict_at_large_lengths(plan):
    big = (1 << 40) - 1
    assert verdict(plan, big, big, big) == (_rezip.OK, 0, big)
    assert verdict(plan, big, big, big - 1) == (_rezip.DIFFERENT, big, big - 1)
    assert verdict(plan, big, big - 1, big - 1) == (_rezip.SHORTER, big, big - 1)
    assert verdict(plan, big - 1, big, big - 1) == (_rezip.LONGER, 0, big - 1)
    assert verdict(plan, 1 << 32, 1 << 32, 0) == (_rezip.DIFFERENT, 1, 0)


def rows(spec):
    t = np.zeros(len(spec), dtype=DT)
    for k, (in_off, n_in, cap, method, flags) in enumerate(spec):
        t[k] = (in_off, n_in, 0, cap, method, flags, 0, 0)
    return t


def check(plan, a, b, len_a, len_b, have_keys):
    ta, tb = rows(a), rows(b)
    bad, side, why = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    rc = plan.rp_check(ta.ctypes.data, tb.ctypes.data, len(a), len_a, len_b, have_keys, ctypes.byref(bad), ctypes.byref(side), ctypes.byref(why))
    return rc, bad.value, side.value, why.value


def py_check(a, b, len_a, len_b, have_keys):
    """uz_check's rules in its order, archive 1's rows first, then the present rows of archive 2"""
    for side, tab, alen in ((1, a, len_a), (2, b, len_b)):
        for i, (in_off, n_in, cap, method, flags) in enumerate(tab):
            if side == 2 and flags & _rezip.ABSENT:
                continue
            why = 0
            if method not in (0, 8, 9, 12, 14):
                why = W_METHOD
            elif n_in >= TIB or cap >= TIB:
                why = W_TOO_LARGE
            elif in_off > alen or n_in > alen - in_off:
                why = W_IN_RANGE
            elif flags & 1 and not have_keys:
                why = W_NO_KEYS
            if why:
                return (E_TOO_LARGE if why == W_TOO_LARGE else E_INVALID), i, side, why
    return 0, -1, 0, 0


GOOD = (10, 20, 100, 8, 0)


def test_every_argument_check_with_its_text_and_index(plan):
    ok = [GOOD, GOOD, GOOD]
    assert check(plan, ok, ok, 1000, 1000, 0) == (0, -1, 0, 0)
    cases = [
        ((10, 20, 100, 1, 0), W_METHOD, E_INVALID, b"unknown method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)"),
        ((10, TIB, 100, 8, 0), W_TOO_LARGE, E_TOO_LARGE, b"a stream or an output of 1 TiB or more"),
        ((10, 20, TIB, 8, 0), W_TOO_LARGE, E_TOO_LARGE, b"a stream or an output of 1 TiB or more"),
        ((990, 11, 100, 8, 0), W_IN_RANGE, E_INVALID, b"its data lie beyond the archive"),
        ((1001, 0, 100, 8, 0), W_IN_RANGE, E_INVALID, b"its data lie beyond the archive"),
        ((10, 20, 100, 8, 1), W_NO_KEYS, E_INVALID, b"encrypted, and no keys were given"),
    ]
    for row, why, rc, text in cases:
        for at in range(3):
            for side in (1, 2):
                a, b = list(ok), list(ok)
                (a if side == 1 else b)[at] = row
                assert check(plan, a, b, 1000, 1000, 0) == (rc, at, side, why) == py_check(a, b, 1000, 1000, 0)
                assert plan.rp_why_text(why) == text
    # archive 1's rows come first; each archive has its own length; keys lift the refusal; an absent row is not looked at
    bad = (990, 11, 100, 8, 0)
    assert check(plan, [GOOD, bad], [bad, GOOD], 1000, 1000, 0)[1:3] == (1, 1)
    assert check(plan, [bad], [GOOD], 1001, 1000, 0)[0] == 0 and check(plan, [GOOD], [bad], 1000, 1001, 0)[0] == 0
    assert check(plan, [(10, 20, 100, 8, 1)], [GOOD], 1000, 1000, 1)[0] == 0
    assert check(plan, [GOOD], [(5000, 5000, TIB, 77, _rezip.ABSENT | 1)], 1000, 1000, 0)[0] == 0
    assert check(plan, [], [], 0, 0, 0) == (0, -1, 0, 0)


def slot(a, b):
    cap = a[2] if b[4] & _rezip.ABSENT or a[2] > b[2] else b[2]
    return (cap + 255) & ~255


def py_groups(a, b, limit):
    ends, g0, n = [], 0, len(a)
    while g0 < n:
        total, g1, live = 0, g0, 0
        while g1 < n:
            s = 0 if b[g1][4] & _rezip.ABSENT else 2 * slot(a[g1], b[g1])
            if live and s and total + s > limit:
                break
            total += s
            live += s != 0
            g1 += 1
        ends.append(g1)
        g0 = g1
    return ends


def groups(plan, a, b, limit):
    ta, tb = rows(a), rows(b)
    ends = (ctypes.c_int * (len(a) + 1))()
    n = plan.rp_groups(ta.ctypes.data, tb.ctypes.data, len(a), limit, ends, len(a) + 1)
    return list(ends[:n])


def random_lists(count=200, seed=5):
    rnd = random.Random(seed)
    out = []
    for _ in range(count):
        n = rnd.choice((0, 1, 2, 5, 17, 60))
        a, b = [], []
        for _ in range(n):
            cap = rnd.choice((0, 1, 255, 256, 257, 4096, 70000, rnd.randrange(1 << 20)))
            capb = cap if rnd.random() < 0.7 else rnd.choice((0, cap + 1, max(cap - 1, 0), rnd.randrange(1 << 20)))
            bad = rnd.random() < 0.03
            a.append((rnd.randrange(1 << 20), rnd.randrange(1 << 20), cap, 1 if bad else rnd.choice((0, 8, 9, 12, 14)), rnd.choice((0, 0, 0, 1, 2))))
            b.append((rnd.randrange(1 << 20), rnd.randrange(1 << 20), capb, rnd.choice((0, 8, 9, 12, 14)), rnd.choice((0, 0, 2, _rezip.ABSENT))))
        out.append((a, b, 1 << 21, rnd.choice((1 << 21, 1 << 20)), rnd.choice((0, 1)), rnd.choice((1, 512, 8192, 150000, 1 << 21, 1 << 30))))
    return out


def test_groups_and_checks_against_the_restatement(plan):
    kinds = set()
    for a, b, len_a, len_b, have_keys, limit in random_lists():
        assert check(plan, a, b, len_a, len_b, have_keys) == py_check(a, b, len_a, len_b, have_keys)
        ends = groups(plan, a, b, limit)
        assert ends == py_groups(a, b, limit)
        assert (ends[-1] if ends else 0) == len(a) and ends == sorted(set(ends))
        g0 = 0
        for g1 in ends:                                        # a group keeps the limit, or holds one pair that takes room
            sizes = [2 * slot(x, y) for x, y in zip(a[g0:g1], b[g0:g1]) if not y[4] & _rezip.ABSENT]
            assert sum(sizes) <= limit or len([s for s in sizes if s]) <= 1
            kinds.add(len(sizes) > 1)
            g0 = g1
        for x, y in zip(a, b):
            ta, tb = rows([x]), rows([y])
            assert plan.rp_slot(ta.ctypes.data, tb.ctypes.data) == slot(x, y)
    assert kinds == {True, False}


def test_piece_geometry(plan):
    P = 1 << plan.rp_piece_log()
    assert P == 16384
    for n in (0, 1, P - 1, P, P + 1, 2 * P + 3, (1 << 40) - 1):
        assert plan.rp_piece_count(n) == (n + P - 1) // P


def test_the_same_lists_under_the_sanitizers(plan, tmp_path):
    """A program of its own (its own main, -fsanitize=address,undefined), run as a child process on the verdicts and the lists of the tests above:
    it ends clean and prints what the restatements give."""
    exe = str(tmp_path / "rezip_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DREZIP_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe, _rezip.SRC],
                   check=True)
    lines, want = [], []
    for f1 in strings():
        for f2 in strings():
            d = first_diff(f1, f2)
            v, pos, _ = _rezip.compare_1_file(f1, f2)
            lines.append("v %d %d %d" % (len(f1), len(f2), d))
            want.append("%d %d %d" % (v, pos, d))
    for a, b, len_a, len_b, have_keys, limit in random_lists(count=80):
        lines.append("g %d %d %d %d %d" % (len(a), len_a, len_b, have_keys, limit))
        lines += ["%d %d %d %d %d | %d %d %d %d %d" % (x + y) for x, y in zip(a, b)]
        want.append("%d %d %d %d | groups:%s" % (py_check(a, b, len_a, len_b, have_keys) + ("".join(" %d" % e for e in py_groups(a, b, limit)),)))
    src = tmp_path / "lists.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert got[-1] == "plan ok" and got[:-1] == want
