"""The group plan of the readers' batch calls (zip-ada_amd/csrc/zada_reader_plan.h: which entries share a launch group, where each entry's input
and output lie in the group's arena, how much of the outputs comes back) through tests/reader/reader_plan_host.cpp, against the restatement in
tests/_readers.py; the same lists once more through a program of its own built with -fsanitize=address,undefined.  No GPU, and nothing is loaded
into this interpreter with a sanitizer."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import _readers as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIR = os.path.join(ROOT, "tests", "reader")
SRC = os.path.join(_DIR, "reader_plan_host.cpp")
HDR = os.path.join(ROOT, "zip-ada_amd", "csrc", "zada_reader_plan.h")
TOP = (1 << 40) - 1               # the longest stream and the largest output the entry points take


@pytest.fixture(scope="module")
def plan():
    p = os.path.join(_DIR, "libreader_plan_host.so")
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(f) for f in (SRC, HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, SRC], check=True)
    L = ctypes.CDLL(p)
    u64, vp = ctypes.c_uint64, ctypes.c_void_p
    L.rp_groups.argtypes = [ctypes.c_int, vp, vp, u64, vp, ctypes.c_int]
    L.rp_layout.restype = u64
    L.rp_layout.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, u64, vp, vp]
    L.rp_pad16.restype = u64
    L.rp_pad16.argtypes = [u64]
    return L


def named_cases():
    """name -> (limit, [(n_in, cap, wrote)])"""
    return {
        "count 1": (1 << 20, [(100, 1000, 1000)]),
        "count 1, beyond the limit": (64, [(100, 1000, 7)]),
        "count 1, nothing": (1 << 20, [(0, 0, 0)]),
        "zero lengths": (64, [(0, 0, 0), (0, 16, 16), (5, 0, 0), (0, 0, 0), (0, 33, 1), (0, 0, 0)]),
        "zero lengths under a limit of nothing": (0, [(0, 0, 0)] * 4),
        "an entry larger than the limit": (4096, [(100, 1000, 1000), (10, 5000, 4999), (100, 1000, 0), (8000, 1, 1), (1, 1, 1)]),
        "exact fit": (4 * 1024, [(1000, 1024, 1024), (17, 1999, 5), (1, 1, 1)]),                   # 1008 + 1024 + 32 + 2000 + 16 + 16 = 4096
        "one byte over": (4 * 1024 - 1, [(1000, 1024, 1024), (17, 1999, 5), (1, 1, 1)]),
        "padding decides": (64, [(1, 1, 1), (1, 1, 1), (1, 1, 0)]),
        "the longest lengths": (TOP, [(TOP, TOP, TOP)] * 5),
        "the longest lengths in one group": (1 << 45, [(TOP, TOP, TOP), (TOP, TOP, 0), (TOP, TOP, 1)] * 3),
        "the longest lengths, an exact fit": (4 << 40, [(TOP, TOP, TOP), (TOP, TOP, TOP), (1, 1, 1)]),
        "only failures": (1 << 20, [(100, 1000, 0)] * 7),
    }


def random_cases(count=300):
    rng = random.Random(47)
    for _ in range(count):
        limit = rng.choice((1, 16, 48, 4096, 65536, 1 << 20))
        n = rng.choice((1, 2, 3, rng.randrange(1, 60)))
        size = lambda: rng.choice((0, 1, 15, 16, 17, rng.randrange(0, 300), rng.randrange(0, 2 * limit + 2)))
        ents = []
        for _ in range(n):
            cap = size()
            ents.append((size(), cap, rng.choice((0, cap, rng.randrange(0, cap + 1)))))
        yield limit, ents


def all_cases():
    return list(named_cases().values()) + list(random_cases())


def restated(limit, ents):
    """[(g0, g1, in_bytes, out_bytes, hi, io, oo)] by tests/_readers.py, in Python's unbounded integers"""
    n_in, caps, wrote = [e[0] for e in ents], [e[1] for e in ents], [e[2] for e in ents]
    out = []
    for g in R.plan_groups(n_in, caps, limit):
        io, oo = R.plan_offsets(n_in, caps, g)
        out.append(g + (R.plan_extent(oo, g[2], wrote[g[0]:g[1]]), io, oo))
    return out


def test_the_restatement_itself():
    """what the plan promises, on the restatement: every entry in exactly one group, in order; a group within the limit unless it is one entry;
    a group closed only where the next entry would not fit; buffers at multiples of 16 that do not overlap; nothing beyond 2 ** 64"""
    for limit, ents in all_cases():
        groups = restated(limit, ents)
        assert [g[0] for g in groups] == [0] + [g[1] for g in groups[:-1]] and groups[-1][1] == len(ents)
        for k, (g0, g1, ib, ob, hi, io, oo) in enumerate(groups):
            assert g1 > g0 and (ib + ob <= limit or g1 == g0 + 1)
            if g1 < len(ents):
                assert ib + ob + R.pad16(ents[g1][0]) + R.pad16(ents[g1][1]) > limit
            assert ib + ob + 16 < 1 << 64 and all(x % 16 == 0 for x in io + oo + [ib, ob])
            spans = [(io[i], ents[g0 + i][0]) for i in range(g1 - g0)] + [(oo[i], ents[g0 + i][1]) for i in range(g1 - g0)]
            assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= ib + ob
            assert io[0] == 0 and oo[0] == ib and 0 <= hi <= ob
            last = [i for i in range(g1 - g0) if ents[g0 + i][2]]
            assert hi == (oo[last[-1]] + ents[g0 + last[-1]][2] - ib if last else 0)
    names = named_cases()
    assert len(restated(*names["exact fit"])) == 1 and len(restated(*names["one byte over"])) == 2
    assert [g[:2] for g in restated(*names["an entry larger than the limit"])] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert [g[:2] for g in restated(*names["padding decides"])] == [(0, 2), (2, 3)]
    assert [g[:4] for g in restated(*names["the longest lengths"])] == [(i, i + 1, 1 << 40, 1 << 40) for i in range(5)]
    assert [g[:4] for g in restated(*names["the longest lengths in one group"])] == [(0, 9, 9 << 40, 9 << 40)]
    assert [g[:2] for g in restated(*names["the longest lengths, an exact fit"])] == [(0, 2), (2, 3)]


def test_the_header_equals_the_restatement(plan):
    assert [plan.rp_pad16(x) for x in (0, 1, 15, 16, 17, TOP)] == [0, 16, 16, 16, 32, 1 << 40]
    for limit, ents in all_cases():
        n = len(ents)
        n_in, caps, wrote = (np.array([e[k] for e in ents], dtype=np.uint64) for k in range(3))
        rows = np.zeros((n, 4), dtype=np.uint64)
        want = restated(limit, ents)
        assert plan.rp_groups(n, n_in.ctypes.data, caps.ctypes.data, limit, rows.ctypes.data, n) == len(want)
        assert [tuple(int(x) for x in r) for r in rows[:len(want)]] == [g[:4] for g in want]
        for g0, g1, ib, ob, hi, io, oo in want:
            a, b = np.full(g1 - g0, 77, np.uint64), np.full(g1 - g0, 77, np.uint64)
            assert plan.rp_layout(g0, n, n_in.ctypes.data, caps.ctypes.data, wrote.ctypes.data, limit, a.ctypes.data, b.ctypes.data) == hi
            assert [int(x) for x in a] == io and [int(x) for x in b] == oo
    assert plan.rp_groups(0, None, None, 1 << 20, None, 0) == 0


def test_the_same_lists_under_the_sanitizers(tmp_path):
    """A program of its own (its own main, -fsanitize=address,undefined), run as a child process on the lists of the tests above: it ends clean and
    prints what the restatement gives."""
    exe = str(tmp_path / "reader_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DREADER_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", exe, SRC],
                   check=True)
    lines, want = [], []
    for limit, ents in all_cases():
        lines.append("%d %d %s" % (limit, len(ents), " ".join("%d %d %d" % e for e in ents)))
        want.append("".join("| %d %d %d %d %d %s" % (g[:5] + (" ".join(str(x) for x in g[5] + g[6]),)) for g in restated(limit, ents)))
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert got[-1] == "plan ok" and got[:-1] == want
