"""The bound on the splitter's similarity distance (zip-ada_amd/csrc/zada_descr_bound.h) never falls below the distance itself.

20 000 seeded pairs (reference descriptor, window descriptor), both made by the oracle's length-limited coder on random histograms, with
what the lazy scan would know about the window: a set U that covers the symbols it uses and a set D of symbols it certainly uses.  The
check itself is a C++ program of its own (tests/hostcheck/descr_bound_main.cpp: its own main, built with -fsanitize=address,undefined,
run as a child process) around the header the kernel uses.  No GPU, and nothing is loaded into this interpreter with a sanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest

from _common import ROOT, oracle

HC = os.path.join(ROOT, "tests", "hostcheck")
PAIRS = 20000
ALPHABETS = (2, 30, 150, 286)          # used literal / length symbols
DISTS = (0, 1, 2, 7, 30)               # used distance symbols (0 and 1: Patch_statistics_for_buggy_decoders adds symbols)


def _lengths(freq, mb=15):
    a = np.zeros(len(freq), dtype=np.int32)
    f = np.ascontiguousarray(freq, dtype=np.uint64)
    assert oracle().zo_llhc(f.ctypes.data, len(f), mb, a.ctypes.data) == 0
    return a.astype(np.uint8)


def _counts(rs, k, total, shape):
    """k positive counts of about `total` in all: random (a fresh distribution every time: exponential weights raised to a random power, from
    nearly flat to a few symbols with all the mass), Zipf-like (text), flat, or geometric"""
    if shape == "random":
        w = rs.exponential(1.0, k) ** rs.uniform(0.2, 4.0)
        c = np.maximum(1, (total * w / w.sum()).astype(np.int64))
    elif shape == "flat":
        c = np.full(k, max(1, total // max(k, 1)))
    elif shape == "zipf":
        c = np.maximum(1, (total / (np.arange(k) + 1.0) / np.log(k + 2.0)).astype(np.int64))
        rs.shuffle(c)
    else:
        c = np.maximum(1, (total * 0.5 ** (np.arange(k) * rs.uniform(0.05, 1.0))).astype(np.int64))
        rs.shuffle(c)
    return c


_NOT_EOB = np.setdiff1d(np.arange(286), [256])


def _descriptor(rs, nlit, ndist, shape):
    """(code lengths [320], used symbols before the patch [320] bool) of a window with nlit used literal / length symbols (the end of block
    among them, counted once: zip-compress-deflate.adb:946) and ndist used distance symbols"""
    ll = np.zeros(288, dtype=np.int64)
    pick = rs.permutation(_NOT_EOB)[:nlit - 1]
    ll[pick] = _counts(rs, nlit - 1, 4097, shape)
    ll[256] = 1
    d = np.zeros(32, dtype=np.int64)
    if ndist:
        d[rs.choice(30, ndist, replace=False)] = _counts(rs, ndist, 800, shape)
    used = np.concatenate([ll > 0, d > 0])
    k = int((d > 0).sum())                                   # Patch_statistics_for_buggy_decoders :340-365
    if k == 0:
        d[0] = d[1] = 1
    elif k == 1:
        if d[0] == 0:
            d[0] = 1
        else:
            d[1] = 1
    return np.concatenate([_lengths(ll), _lengths(d)]), used


def _mask(b):
    return np.packbits(np.asarray(b, dtype=bool), bitorder="little").view("<u4").copy()      # symbol s: bit s & 31 of word s >> 5


def _known(rs, used, exact):
    """(U, D) as the scan has them: D = symbols seen in the part of the window that lies in whole pieces, U = D and what the last, partly
    covered piece holds -- here: exact sets, or a random subset / superset; then the patch rule of db_patch_dist"""
    D = used.copy(); U = used.copy()
    if not exact:
        D &= rs.rand(320) < 0.8
        U |= (rs.rand(320) < 0.05) & (np.arange(320) < 286) | (rs.rand(320) < 0.1) & (np.arange(320) >= 288) & (np.arange(320) < 318)
    D[256] = U[256] = True
    if D[288:].sum() < 2:
        U[288] = U[289] = True
    return _mask(U), _mask(D)


@pytest.fixture(scope="module")
def checker():
    exe = os.path.join(HC, "descr_bound_check_asan")
    src = os.path.join(HC, "descr_bound_main.cpp")
    deps = [src] + [os.path.join(ROOT, "zip-ada_amd", "csrc", h) for h in ("zada_descr_bound.h", "zada_logic.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, src], check=True)
    return exe


def _cases():
    rs = np.random.RandomState(20261)

    def fresh():
        # a histogram of its own for every descriptor: alphabet and distances by turns, the counts random (three in four) or of a fixed shape;
        # the two alphabets coded separately, as the product codes them
        k = rs.randint(1 << 30)
        shape = ("random", "random", "random", ("zipf", "flat", "geo")[k % 3])[(k >> 8) % 4]
        return _descriptor(rs, ALPHABETS[(k >> 16) % len(ALPHABETS)], DISTS[(k >> 20) % len(DISTS)], shape)
    out = []
    # directed 0: a 150-symbol text-like window against itself, exact sets.  directed 1: 257 flat literal / length symbols and 4 flat distances
    text = _descriptor(np.random.RandomState(1), 150, 20, "zipf")
    flat = _descriptor(np.random.RandomState(2), 257, 4, "flat")
    for bl, used in (text, flat):
        U, D = _known(rs, used, True)
        out.append((bl, bl, U, D))
    while len(out) < PAIRS + 2:
        ref = fresh()[0]
        win, used = fresh()
        U, D = _known(rs, used, exact=bool(len(out) & 1))
        out.append((ref, win, U, D))
    return out, flat[0]


def test_bound_is_never_below_the_distance(checker, tmp_path):
    cases, flat = _cases()
    assert sorted(set(flat[:288])) == [0, 8, 9] and int((flat[:288] > 0).sum()) == 257      # 255 codes of 8 bits, 2 of 9
    p = tmp_path / "cases.bin"
    with open(p, "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for ref, win, U, D in cases:
            f.write(ref.tobytes()); f.write(win.tobytes()); f.write(U.tobytes()); f.write(D.tobytes())
    r = subprocess.run([checker, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    m = re.search(r"cases (\d+) violations (\d+) plain_violations (\d+) decided (\d+) plain_decided (\d+) bad_sets (\d+)", r.stdout)
    assert m and int(m.group(1)) == PAIRS + 2 and int(m.group(2)) == 0 and int(m.group(3)) == 0 and int(m.group(6)) == 0
    assert int(m.group(4)) > 0                                                       # (the bound is not vacuous on these pairs)
    d = {int(k): (int(t), int(b), int(pl)) for k, t, b, pl in re.findall(r"directed (\d+) true (\d+) bound (\d+) plain (\d+)", r.stdout)}
    # identical vectors, exact sets: a 150-symbol text-like window is decided (205 000 = step level 3's threshold) ...
    assert d[0][0] == 0 and d[0][1] < 205000
    # ... and the flat 257-symbol one is decided with the Kraft term and what D proves, not by the plain bound
    assert d[1][0] == 0 and d[1][1] < 205000 <= d[1][2]
