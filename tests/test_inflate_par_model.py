"""The CPU model of the parallel Inflate (tests/inflate_par/inflate_par_host.cpp: zip-ada_amd/csrc/zada_inflate_par_logic.h with one lane, the
chunks in a loop) against zlib on valid streams and against the one-wave model on damaged ones; the finder's census, which the default of
"inflate_par_repair_pct" and the GPU tests' assertions on the record rest on; the model under ASan + UBSan as a program of its own."""
import json
import os
import struct
import subprocess
import sys
import zlib

import pytest

import _inflate
import _inflate_par as P
from _common import ROOT
from _inflate import model_inflate

CENSUS = os.path.join(ROOT, "profiles", "inflate_par", "finder_census.json")
HUGE_KIB = 65536          # a chunk larger than every stream here: the stream is one chunk


def test_valid_streams_against_zlib():
    n = par = 0
    for label, data, stream in _inflate.valid_streams():
        want = (0, data, len(data), _inflate.zlib_in_used(stream), zlib.crc32(data) ^ 0xFFFFFFFF)
        assert zlib.decompress(stream, -15) == data, label
        for ck in (4, 16, HUGE_KIB):
            rc, out, ol, used, reg, _, info = P.model_inflate_par(stream, len(data), ck)
            assert (rc, out, ol, used, reg) == want, (label, ck, info)
            assert info["chunks"] == (len(stream) + (ck << 10) - 1) // (ck << 10) and info["streams"] == 1, (label, ck, info)
            if ck == HUGE_KIB:
                assert info["fell_back"] == 1 and info["reason"] == "single chunk", (label, info)
            elif not info["fell_back"]:
                assert info["live_chunks"] >= 2 and info["scout_rounds"] == 1 + info["repairs"], (label, ck, info)
                par += 1
            n += 1
    assert n > 1500 and par > 300, (n, par)


DAMAGED_STEP = 1          # every k-th case of the 20 000: all of them take about a minute here


def test_damaged_streams_against_the_one_wave_model():
    cases, _ = _inflate.damaged_corpus()
    assert len(cases) == 20000
    picked = list(range(0, len(cases), DAMAGED_STEP))
    assert {k % 4 for k in picked} == {0, 1, 2, 3}, "all four kinds of damage"
    n_par = n_bad = 0
    for k in picked:
        s, cap = cases[k]
        rc, out, ol, used, reg, rule = model_inflate(s, cap, 8)
        got = P.model_inflate_par(s, cap, 4)
        assert got[:6] == (rc, out, ol, used, reg, rule), (k, got[5:], rule)
        if rc:
            assert got[6]["fell_back"] == 1, (k, got[6])          # a damaged stream is the one wave's to judge
            n_bad += 1
        n_par += not got[6]["fell_back"]
    assert n_bad > len(picked) // 4 and n_par > len(picked) // 20, (n_bad, n_par)


def _census_row(label, stream, size, ck):
    row = dict(stream=label, bytes=len(stream), chunk_kib=ck)
    row.update(P.census(stream, ck))
    info = P.model_inflate_par(stream, size, ck, repair_pct=100)[6]
    row.update(live_chunks=info["live_chunks"], repairs=info["repairs"], fell_back=info["fell_back"], reason=info["reason"])
    return row


def census_rows(big=False):
    """The census: every valid stream (without the 4 MiB few-symbol inputs unless big) and the 2 MiB corpus streams, at 4 and 16 KiB chunks, the
    repair bound out of the way (100 per cent) so that `repairs` is what the chain needs."""
    rows = []
    streams = [(l, s, len(d)) for l, d, s in _inflate.valid_streams(big)] + [(l, s, len(d)) for l, d, s in P.corpus_streams()]
    for label, stream, size in streams:
        for ck in (4, 16):
            if len(stream) > ck << 10:
                rows.append(_census_row(label, stream, size, ck))
    return rows


def test_finder_census_and_the_repair_bound():
    """What the committed census says about the 2 MiB corpus streams is what the model finds today; on the dynamic-block streams the GPU tests
    name, the model stays within the default repair bound without falling back; the finder never lost a candidate it should have found."""
    with open(CENSUS) as f:
        committed = {(r["stream"], r["chunk_kib"]): r for r in json.load(f)["rows"]}
    streams = {l: (d, s) for l, d, s in P.corpus_streams()}
    assert len(streams["corpus_2m/oracle10"][1]) == 722132
    for label, (data, stream) in streams.items():
        for ck in (4, 16):
            row = _census_row(label, stream, len(data), ck)
            assert committed[(label, ck)] == row, (label, ck)
            # a true block start the finder can see (dynamic, not final) is missed only when an earlier candidate in the same chunk took its place
            assert row["found_true"] + row["false_positive"] + row["found_nothing"] == row["chunks"] - 1
            assert row["false_positive"] == 0, row
    assert committed[("corpus_2m/oracle10", 4)]["blocks"] == 15
    # the margin of the default: the dynamic-block streams of the census need far fewer repairs than the bound allows
    for r in committed.values():
        if r["dynamic"] >= r["blocks"] - 1 and r["blocks"] > 1:
            assert r["repairs"] <= 1 + r["false_positive"], r
    for label in P.NAMED_DYNAMIC:
        data, stream = streams[label]
        for ck in (4, 16):
            rc, out, _, _, _, _, info = P.model_inflate_par(stream, len(data), ck)
            assert rc == 0 and out == data and info["fell_back"] == 0 and info["live_chunks"] >= 2, (label, ck, info)
            assert info["repairs"] <= (info["chunks"] * P.REPAIR_PCT) // 100 + 2, (label, ck, info)


def test_the_streams_the_gpu_tests_assert_markers_and_repairs_on():
    """The GPU tests assert fell_back == 0 with marker bytes > 0, or repairs >= 1, on these streams at 4 KiB chunks: the model says they can."""
    for name, (data, stream, markers) in P.marker_streams().items():
        rc, out, _, used, _, _, info = P.model_inflate_par(stream, len(data), 4)
        assert rc == 0 and out == data and used == len(stream) and info["fell_back"] == 0 and info["live_chunks"] >= 2, (name, info)
        assert (info["marker_bytes"] > 0) == markers, (name, info)
    inner, outer = P.planted_false_positive()
    rc, out, _, _, _, _, info = P.model_inflate_par(outer, len(inner), 4)
    assert rc == 0 and out == inner and info["fell_back"] == 0 and info["repairs"] >= 1, info
    assert P.census(outer, 4)["false_positive"] >= 1              # the inner stream's headers are found, and are no block starts


def test_model_is_clean_under_asan_and_ubsan(tmp_path):
    """The stand-alone program (its own main, nothing preloaded anywhere): the small valid streams at three chunk sizes and every 40th damaged
    stream, on heap buffers of exact size."""
    prog = P.build_check_program()
    cases, _ = _inflate.damaged_corpus()
    path = tmp_path / "cases.bin"
    n = 0
    with open(path, "wb") as f:
        for label, data, stream in _inflate.valid_streams(big=False):
            if len(data) > 400000:
                continue
            for ck in (4, 16, HUGE_KIB):
                f.write(struct.pack("<4I", len(stream), len(data), ck, P.REPAIR_PCT) + stream)
                n += 1
        for _, (data, stream, _) in P.marker_streams().items():
            f.write(struct.pack("<4I", len(stream), len(data), 4, P.REPAIR_PCT) + stream)
            n += 1
        for s, cap in cases[::40]:
            f.write(struct.pack("<4I", len(s), cap, 4, P.REPAIR_PCT) + s)
            n += 1
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and ("par check ok: %d cases" % n) in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__" and sys.argv[1:] == ["census"]:
    os.makedirs(os.path.dirname(CENSUS), exist_ok=True)
    with open(CENSUS, "w") as f:
        json.dump({"what": "finder census of the parallel Inflate's CPU model (tests/test_inflate_par_model.py census)", "rows": census_rows()}, f, indent=1)
    print("wrote", CENSUS)
