"""The CPU model of the parallel Inflate on Deflate64 streams (tests/inflate_par/inflate_par64_host.cpp: the format 9 pipeline of
zip-ada_amd/csrc/zada_inflate_par_logic.h with one lane -- 32-bit symbols, a window of 65 536, the finder without the HDIST rule) against the
one-wave model on the streams of _deflate64.py, valid and damaged; the record the GPU test (test_gpu_inflate_par64.py) asserts; the finder's
census; the model under ASan + UBSan as a program of its own."""
import json
import os
import struct
import subprocess
import sys
import zlib

import _deflate64 as D
import _inflate_par64 as P
from _common import ROOT
from _inflate import E_DATA, model_inflate
from _inflate_par import REPAIR_PCT

CENSUS = os.path.join(ROOT, "profiles", "inflate_par", "finder_census64.json")
HUGE_KIB = 65536          # a chunk larger than every stream here: the stream is one chunk


def test_the_writer_makes_deflate64_streams():
    """Every stream decodes to its input through the one-wave model as format 9 and is refused as format 8; it holds matches beyond Deflate's
    window, matches longer than Deflate's 258 and distance codes 30 or 31."""
    for name, (data, stream, tokens, info) in D.streams().items():
        rc, out, ol, used, reg, rule = model_inflate(stream, len(data), 9)
        assert (rc, out, ol, used, reg ^ 0xFFFFFFFF) == (0, data, len(data), len(stream), zlib.crc32(data)), (name, rule)
        assert bytes(D.expand(tokens)) == data and info["block_out"][-1] == len(data) and info["block_bits"][-1] + 7 >> 3 == len(stream), name
        assert model_inflate(stream, len(data), 8)[0] == E_DATA, name
        far, long_, codes = D.token_stats(tokens)
        assert far > 0 and long_ > 0 and codes > 0, (name, far, long_, codes)
    s = D.streams()
    assert len(s["period_49152"][0]) == 393216 and len(s["period_65000"][0]) == 520000
    assert len(s["far_first"][3]["block_bits"]) == 6 and s["far_first"][3]["block_out"][2] == 65536 == s["near_first"][3]["block_out"][2]
    # what deflate64 (data, per_block) makes is what the token lists make
    d = s["period_49152"][0][:60000]
    small = D.deflate64(d, 500)
    assert model_inflate(small, len(d), 9)[:2] == (0, d) and small == D.deflate64_blocks([D.tokenize(d)[i:i + 500] for i in range(0, len(D.tokenize(d)), 500)])


def test_the_parallel_model_equals_the_one_wave_model():
    """At 4 and 16 KiB chunks: rc, bytes, out_len, in_used, CRC register and rule, and the record the GPU test asserts."""
    for name, (data, stream, _, _) in D.streams().items():
        want = model_inflate(stream, len(data), 9)
        assert want[0] == 0 and want[1] == data
        for ck in P.CHUNKS_KIB:
            got = P.model_inflate_par64(stream, len(data), ck)
            info = got[6]
            assert got[:6] == want, (name, ck, info)
            assert info["chunks"] == (len(stream) + (ck << 10) - 1) // (ck << 10) and info["streams"] == 1, (name, ck, info)
            assert info["fell_back"] == 0 and info["reason"] == "none" and info["live_chunks"] >= 2 and info["marker_bytes"] > 0, (name, ck, info)
            assert info["repairs"] <= info["chunks"] * REPAIR_PCT // 100 + 2 and info["scout_rounds"] == 1 + info["repairs"], (name, ck, info)
            assert len(info["live_bytes"]) == info["live_chunks"] and sum(info["live_bytes"]) == len(data), (name, ck, info)
        got = P.model_inflate_par64(stream, len(data), HUGE_KIB)
        assert got[:6] == want and got[6]["fell_back"] == 1 and got[6]["reason"] == "single chunk", (name, got[6])
        # the CRC register started elsewhere, and a cap one short: the one wave's verdict
        assert P.model_inflate_par64(stream, len(data), 4, crc=0x12345678)[:6] == model_inflate(stream, len(data), 9, crc=0x12345678), name
        short = P.model_inflate_par64(stream, len(data) - 1, 4)
        assert short[:6] == model_inflate(stream, len(data) - 1, 9) and short[0] == E_DATA and short[6]["fell_back"] == 1, (name, short[6])
    # the archive of the GPU test reads period_65000 at the default chunk size of 64 KiB
    data, stream, _, _ = D.streams()["period_65000"]
    info = P.model_inflate_par64(stream, len(data), 64)[6]
    assert info["fell_back"] == 0 and info["live_chunks"] >= 2 and info["marker_bytes"] > 0, info
    # both branches of the window step's `from`: a live chunk with more symbols than the window holds, and one with fewer
    data, stream, _, _ = D.streams()["period_65000"]
    live = P.model_inflate_par64(stream, len(data), 4)[6]["live_bytes"]
    assert max(live[1:]) > 65536 and min(live[1:]) < 65536, live
    # the maximal tokens of far_first / near_first begin in a live chunk that is not the first one: they run from markers into their own chunk
    for name in ("far_first", "near_first"):
        data, stream, _, _ = D.streams()[name]
        info = P.model_inflate_par64(stream, len(data), 4)[6]
        assert sum(info["live_bytes"][:2]) == 65536 and info["live_bytes"][2] > 65538 and info["repairs"] == 1, (name, info)


def test_damaged_streams_against_the_one_wave_model():
    cases = D.damaged_cases()
    assert len(cases) == 2000 and {(k % 4, (k // 4) % 4) for k in range(len(cases))} == {(a, b) for a in range(4) for b in range(4)}
    n_par = n_bad = 0
    for k, (name, s, cap) in enumerate(cases):
        want = model_inflate(s, cap, 9)
        got = P.model_inflate_par64(s, cap, 4)
        assert got[:6] == want, (k, name, got[5:], want[5])
        if want[0]:
            assert got[6]["fell_back"] == 1, (k, name, got[6])          # a damaged stream is the one wave's to judge
            n_bad += 1
        n_par += not got[6]["fell_back"]
    assert n_bad > len(cases) // 10 and n_par > len(cases) // 20, (n_bad, n_par)
    # the 60 of them the GPU test runs: none is empty, and the same shares hold
    picked = D.gpu_damaged_picks()
    verdicts = [(model_inflate(s, cap, 9)[0], P.model_inflate_par64(s, cap, 4)[6]["fell_back"]) for _, s, cap in picked]
    assert all(len(s) > 0 for _, s, _ in picked) and len(picked) == 60
    assert sum(1 for rc, _ in verdicts if rc) > 60 // 10 and sum(1 for _, fb in verdicts if not fb) > 60 // 20, verdicts


def census_rows():
    """The finder on the four streams at 4 and 16 KiB chunks, the repair bound out of the way (100 per cent) so that `repairs` is what the chain
    needs; right: the parallel model's bytes are the input."""
    rows = []
    for name, (data, stream, _, _) in D.streams().items():
        for ck in P.CHUNKS_KIB:
            row = dict(stream=name, bytes=len(stream), chunk_kib=ck)
            row.update(P.census(stream, ck))
            rc, out, _, _, _, _, info = P.model_inflate_par64(stream, len(data), ck, repair_pct=100)
            row.update(live_chunks=info["live_chunks"], repairs=info["repairs"], fell_back=info["fell_back"], reason=info["reason"], marker_bytes=info["marker_bytes"],
                       right=int(rc == 0 and out == data))
            rows.append(row)
    return rows


def test_finder_census():
    """The committed census is what the model finds today.  The filter has lost a rule (any HDIST passes), so false positives are reported, not
    forbidden: the chain makes them harmless, and what is asserted is that the bytes are right on every row."""
    with open(CENSUS) as f:
        committed = json.load(f)["rows"]
    rows = census_rows()
    assert committed == rows
    for row in rows:
        assert row["found_true"] + row["false_positive"] + row["found_nothing"] == row["chunks"] - 1, row
        assert row["right"] == 1 and row["fell_back"] == 0, row
        assert row["repairs"] <= row["chunks"] * REPAIR_PCT // 100 + 2, row
    print("false positives:", {(r["stream"], r["chunk_kib"]): r["false_positive"] for r in rows})


def test_model_is_clean_under_asan_and_ubsan(tmp_path):
    """The stand-alone program (its own main, nothing preloaded anywhere): the valid streams at three chunk sizes and every 40th damaged one, on
    heap buffers of exact size."""
    prog = P.build_check_program()
    path = tmp_path / "cases.bin"
    n = 0
    with open(path, "wb") as f:
        for name, (data, stream, _, _) in D.streams().items():
            for ck in P.CHUNKS_KIB + (HUGE_KIB,):
                f.write(struct.pack("<4I", len(stream), len(data), ck, REPAIR_PCT) + stream)
                n += 1
        for name, s, cap in D.damaged_cases()[::40]:
            f.write(struct.pack("<4I", len(s), cap, 4, REPAIR_PCT) + s)
            n += 1
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and ("par64 check ok: %d cases" % n) in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__" and sys.argv[1:] == ["census"]:
    os.makedirs(os.path.dirname(CENSUS), exist_ok=True)
    with open(CENSUS, "w") as f:
        json.dump({"what": "finder census of the parallel Inflate's CPU model on Deflate64 streams (tests/test_inflate_par64_model.py census)", "rows": census_rows()}, f, indent=1)
    print("wrote", CENSUS)
