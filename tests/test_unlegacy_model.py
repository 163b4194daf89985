"""The Shrink / Reduce / Implode readers on the CPU: the product's logic header (zip-ada_amd/csrc/zada_unlegacy_logic.h, one lane) against the
decoders as the reference states them (tests/unlegacy/unlegacy_model.c), PKZIP's own streams, the encoder models of tests/legacy/, Info-ZIP's
unzip where it is installed, and a corpus of damaged streams -- the latter once more under ASan + UBSan in a stand-alone program."""
import hashlib
import random
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import _legacy as L
import _unlegacy as U


def _both(method, flags, stream, cap, census=None):
    """The two forms on one case: they agree on everything; -> the logic header's result."""
    h = U.host_decode(method, flags, stream, cap)
    s = U.stated_decode(method, flags, stream, cap, census)
    assert (h[0], h[1], h[2], h[3], h[5]) == s, (method, flags, len(stream), cap, h[0], h[2:], s[0], s[2:])
    return h


@pytest.fixture(scope="module")
def census():
    return np.zeros(len(U.CENSUS), dtype=np.uint64)


def test_fixtures_decode_to_the_digest(census):
    assert [r["format"] for r, _ in U.fixtures()] == [2, 3, 4, 5, 1, 6, 6]
    for row, payload in U.fixtures():
        assert len(payload) == row["csize"] and row["size"] == 81682 and row["crc32"] == "840ff735"
        rc, out, out_len, in_used, reg, rec = _both(row["format"], row["flags"], payload, row["size"], census)
        assert rc == 0 and out_len == row["size"] and in_used == len(payload) and rec == (0, in_used, out_len, 0), (row["file"], rc, rec)
        assert hashlib.sha256(out).hexdigest() == row["sha256"] and reg ^ 0xFFFFFFFF == int(row["crc32"], 16), row["file"]


@pytest.mark.parametrize("method", [1, 2, 3, 4, 5])
def test_encoder_streams_round_trip(method, census):
    r = random.Random(100 + method)
    ins = L.gpu_test_inputs(method) + [L.edge_input(r.randint(0, 3000), seed=1000 + k) if k % 4 else L.rnd(k, r.randint(0, 3000), bytes(range(256))) for k in range(2000)]
    for d in ins:
        s = U.encode(d, method)
        rc, out, out_len, in_used, reg, rec = _both(method, 0, s, len(d), census)
        assert rc == 0 and out == d and out_len == len(d), (method, len(d), rec)
        assert in_used == (0 if method == 1 and not d else len(s)) and reg == zlib.crc32(d) ^ 0xFFFFFFFF, (method, len(d), in_used, len(s))
        assert (L.unshrink(s, len(d)) if method == 1 else L.unreduce(s, method - 1, len(d))) == d          # (the encoder models' own decoders)


@pytest.mark.parametrize("flags", U.IMPLODE_FLAGS)
def test_imploder_streams_round_trip(flags, census):
    for name, d, reach in U.implode_inputs():
        s = U.implode(d, flags, reach)
        rc, out, out_len, in_used, reg, rec = _both(6, flags, s, len(d), census)
        assert rc == 0 and out == d and in_used == len(s) and reg == zlib.crc32(d) ^ 0xFFFFFFFF, (name, flags, rec)


def test_crafted_streams(census):
    for name, (method, flags, s, cap, rule) in U.crafted().items():
        rc, out, out_len, in_used, reg, rec = _both(method, flags, s, cap, census)
        assert rec[0] == rule and rc == (U.E_DATA if rule else 0), (name, rc, rec)
        if rule:
            assert (out, out_len, in_used, reg) == (b"", 0, 0, 0xFFFFFFFF), name
    assert _both(1, 0, U.crafted()["shrink_orphans_valid"][2], 8)[1] == b"aaaaaaab"
    assert _both(5, 0, U.crafted()["reduce_zero_fill"][2], 10)[1] == bytes(9) + b"A"
    assert _both(2, 0, U.crafted()["reduce_slen_63"][2], 6)[1] == b"A\0A\0A\0"
    assert U.host().ug_unlegacy(7, 0, None, 0, None, 0, 0, (U.ctypes.c_uint64 * 8)()) == -1


def test_shrink_stream_with_a_full_table(census):
    d = U.full_table_input()
    s = U.shrink_no_clear(d)
    before = int(census[U.CENSUS.index("sh_full_table")])
    rc, out, out_len, in_used, reg, rec = _both(1, 0, s, len(d), census)
    assert rc == 0 and out == d and in_used == len(s) and census[U.CENSUS.index("sh_full_table")] > before + 100
    assert L.unshrink(s, len(d)) == d


def test_census_reaches_every_branch(census):
    """(runs behind the tests above: fixtures, encoder streams, imploder streams and crafted streams together)"""
    missing = [n for n, v in zip(U.CENSUS, census) if v == 0]
    assert not missing, (missing, dict(zip(U.CENSUS, census.tolist())))


@pytest.mark.skipif(shutil.which("unzip") is None, reason="no unzip on this machine")
def test_unzip_accepts_the_shrink_and_implode_streams(tmp_path):
    entries = []
    for row, payload in U.fixtures():
        if row["format"] in (1, 6):
            entries.append((row["file"], payload, row["format"], row["flags"], int(row["crc32"], 16), row["size"]))
    for flags in U.IMPLODE_FLAGS:
        for name, d, reach in U.implode_inputs():
            entries.append(("%s_%d" % (name, flags), U.implode(d, flags, reach), 6, flags, zlib.crc32(d), len(d)))
    for name, d in L.shrink_inputs().items():
        entries.append((name, U.encode(d, 1), 1, 0, zlib.crc32(d), len(d)))
    p = tmp_path / "legacy.zip"
    p.write_bytes(U.zip_of(entries))
    r = subprocess.run(["unzip", "-t", str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and "No errors detected" in r.stdout, (r.stdout[-1500:], r.stderr[-500:])


@pytest.fixture(scope="module")
def corpus_results():
    cases = U.damaged_corpus()
    return cases, [U.host_decode(m, f, s, cap) for m, f, s, cap in cases]


def test_damaged_corpus_both_forms_agree(corpus_results):
    cases, res = corpus_results
    assert len(cases) >= 20000
    seen = {}
    for (m, f, s, cap), h in zip(cases, res):
        st = U.stated_decode(m, f, s, cap)
        assert (h[0], h[1], h[2], h[3], h[5]) == st, (m, f, len(s), cap, h[0], h[2:], st[0], st[2:])
        assert h[0] == (U.E_DATA if h[5][0] else 0)
        if h[0]:
            assert (h[1], h[2], h[3], h[4]) == (b"", 0, 0, 0xFFFFFFFF)
        else:
            assert h[2] == cap and h[3] <= len(s) and h[4] == zlib.crc32(h[1]) ^ 0xFFFFFFFF
        seen[(m, h[5][0])] = seen.get((m, h[5][0]), 0) + 1
    rules = {rule for _, rule in seen}
    assert rules == set(range(len(U.RULES))), sorted(seen.items())          # every rule of UlgRule occurs, and so do valid streams
    assert U.host().ug_nrules() == len(U.RULES)
    for m in range(1, 7):                                                    # both departures under every method
        assert seen.get((m, 1)) and seen.get((m, 2)) and seen.get((m, 0)), (m, sorted(seen.items()))


def test_damaged_corpus_under_sanitizers(corpus_results, tmp_path):
    """The same corpus through the stand-alone program built with -fsanitize=address,undefined (every buffer an exact-size heap block), as a child process."""
    cases, res = corpus_results
    got = U.run_program(cases, tmp_path)
    for k, h in enumerate(res):
        want = [h[0] & 0xFFFFFFFFFFFFFFFF, h[2], h[3], h[5][0], h[5][1], h[4], h[5][2], 0, 0]          # (the CRC-32 register stands for the bytes)
        assert got[k].tolist() == want, (k, cases[k][0], cases[k][1], cases[k][3], got[k].tolist(), want)
