"""The CPU model of the batched parallel Inflate (tests/inflate_par/inflate_par_batch_host.cpp: the plan of
zip-ada_amd/csrc/zada_inflate_par_batch_plan.h around zada_inflate_par_logic.h, every kernel a loop) against the single-stream models
(_inflate_par.model_inflate_par, _inflate.model_inflate), which stay its reference: the same answer per stream, the same summed record except
scout_rounds, which is what the batch is for; the model under ASan + UBSan as a program of its own."""
import os
import struct
import subprocess

import _inflate
import _inflate_par as P
import _inflate_par_batch as B
from _inflate import model_inflate

# the repairs each of the rows needs at 4 KiB chunks by the single-stream model: what the GPU tests' 139 and 64 scout launches rest on
REPAIRS = [1, 1, 3, 2, 63, 1, 1, 33, 1, 1, 1, 0, 0, 0, 1, 3, 3, 2, 1, 1]


def _same_as_single(rows_out, singles):
    for (label, data, stream), got, one in zip(B.the_rows(), rows_out, singles):
        assert got[:5] == one[:5] and got[0] == 0 and got[1] == data, label
        assert got[5] == ("taken" if not one[6]["fell_back"] else one[6]["reason"]), (label, got[5], one[6])


def test_the_rows_equal_the_single_stream_model():
    singles = B.single_records()
    assert [r[6]["repairs"] for r in singles] == REPAIRS
    assert [r[6]["reason"] for r in singles] == ["none"] * 11 + ["single chunk"] * 3 + ["none"] * 6
    marks = [r[6]["marker_bytes"] for r in singles]
    assert marks[4] == 0 and marks[6] == 0 and max(marks) == 1262009, marks          # random_64k_x16, planted
    rows_out, rec, ends = B.rows_model()
    _same_as_single(rows_out, singles)
    want = B.sum_records([r[6] for r in singles])
    assert want["scout_rounds"] == 139 and want["streams"] == 20 and want["fell_back"] == 3 and want["repairs"] == 119
    assert {k: v for k, v in rec.items() if k != "scout_rounds"} == {k: v for k, v in want.items() if k != "scout_rounds"}
    assert rec["scout_rounds"] == 64 and ends == [20]                                # one sub-pass: 1 + the 63 repairs of random_64k_x16


def test_the_workspace_bound_cuts_passes_and_changes_no_byte():
    """inflate_par_batch_mib = 1: a pass promises at most 1 MiB of symbols, 2 bytes per output byte; a stream that alone promises more is a pass of
    its own.  scout_rounds is the sum over the sub-passes of 1 + the most repairs of a stream in it, recomputed here from the single-stream records
    and the cut the model reports."""
    singles = B.single_records()
    rows_out, rec, ends = B.rows_model(1)
    _same_as_single(rows_out, singles)
    # the cut, recomputed: rows in order while the promise stays within the bound
    caps = [2 * len(d) for _, d, _ in B.the_rows()]
    mine, k = [], 0
    while k < 20:
        total, j = 0, k
        while j < 20 and (j == k or total + caps[j] <= 1 << 20):
            total += caps[j]
            j += 1
        mine.append(j)
        k = j
    assert ends == mine and len(ends) > 5
    first = dict(zip(ends, [0] + ends))
    alone = [e for e in ends if e - first[e] == 1 and caps[first[e]] > 1 << 20]
    assert any(len(B.the_rows()[e - 1][1]) == 2 << 20 for e in alone)                # a 2 MiB output alone in its pass
    rounds = 0
    for e in ends:
        reps = [singles[k][6]["repairs"] for k in range(first[e], e) if singles[k][6]["chunks"] >= 2]
        if reps:
            rounds += 1 + max(reps)
    assert rec["scout_rounds"] == rounds
    full = B.rows_model()[1]
    assert {k: v for k, v in rec.items() if k != "scout_rounds"} == {k: v for k, v in full.items() if k != "scout_rounds"}


def test_a_table_of_one_is_the_single_model():
    for k in (2, 4, 11, 19):
        label, data, stream = B.the_rows()[k]
        rows_out, rec, ends = B.model_batch([(8, stream, len(data))], 4)
        one = B.single_records()[k]
        assert rows_out[0][:5] == one[:5] and rec == one[6] and ends == [1], (label, rec, one[6])
    # not selected: the one wave's, and an empty record
    label, data, stream = B.the_rows()[0]
    rows_out, rec, ends = B.model_batch([(8, stream, len(data))], 4, min_kib=len(stream) // 1024 + 1)
    assert rows_out[0][:3] == (0, data, len(data)) and rows_out[0][5] == "not selected" and rec["streams"] == 0 and ends == []


def test_damaged_streams_in_one_table():
    """Every tenth case of the damaged corpus as ONE table: per stream the one-wave model's answer; the path takes exactly the streams the
    single-stream model takes."""
    cases, _ = _inflate.damaged_corpus()
    picked = cases[::10]
    rows_out, rec, _ = B.model_batch([(8, s, cap) for s, cap in picked], 4)
    taken = 0
    for k, (s, cap) in enumerate(picked):
        rc, out, ol, used, reg, _ = model_inflate(s, cap, 8)
        assert rows_out[k][:5] == (rc, out, ol, used, reg), k
        if len(s) >= 4096:
            one = P.model_inflate_par(s, cap, 4)[6]
            taken += not one["fell_back"]
            assert (rows_out[k][5] == "taken") == (not one["fell_back"]), (k, rows_out[k][5], one)
        else:
            assert rows_out[k][5] == "not selected", k
    assert rec["streams"] == sum(len(s) >= 4096 for s, _ in picked) and rec["streams"] - rec["fell_back"] == taken and taken > 50, (rec, taken)


def test_model_is_clean_under_asan_and_ubsan(tmp_path):
    """The stand-alone program (its own main, nothing preloaded anywhere): the small rows as one table at two bounds, the Deflate64 streams among
    Deflate ones, and every 40th damaged stream as one table, on heap buffers of exact size."""
    import _deflate64
    prog = B.build_check_program()
    cases, _ = _inflate.damaged_corpus()
    path = tmp_path / "tables.bin"
    small = [(8, s, len(d)) for _, d, s in B.the_rows() if len(d) <= 400000]
    d64 = [(9, s, len(d)) for d, s, _, _ in _deflate64.streams().values()]
    tables = [(small, 4, 0, 4, B.BATCH_MIB), (small, 4, 0, 4, 1), (small[:4] + d64, 4, 1, 4, B.BATCH_MIB), (small[:4] + d64, 16, 1, 4, 1), (small[:4] + d64, 4, 0, 4, B.BATCH_MIB),
              ([(8, s, cap) for s, cap in cases[::40]], 4, 0, 4, B.BATCH_MIB)]
    n = 0
    with open(path, "wb") as f:
        for tab, ck, knob64, min_kib, mib in tables:
            f.write(struct.pack("<6I", len(tab), ck, P.REPAIR_PCT, knob64, min_kib, mib))
            for fmt, s, cap in tab:
                f.write(struct.pack("<3I", len(s), cap, fmt) + s)
                n += 1
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and ("par batch check ok: %d tables, %d streams" % (len(tables), n)) in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
