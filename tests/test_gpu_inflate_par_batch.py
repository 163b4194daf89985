"""The batched parallel Inflate (the knob "inflate_par_batch": the large entries of one zada_unzip_device group in the same launches) through
Encoder.unzip_device on raw "archives" of hand-made rows (_inflate_par_batch.run_table: outputs at every alignment, adjacent or a few guard bytes
apart, a CRC register per row) and through UnZip / FindZip / CompZip: against zlib, against the same call with the knob at 0 and against the CPU
models, the record asserted next to the bytes."""
import io
import os
import subprocess
import sys
import zipfile
import zlib

import numpy as np
import pytest

import _inflate
import _inflate_par as P
import _inflate_par_batch as B
from _common import product, silesia_mix
from _inflate import E_DATA, model_inflate

pytestmark = pytest.mark.gpu
PW = "p\xe4ss \xff"
KNOBS = {"inflate_par_chunk_kib": 64, "inflate_par_repair_pct": P.REPAIR_PCT, "inflate_par_min_kib": 0, "inflate_par_deflate64": 0, "inflate_par_batch": 0,
         "inflate_par_batch_mib": B.BATCH_MIB}


def _reset(enc):
    for k, v in KNOBS.items():
        enc.set_knob(k, v)


@pytest.fixture()
def par(encoder):
    """The session's encoder with the knobs of the parallel path at their defaults before and after."""
    _reset(encoder)
    yield encoder
    _reset(encoder)


def _knobs(enc, **kw):
    for k, v in kw.items():
        enc.set_knob("inflate_par_" + k, v)


def _but_rounds(rec):
    return {k: v for k, v in rec.items() if k != "scout_rounds"}


def test_knobs_and_keyword(par):
    za = product()
    par.set_knob("inflate_par_batch", 1)
    par.set_knob("inflate_par_batch_mib", 1)
    for name, bad in (("inflate_par_batch", 2), ("inflate_par_batch", -1), ("inflate_par_batch_mib", 0), ("inflate_par_batch_mib", 1048577)):
        with pytest.raises(za.ZadaError):
            par.set_knob(name, bad)
    par.set_knob("inflate_par_batch_mib", 1048576)
    with pytest.raises(za.ZadaError):
        za.UnZip(par, parallel_batch=True)
    assert za.UnZip(par, parallel_inflate=64, parallel_batch=True).parallel_batch is True


def _check_rows(table, datas, res, host, offs, starts, label):
    for k, ((method, stream, _), data) in enumerate(zip(table, datas)):
        used = _inflate.zlib_in_used(stream) if method == 8 else len(stream)          # (zlib reads no Deflate64)
        assert (int(res["rc"][k]), int(res["out_len"][k]), int(res["in_used"][k])) == (0, len(data), used), (label, k)
        assert B.row_bytes(host, offs, res, k) == data, (label, k)
        assert int(res["crc"][k]) == zlib.crc32(data, starts[k] ^ 0xFFFFFFFF) ^ 0xFFFFFFFF, (label, k)


def _rows_table():
    rows = B.the_rows()
    return [(8, s, len(d)) for _, d, s in rows], [d for _, d, _ in rows]


def test_the_rows_in_one_call_both_ways(par):
    table, datas = _rows_table()
    offs, total = B.layout([cap for _, _, cap in table])
    gaps = [offs[k + 1] - offs[k] - table[k][2] for k in range(19)]
    assert {o % 16 for o in offs} == set(range(16)) and 0 in gaps and max(gaps) < 16, gaps
    starts = [int(x) for x in np.random.default_rng(3).integers(0, 1 << 32, 20)]
    _knobs(par, chunk_kib=4, min_kib=4)
    recs = {}
    for knob in (0, 1):
        par.set_knob("inflate_par_batch", knob)
        rc, res, host, offs2 = B.run_table(par, table, starts, (offs, total))
        recs[knob] = par.inflate_par_last()
        print("inflate_par_batch =", knob, recs[knob])
        assert rc == 0
        _check_rows(table, datas, res, host, offs2, starts, knob)
    assert _but_rounds(recs[0]) == _but_rounds(recs[1])
    assert recs[0] == B.sum_records([r[6] for r in B.single_records()]) and recs[0]["scout_rounds"] == 139
    assert recs[1] == B.rows_model()[1] and recs[1]["scout_rounds"] == 64
    assert recs[1]["streams"] == 20 and recs[1]["fell_back"] == 3 and recs[1]["reason"] == "single chunk"


def test_the_rows_in_passes_of_one_mib(par):
    table, datas = _rows_table()
    _knobs(par, chunk_kib=4, min_kib=4, batch=1, batch_mib=1)
    rc, res, host, offs = B.run_table(par, table)
    rec = par.inflate_par_last()
    assert rc == 0
    _check_rows(table, datas, res, host, offs, [B.START] * 20, "1 MiB")
    assert rec == B.rows_model(1)[1] and rec["scout_rounds"] > 64, rec


def test_six_hundred_rows(par):
    """300 copies of one stream of about 20 chunks interleaved with 300 rows below "inflate_par_min_kib": the stream and live tables beyond 256 rows;
    every copy needs its one repair in the same round."""
    data = _inflate.golden("sample_pgm_100k.bin")
    stream = _inflate.zlib_raw(data, 6, zlib.Z_DEFAULT_STRATEGY)
    one = P.model_inflate_par(stream, len(data), 4)[6]
    assert one["repairs"] == 1 and one["fell_back"] == 0
    small = [silesia_mix(900 + 7 * k, class_mask=1, offset=1000 * k) for k in range(300)]
    table, datas = [], []
    for k in range(300):
        table += [(8, stream, len(data)), (8, _inflate.zlib_raw(small[k], 6, zlib.Z_DEFAULT_STRATEGY), len(small[k]))]
        datas += [data, small[k]]
    assert all(len(s) < 4096 for _, s, _ in table[1::2])
    _knobs(par, chunk_kib=4, min_kib=4, batch=1)
    rc, res, host, offs = B.run_table(par, table)
    rec = par.inflate_par_last()
    assert rc == 0
    _check_rows(table, datas, res, host, offs, [B.START] * 600, "600")
    assert rec["streams"] == 300 and rec["fell_back"] == 0 and rec["scout_rounds"] == 2 and rec["repairs"] == 300, rec
    assert rec["live_chunks"] == 300 * one["live_chunks"] and rec["marker_bytes"] == 300 * one["marker_bytes"], (rec, one)


def test_caps_and_damage_inside_a_batch(par):
    """A cap one byte short, an exact one and a flipped payload bit in one group.  The rows the path hands over are judged by the one-wave batch, as
    with the knobs off -- and that decoder writes what it decoded before it met the damage into the row's range, with the knobs off as well.  So
    "nothing was written to a failed row's range" is asserted in the form that can hold: the whole output buffer, failed rows' ranges included, is
    byte for byte what the call with "inflate_par_min_kib" = 0 leaves (had the path finished a stream before it found the damage, its bytes would
    lie behind the one wave's), and no byte outside the rows' ranges changed (run_table)."""
    label, data, stream = next(r for r in B.the_rows() if r[0] == "corpus_2m/zlib6")
    table = [(8, stream, len(data) - 1), (8, stream, len(data)), (8, B.flip(stream, len(data), refused=True), len(data))]
    starts = [0x12345678, 0x9ABCDEF0, 0x0F1E2D3C]
    _knobs(par, chunk_kib=4)
    rc0, want, host0, offs = B.run_table(par, table, starts)
    text0 = par.lib.zada_last_error(par.ctx).decode()
    _knobs(par, min_kib=4, batch=1)
    rc1, got, host1, _ = B.run_table(par, table, starts)
    text1 = par.lib.zada_last_error(par.ctx).decode()
    rec = par.inflate_par_last()
    assert rc0 == rc1 == E_DATA and text0 == text1 and text0
    for f in ("rc", "out_len", "in_used", "crc"):
        assert list(got[f]) == list(want[f]), (f, got, want)
    assert int(got["rc"][0]) == E_DATA and int(got["rc"][1]) == 0 and int(got["rc"][2]) == E_DATA and int(got["crc"][0]) == starts[0] and int(got["crc"][2]) == starts[2]
    assert B.row_bytes(host1, offs, got, 1) == data and int(got["crc"][1]) == zlib.crc32(data, starts[1] ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
    assert np.array_equal(host0, host1)
    assert int(got["out_len"][0]) == 0 and int(got["out_len"][2]) == 0
    assert rec["streams"] == 3 and rec["fell_back"] == 2 and rec["reason"] == "damaged", rec


@pytest.mark.parametrize("chunk_kib", (4, 16))
def test_deflate64_in_the_same_group(par, chunk_kib):
    import _deflate64
    d64 = list(_deflate64.streams().values())
    rows = B.the_rows()[:4]
    table, datas = [], []
    for k in range(4):
        table += [(9, d64[k][1], len(d64[k][0])), (8, rows[k][2], len(rows[k][1]))]
        datas += [d64[k][0], rows[k][1]]
    _knobs(par, chunk_kib=chunk_kib)
    rc0, want, host0, offs = B.run_table(par, table)
    assert rc0 == 0
    _check_rows(table, datas, want, host0, offs, [B.START] * 8, "one wave")
    _knobs(par, min_kib=4, batch=1, deflate64=1)
    rc1, got, host1, _ = B.run_table(par, table)
    rec = par.inflate_par_last()
    assert rc1 == 0 and got.tobytes() == want.tobytes() and np.array_equal(host0, host1)
    model = B.model_batch(table, chunk_kib, deflate64=1)[1]
    assert rec == model and rec["streams"] == 8 and rec["streams"] - rec["fell_back"] >= 5, (rec, model)
    _knobs(par, deflate64=0)
    rc2, got2, host2, _ = B.run_table(par, table)
    rec2 = par.inflate_par_last()
    assert rc2 == 0 and got2.tobytes() == want.tobytes() and np.array_equal(host0, host2)
    assert rec2 == B.model_batch(table, chunk_kib, deflate64=0)[1] and rec2["streams"] == 4, rec2


DAMAGED_TIME_LIMIT = 300          # seconds for the child process of the damaged streams


def test_damaged_streams_in_one_call_equal_the_cpu_model():
    """Every tenth case of the damaged corpus at 4 KiB chunks as ONE table in ONE call: rc, bytes written, input used and CRC per row equal the CPU
    model's of the one-wave decoder, the path takes as many streams as its CPU model and no byte outside the delivered ranges changes.  An error-path
    test on inputs the same logic has survived on a CPU under ASan + UBSan; it runs once, in a child process of its own under its own time limit, and
    nothing here runs it again if it fails."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import test_gpu_inflate_par_batch as t; t._damaged_main()" % here
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=DAMAGED_TIME_LIMIT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "damaged table ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _damaged_main():
    za = product()
    enc = za.Encoder(0)
    _knobs(enc, chunk_kib=4, min_kib=4, batch=1)
    cases, _ = _inflate.damaged_corpus()
    table = [(8, s, cap) for s, cap in cases[::10]]
    _, model_rec, _ = B.model_batch(table, 4)
    rc, res, host, offs = B.run_table(enc, table)
    rec = enc.inflate_par_last()
    n_ok = 0
    for k, (_, s, cap) in enumerate(table):
        mrc, out, ol, used, reg, rule = model_inflate(s, cap, 8)
        got = (int(res["rc"][k]), B.row_bytes(host, offs, res, k), int(res["out_len"][k]), int(res["in_used"][k]), int(res["crc"][k]))
        assert got == (mrc, out, ol, used, reg if mrc == 0 else 0xFFFFFFFF), (k, rule, got[0], got[2:], (mrc, ol, used))
        n_ok += mrc == 0
    assert rc == E_DATA and n_ok > 100
    assert rec == model_rec and rec["streams"] - rec["fell_back"] > 50, (rec, model_rec)
    enc.close()
    print("damaged table ok: %d rows, %d accepted, %d of %d large ones in parallel" % (len(table), n_ok, rec["streams"] - rec["fell_back"], rec["streams"]))


def _archive(par, writer):
    """The archive of test_gpu_inflate_par.test_unzip_with_parallel_inflate: a 3 MiB Deflate entry, twenty small ones, a stored one, a large encrypted
    one (ZipCreate only) and a large one with a flipped payload bit."""
    za = product()
    mix = silesia_mix(5 << 20, version=2)
    ents = [("big/three_mib.bin", mix[:3 << 20])]
    ents += [("small/%02d.txt" % i, mix[(3 << 20) + i * 5000:(3 << 20) + i * 5000 + 300 + 233 * i]) for i in range(20)]
    ents += [("big/secret.bin", mix[3 << 20:4 << 20]), ("big/damaged.bin", mix[4 << 20:5 << 20])]
    stored = ("stored.bin", mix[1000:41000])
    if writer == "ZipCreate":
        zc = za.ZipCreate(par, za.Method.Deflate_3)
        for nm, d in ents:
            zc.add_stream(nm, d, password=PW if nm == "big/secret.bin" else None)
        zc.add_compressed(stored[0], stored[1], zlib.crc32(stored[1]), len(stored[1]), 0)
        arc = zc.finish()
    else:
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w", zipfile.ZIP_DEFLATED) as z:
            for nm, d in ents:
                z.writestr(nm, d)
            z.writestr(zipfile.ZipInfo(stored[0]), stored[1], compress_type=zipfile.ZIP_STORED)
        arc = b.getvalue()
    e = za.ZipInfo.load(arc)["big/damaged.bin"]
    bad = B.flip(arc[e.data_offset:e.data_offset + e.csize], e.usize)
    return arc[:e.data_offset] + bad + arc[e.data_offset + e.csize:]


def _plain(x):
    """A result with its exceptions as (type, text) and its tensors as bytes, to compare two of them."""
    if isinstance(x, Exception):
        return (type(x).__name__, str(x))
    if isinstance(x, (tuple, list)):
        return tuple(_plain(y) for y in x)
    if hasattr(x, "cpu"):
        return bytes(x.cpu().numpy())
    return x


@pytest.mark.parametrize("writer", ("ZipCreate", "zipfile"))
def test_archives(par, writer):
    import torch
    za = product()
    arc = _archive(par, writer)
    t = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).cuda()
    dinfo = za.ZipInfo.load_device(t)
    want = za.UnZip(par).extract_device(dinfo, password=PW, errors="collect")
    assert type(want["big/damaged.bin"]) in (za.CRCError, za.DataError) and not isinstance(want["big/three_mib.bin"], Exception)
    par.set_knob("inflate_par_batch_mib", 77)                   # (not a value the reader sets: it has to survive the calls)
    fast = za.UnZip(par, parallel_inflate=64, parallel_batch=True)
    got = fast.extract_device(dinfo, password=PW, errors="collect")
    assert list(got) == list(want) and {k: _plain(v) for k, v in got.items()} == {k: _plain(v) for k, v in want.items()}
    rec = par.inflate_par_last()
    assert rec["streams"] == 3 and rec["fell_back"] <= 1 and rec["live_chunks"] >= 4 and rec["scout_rounds"] >= 1, rec
    assert par._knobs_set["inflate_par_batch"] == 0 and par._knobs_set["inflate_par_min_kib"] == 0 and par._knobs_set["inflate_par_batch_mib"] == 77
    with pytest.raises(type(want["big/damaged.bin"])) as a:
        fast.extract_device(dinfo, password=PW)
    assert str(a.value) == str(want["big/damaged.bin"]) and par._knobs_set["inflate_par_batch"] == 0
    # a caller's own setting comes back too
    par.set_knob("inflate_par_batch", 1)
    fast.extract_device(dinfo, password=PW, errors="collect")
    assert par._knobs_set["inflate_par_batch"] == 1
    par.set_knob("inflate_par_batch", 0)
    za.UnZip(par).extract_device(dinfo, password=PW, errors="collect")
    assert par.inflate_par_last() == rec                       # the default reader never took the path
    # Find_Zip and Comp_Zip run on zada_unzip_device: the knobs on the encoder
    text = arc[za.ZipInfo.load(arc)["stored.bin"].data_offset + 100:][:12]
    f0 = za.FindZip(par).find_device(dinfo, text, password=PW)
    c0 = za.CompZip(par).compare_device(dinfo, dinfo, password=PW)
    _knobs(par, min_kib=64, batch=1)
    f1 = za.FindZip(par).find_device(dinfo, text, password=PW)
    assert par.inflate_par_last()["streams"] == 3
    c1 = za.CompZip(par).compare_device(dinfo, dinfo, password=PW)
    assert par.inflate_par_last()["streams"] == 3
    assert _plain(f1.entries) == _plain(f0.entries) and f1.in_contents == f0.in_contents and f1.damaged == f0.damaged >= 1 and len(f0.in_contents) >= 1
    assert _plain(c1.entries) == _plain(c0.entries) and repr(c1) == repr(c0) and c0.damaged >= 1


def test_eight_entries_at_size(par):
    """Eight entries of 4 MiB, written on the device with Deflate_3 and read back at the default chunk size, batched: the bytes, and no more scout
    launches than the neediest entry asks for when it runs alone."""
    import torch
    za = product()
    mix = silesia_mix(32 << 20, version=2)
    tensors = [torch.from_numpy(np.frombuffer(mix[k << 22:(k + 1) << 22], dtype=np.uint8).copy()).cuda() for k in range(8)]
    arc = za.ZipCreate(par, za.Method.Deflate_3).write_device(["e%d.bin" % k for k in range(8)], tensors).clone()
    dinfo = za.ZipInfo.load_device(arc)
    assert all(e.method == 8 and e.csize >= 64 << 10 for e in dinfo.entries)
    got = za.UnZip(par, parallel_inflate=64, parallel_batch=True).extract_device(dinfo)
    rec = par.inflate_par_last()
    for k in range(8):
        assert torch.equal(got["e%d.bin" % k], tensors[k]), k
    assert rec["streams"] == 8 and rec["fell_back"] == 0, rec
    out = torch.empty(4 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    repairs = []
    for e in dinfo.entries:
        assert par.inflate_par_device(arc.data_ptr() + e.data_offset, e.csize, out.data_ptr(), e.usize)[0] == e.usize
        one = par.inflate_par_last()
        assert one["fell_back"] == 0
        repairs.append(one["repairs"])
    assert rec["repairs"] == sum(repairs) and rec["scout_rounds"] <= 1 + max(repairs), (rec, repairs)
