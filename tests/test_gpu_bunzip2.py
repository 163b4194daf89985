"""The BZip2 reader on the GPU (csrc/zada_bunzip2.hip: every block in parallel) against the expected bytes, libbz2 and the CPU model of the same
decoder logic (tests/bunzip2/bunzip2_host.cpp, tested against libbz2 and under ASan + UBSan in test_bunzip2_model.py); the archive reader on top."""
import bz2
import ctypes
import hashlib
import io
import subprocess
import time
import zipfile
import zlib

import numpy as np
import pytest

import _bunzip2
import _readers
from _bunzip2 import E_DATA, model_bunzip2
from _common import product, silesia_mix

pytestmark = pytest.mark.gpu
PW = "p\xe4ss \xff"


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b) if len(b) else bytearray(1), dtype=torch.uint8).cuda()


def _device_bunzip2(enc, stream, cap, a_in=0, a_out=0, crc=0xFFFFFFFF):
    """bunzip2_device with the input at alignment a_in and the output at alignment a_out of a 256-byte aligned allocation, guard bytes on both
    sides of the output.  -> (bytes, in_used, crc register)"""
    import torch
    t_in = torch.zeros(len(stream) + 32, dtype=torch.uint8, device="cuda")
    t_in[a_in:a_in + len(stream)] = _dev(stream)[:len(stream)]
    t_out = torch.full((cap + 48,), 0xA5, dtype=torch.uint8, device="cuda")
    ol, used, reg = enc.bunzip2_device(t_in.data_ptr() + a_in, len(stream), t_out.data_ptr() + a_out, cap, crc)
    host = bytes(t_out.cpu().numpy())
    assert host[:a_out] == b"\xa5" * a_out and host[a_out + cap:] == b"\xa5" * (48 - a_out), "bytes outside the output buffer were written"
    assert ol <= cap
    return host[a_out:a_out + ol], used, reg


def _guarded_batch(enc, streams, caps):
    """zada_bunzip2_batch with 16 guard bytes behind every output buffer -> (rcs, out_lens, in_useds, crcs, outputs); asserts the guards."""
    cnt = len(streams)
    lens = np.array([len(s) for s in streams], dtype=np.uint64)
    caps = np.array(caps, dtype=np.uint64)
    keep = [s if len(s) else b"\0" for s in streams]
    ins = np.array([ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p).value for s in keep], dtype=np.uint64)
    offs = np.concatenate(([0], np.cumsum(caps + 16)[:-1])).astype(np.uint64)
    arena = np.full(int((caps + 16).sum()), 0xA5, dtype=np.uint8)
    outp = (arena.ctypes.data + offs).astype(np.uint64)
    ols, ius = np.zeros(cnt, np.uint64), np.zeros(cnt, np.uint64)
    crcs = np.full(cnt, 0xFFFFFFFF, dtype=np.uint32)
    rcs = np.full(cnt, 99, dtype=np.int32)
    worst = enc.lib.zada_bunzip2_batch(enc.ctx, cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data, caps.ctypes.data, ols.ctypes.data, ius.ctypes.data,
                                       crcs.ctypes.data, rcs.ctypes.data)
    assert worst in (0, E_DATA), (worst, enc.lib.zada_last_error(enc.ctx))
    outs = []
    for k in range(cnt):
        o, cap = int(offs[k]), int(caps[k])
        assert arena[o + cap:o + cap + 16].tobytes() == b"\xa5" * 16, k
        outs.append(arena[o:o + int(ols[k])].tobytes() if rcs[k] == 0 else None)
    return rcs, ols, ius, crcs, outs


@pytest.fixture(scope="module")
def streams(encoder):
    """(label, data, stream): every input of the CPU test through bz2.compress at levels 1 and 9 and through the product's BZip2_1 / _2 / _3 (bit for
    bit the oracle's streams, test_gpu_bzip2.py -- made here on the GPU), the three-block stream and the reference's own payload."""
    out = []
    for label, data, s in _bunzip2.valid_streams(product_encoder=encoder):
        out.append((label, data if data is not None else bz2.decompress(s), s))
    return out


def test_valid_streams_batch(encoder, streams):
    assert len(streams) > 350
    got = encoder.bunzip2_batch([s for _, _, s in streams], [len(d) for _, d, _ in streams])
    for (label, data, stream), (rc, out, ol, used, reg) in zip(streams, got):
        assert rc == 0 and out == data and ol == len(data), label
        assert used == len(stream) and reg ^ 0xFFFFFFFF == zlib.crc32(data), label
    # trailing bytes and a larger cap change nothing
    some = streams[::7]
    got = encoder.bunzip2_batch([s + b"\x55\x00\xaa" for _, _, s in some], [len(d) + 5 for _, d, _ in some])
    for (label, data, stream), (rc, out, ol, used, reg) in zip(some, got):
        assert (rc, out, used) == (0, data, len(stream)), label
    # one byte less of cap for every eleventh stream: E_DATA for that entry alone, the guard bytes behind every buffer untouched
    some = [x for x in streams if len(x[1])]
    caps = [len(d) - (1 if i % 11 == 0 else 0) for i, (_, d, _) in enumerate(some)]
    rcs, ols, ius, crcs, outs = _guarded_batch(encoder, [s for _, _, s in some], caps)
    rules = encoder.bunzip2_last_records()
    for i, (label, data, stream) in enumerate(some):
        if i % 11 == 0:
            assert rcs[i] == E_DATA and ols[i] == 0 and ius[i] == 0 and int(rules[i, 0]) == 19, label          # BZD_R_OUTPUT_FULL
        else:
            assert rcs[i] == 0 and outs[i] == data, label


def test_valid_streams_single(encoder, streams):
    """The single call on host buffers; size unknown and one byte less of cap for every eleventh stream."""
    za = product()
    for k, (label, data, stream) in enumerate(streams):
        assert encoder.bunzip2(stream, len(data)) == (data, len(stream), zlib.crc32(data) ^ 0xFFFFFFFF), label
        if k % 11:
            continue
        assert encoder.bunzip2(stream)[0] == data, label
        if len(data):
            with pytest.raises(za.DataError):
                encoder.bunzip2(stream, len(data) - 1)
    with pytest.raises(za.DataError):
        encoder.bunzip2(b"", 10)
    assert encoder.bunzip2(bz2.compress(b""), 0) == (b"", 14, 0xFFFFFFFF)
    assert encoder.bunzip2_batch([], []) == []


def test_valid_streams_device(encoder, streams):
    """Device pointers: the alignments of input and output rotate over all sixteen each from stream to stream."""
    for k, (label, data, stream) in enumerate(streams):
        out, used, reg = _device_bunzip2(encoder, stream, len(data), k % 16, (k // 16) % 16)
        assert out == data and used == len(stream) and reg ^ 0xFFFFFFFF == zlib.crc32(data), (label, k)


def test_reference_payload_and_the_empty_block(encoder):
    p, size, crc, sha = _bunzip2.reference_payload()
    out, used, reg = encoder.bunzip2(p, size)
    assert len(out) == size and used == len(p) and hashlib.sha256(out).hexdigest() == sha and reg ^ 0xFFFFFFFF == crc
    # what the three BZip2 methods write for no bytes holds a block of no symbols: refused as libbz2 refuses it, on the GPU as in the model
    for m in (12, 13, 14):
        rc, s, _ = encoder.bzip2(b"", m)
        assert rc in (0, 1) and s in _bunzip2.empty_block_streams()
        got = encoder.bunzip2_batch([s], [0])
        assert got[0][0] == E_DATA and int(encoder.bunzip2_last_records()[0, 0]) == 5                           # BZD_R_NO_BYTE_IN_USE


DAMAGED_TIME_LIMIT = 600          # seconds for the child process of the damaged corpus


def test_damaged_corpus_equals_the_cpu_model():
    """20 000 damaged streams in ONE zada_bunzip2_batch call: rc, rule, bytes written, input used and the bytes themselves equal the CPU model's
    for every entry (the model follows libbz2: test_bunzip2_model.py), and the 16 guard bytes behind every output buffer are untouched.  It runs
    once, in a child process of its own under its own time limit, and nothing here runs it again if it fails."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import test_gpu_bunzip2 as t; t._damaged_corpus_main()" % here
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=DAMAGED_TIME_LIMIT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "damaged corpus ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _damaged_corpus_main():
    za = product()
    encoder = za.Encoder(0)
    cases, _ = _bunzip2.damaged_corpus()
    assert len(cases) == 20000
    t0 = time.time()
    rcs, ols, ius, crcs, outs = _guarded_batch(encoder, [s for s, _, _ in cases], [c for _, c, _ in cases])
    print("damaged corpus: %.2f s (%s)" % (time.time() - t0, encoder.lib.zada_last_error(encoder.ctx).decode()))
    rules = encoder.bunzip2_last_records()
    M = _bunzip2.model()
    n_ok = 0
    for k, (s, cap, kind) in enumerate(cases):
        rc, out, ol, used, reg, rule = model_bunzip2(s, cap)
        got_rule = M.bm_rule_name(int(rules[k, 0])).decode()
        assert (int(rcs[k]), got_rule, int(ols[k]), int(ius[k])) == (rc, rule, ol, used), (k, kind, rule, got_rule, int(rules[k, 1]), int(rules[k, 2]))
        if rc == 0:
            assert outs[k] == out and int(crcs[k]) == reg, k
            n_ok += 1
    print("accepted", n_ok)
    # the same on device buffers, one entry per call, guard bytes in device memory on both sides of the output
    for k in range(0, len(cases), 197):
        s, cap, _ = cases[k]
        rc, out, ol, used, reg, _ = model_bunzip2(s, cap)
        if rc == 0:
            assert _device_bunzip2(encoder, s, cap, k % 16, (k // 16) % 16) == (out, used, reg), k
        elif len(s):
            try:
                _device_bunzip2(encoder, s, cap, k % 16, (k // 16) % 16)
            except za.DataError:
                pass
            else:
                raise AssertionError("entry %d: the device call accepted what the model refuses" % k)
    # what zada.h promises a C caller for such an entry: *out_len = *in_used = 0, the CRC register as it was
    import torch
    s, cap, _ = next(c for c in cases if len(c[0]) > 100)
    t_in, t_out = _dev(s), torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    ol, iu, reg = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(0x1234)
    assert encoder.lib.zada_bunzip2_device(encoder.ctx, t_in.data_ptr(), len(s), t_out.data_ptr(), cap, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg)) == E_DATA
    assert (ol.value, iu.value, reg.value) == (0, 0, 0x1234)
    assert b"bunzip2: entry 0: " in encoder.lib.zada_last_error(encoder.ctx) and b" in block " in encoder.lib.zada_last_error(encoder.ctx)
    # sizes no device holds are refused before anything is sized from them
    assert encoder.lib.zada_bunzip2_device(encoder.ctx, t_in.data_ptr(), len(s), t_out.data_ptr(), (1 << 64) - 8, None, None, None) == -4
    assert encoder.lib.zada_bunzip2_device(encoder.ctx, None, 5, t_out.data_ptr(), 5, None, None, None) == -1
    try:
        encoder.bunzip2_batch([s, s], [(1 << 64) - 8, 40])
    except za.ZadaError:
        pass
    else:
        raise AssertionError("a cap near 2 ** 64 was taken")
    encoder.close()
    print("damaged corpus ok")


def test_crafted_streams_alone_and_as_neighbours(encoder):
    M = _bunzip2.model()
    cases = _bunzip2.crafted_cases()
    names = list(cases)
    for name in names:
        stream, expect, rule = cases[name]
        got = encoder.bunzip2_batch([stream], [1 << 20])[0]
        rec = encoder.bunzip2_last_records()
        if expect is None:
            assert got[0] == E_DATA and M.bm_rule_name(int(rec[0, 0])).decode() == rule, name
        else:
            assert got[0] == 0 and got[1] == expect and got[3] == model_bunzip2(stream, 1 << 20)[3], name
    # as neighbours in one arena, caps exact: the scan of one entry does not see its neighbour's bytes.  Between them, two entries cut in
    # the middle of a magic whose other half begins the next entry
    s0, e0, _ = cases["c_magic_behind_footer"]
    half = _bunzip2.BLOCK_MAGIC.to_bytes(6, "big")
    extra = [(s0 + half[:3], e0), (half[3:] + s0, None), (cases["a_cycles"][0][:-3] + half[:3], None)]
    batch = [(cases[n][0], cases[n][1]) for n in names] + extra + [(cases[n][0], cases[n][1]) for n in reversed(names)]
    rcs, ols, ius, crcs, outs = _guarded_batch(encoder, [s for s, _ in batch], [len(e) if e is not None else 4096 for _, e in batch])
    for k, (s, e) in enumerate(batch):
        m = model_bunzip2(s, len(e) if e is not None else 4096)
        assert (int(rcs[k]), outs[k], int(ius[k])) == (m[0], m[1] if m[0] == 0 else None, m[3]), k
        assert (rcs[k] == 0) == (e is not None) and (e is None or outs[k] == e), k
    # the false magic of (b) was a candidate that the chain never reached: one block in the chain
    s, exp, at = _bunzip2.magic_inside_block(3)
    assert encoder.bunzip2(s, len(exp))[0] == exp
    assert len(encoder.bunzip2_last_records(blocks=True)) == 1


@pytest.fixture(scope="module")
def mix2():
    return silesia_mix(4 << 20, version=2)


def test_two_full_level9_blocks_on_device(encoder, mix2):
    """1.9 MB at level 9: two blocks of 900 000 bytes and a short one -- the at-size slot and the walk over 14 000 splitters per block."""
    import torch
    d = mix2[:1900000]
    s = bz2.compress(d, 9)
    t_in, t_out = _dev(s), torch.full((len(d) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    t0 = time.time()
    ol, used, reg = encoder.bunzip2_device(t_in.data_ptr(), len(s), t_out.data_ptr(), len(d))
    print("1.9 MB, three blocks: %.3f s" % (time.time() - t0))
    assert (ol, used) == (len(d), len(s)) and reg ^ 0xFFFFFFFF == zlib.crc32(d)
    host = bytes(t_out.cpu().numpy())
    assert host[:len(d)] == d and host[len(d):] == b"\xa5" * 16
    blocks = encoder.bunzip2_last_records(blocks=True)
    assert len(blocks) == 3 and int(blocks[0, 1]) >= 900000 - 19 and int(blocks[1, 1]) >= 900000 - 19
    want = model_bunzip2(s, len(d), records=8)[6]
    assert [tuple(int(x) for x in b[1:]) for b in blocks] == [tuple(int(x) for x in w) for w in want]


def test_forty_small_blocks_of_the_splitter(encoder):
    """One BZip2_3 stream whose blocks the writer's splitting tactics cut small: the input, and the model's per-block records."""
    rng = np.random.default_rng(12)
    parts = []
    for j in range(26):
        k = int(rng.choice([2, 3, 4, 6, 8, 12, 16, 24, 26]))
        parts.append(rng.integers([48, 65, 97][j % 3], [48, 65, 97][j % 3] + k, int(rng.integers(30000, 60000)), dtype=np.uint8))
    d = bytes(np.concatenate(parts))
    rc, s, crc = encoder.bzip2(d, 14)
    assert rc == 0
    out, used, reg = encoder.bunzip2(s, len(d))
    assert out == d and used == len(s) and reg == crc
    blocks = encoder.bunzip2_last_records(blocks=True)
    print("blocks:", len(blocks))
    assert len(blocks) >= 30
    want = model_bunzip2(s, len(d), records=256)[6]
    assert [tuple(int(x) for x in b[1:]) for b in blocks] == [tuple(int(x) for x in w) for w in want]


@pytest.mark.parametrize("method", (12, 13, 14))
def test_round_trip_of_small_entries(encoder, mix2, method):
    rng = np.random.default_rng(method)
    datas, off = [], 0
    for ln in rng.integers(0, 40001, 2000):
        datas.append(mix2[off % (3 << 20):off % (3 << 20) + int(ln)]); off += int(ln)
    t0 = time.time()
    packed = encoder.bzip2_batch(datas, method)
    t1 = time.time()
    comp = [i for i, p in enumerate(packed) if p[0] in (0, 1) and p[1] is not None and len(datas[i])]
    got = encoder.bunzip2_batch([packed[i][1] for i in comp], [len(datas[i]) for i in comp])
    t2 = time.time()
    print("method %d: %d entries, bzip2_batch %.2f s, bunzip2_batch %.2f s" % (method, len(comp), t1 - t0, t2 - t1))
    assert len(comp) > len(datas) * 0.9
    for i, (rc, out, ol, used, reg) in zip(comp, got):
        assert rc == 0 and out == datas[i] and used == len(packed[i][1]) and reg == packed[i][2], i
    # test_only: verdicts, sizes and CRCs without bytes
    got = encoder.bunzip2_batch([packed[i][1] for i in comp[:300]], [len(datas[i]) for i in comp[:300]], deliver=False)
    for i, (rc, out, ol, used, reg) in zip(comp, got):
        assert (rc, out, ol, reg) == (0, None, len(datas[i]), packed[i][2]), i


def _entries(mix2):
    return [("a/text.txt", silesia_mix(200000, class_mask=1)), ("b/rand.bin", bytes(np.random.RandomState(3).randint(0, 256, 3000).astype(np.uint8))),
            ("empty", b""), ("mix.bin", mix2[:1200000]), ("one", b"z"), ("c/ümlaut.txt", b"abc" * 5000), ("photo.jpg", _bunzip2.golden("sample.jpg"))]


def _check_archive(encoder, archive, entries, password=None):
    za = product()
    info = za.ZipInfo.load(archive)
    uz = za.UnZip(encoder, bzip2=True)
    want = dict(entries)
    assert uz.extract(info, password=password) == want
    assert uz.extract(info, password=password, test_only=True) == {nm: None for nm in want}
    assert uz.extract(info, what=[entries[3][0], entries[0][0]], password=password) == {entries[3][0]: entries[3][1], entries[0][0]: entries[0][1]}
    return info


@pytest.mark.parametrize("password", (None, PW))
def test_archives_of_the_writer(encoder, mix2, password):
    za = product()
    entries = _entries(mix2)
    zc = za.ZipCreate(encoder, za.Method.BZip2_3)
    zc.add_streams([e[0] for e in entries], [e[1] for e in entries], password=password)
    arc = zc.finish()
    info = _check_archive(encoder, arc, entries, password)
    assert 12 in {e.method for e in info.entries} and {e.method for e in info.entries} <= {0, 12}
    assert all(e.encrypted == (password is not None) for e in info.entries)
    # the default reader still leaves these entries alone, with the words it always had
    got = za.UnZip(encoder).extract(info, password=password, errors="collect")
    for e in info.entries:
        if e.method == 12:
            assert isinstance(got[e.name], za.UnsupportedMethod) and "BZip2" in str(got[e.name]) and "out of scope" in str(got[e.name])
        else:
            assert got[e.name] == dict(entries)[e.name]


def test_archive_of_zipfile_and_what_the_reader_refuses(encoder, mix2):
    za = product()
    entries = _entries(mix2)
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w", zipfile.ZIP_BZIP2) as z:
        for nm, d in entries:
            z.writestr(nm, d)
        z.writestr(zipfile.ZipInfo("deflated.txt"), entries[0][1], compress_type=zipfile.ZIP_DEFLATED)
        z.writestr(zipfile.ZipInfo("lzma.bin"), entries[5][1], compress_type=zipfile.ZIP_LZMA)
    arc = b.getvalue()
    info = za.ZipInfo.load(arc)
    uz = za.UnZip(encoder, bzip2=True)
    got = uz.extract(info, errors="collect")
    assert {k: v for k, v in got.items() if k not in ("deflated.txt", "lzma.bin")} == dict(entries) and got["deflated.txt"] == entries[0][1]
    assert isinstance(got["lzma.bin"], za.UnsupportedMethod) and "LZMA" in str(got["lzma.bin"])
    # one flipped payload byte: DataError, CRCError or SizeError for that entry only
    for name, at in (("mix.bin", 100000), ("a/text.txt", 30), ("photo.jpg", 40000), ("mix.bin", 2)):
        e = info[name]
        assert e.method == 12
        bad = bytearray(arc)
        bad[e.data_offset + min(at, e.csize - 1)] ^= 0x10
        got = uz.extract(za.ZipInfo.load(bytes(bad)), errors="collect")
        assert isinstance(got[name], (za.CRCError, za.DataError, za.SizeError)), name
        assert {k: v for k, v in got.items() if k not in (name, "lzma.bin")} == {k: v for k, v in list(entries) + [("deflated.txt", entries[0][1])] if k != name}
        t = uz.extract(za.ZipInfo.load(bytes(bad)), test_only=True)
        assert isinstance(t[name], za.ZadaError) and all(x is None for k, x in t.items() if k not in (name, "lzma.bin"))
    with pytest.raises(za.UnsupportedMethod):
        za.UnZip(encoder).extract(za.ZipInfo.load(arc), what="one")


def test_argument_checks_come_first(encoder):
    _readers.argument_checks(encoder, "bunzip2")


def test_several_launch_groups(encoder):
    """bunzip_batch_mib = 16 (8 MiB of streams and outputs per group): the entries go through several groups; bz2 says what every entry holds."""
    _readers.several_launch_groups(encoder, "bunzip2")
