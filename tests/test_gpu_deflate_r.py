"""GPU tests of Deflate_R (LZ77.Rich front end, csrc/zada_rich.hip): tokens, streams, CRC, block trace and every entry
point against the CPU model (tests/rich/rich_model.c) and the oracle's entropy stage fed the model's tokens."""
import io
import zipfile
import zlib

import numpy as np
import pytest

import _rich
from _common import oracle_zip_compressed, product, silesia_mix
from test_rich_model import all_cases

pytestmark = pytest.mark.gpu

R = 11          # Method.Deflate_R


def crc_reg(d):
    return zlib.crc32(d) ^ 0xFFFFFFFF


def expect(d, toks=None):
    """(rc, stream, block trace) the reference writes for Deflate_R on d."""
    blocks = []
    rc, s = _rich.deflate_r(d, toks, blocks)
    return rc, s, blocks


def gpu(enc, d):
    out = bytearray(len(d) + 64)
    rc, ol, crc = enc.deflate_into(d, out, R)
    return rc, bytes(out[:ol]) if rc == 0 else b"", crc


@pytest.fixture(scope="module")
def cases():
    return all_cases()


def test_tokens_equal_the_model(encoder, cases):
    for name, d in cases.items():
        a = _rich.tokens(d)
        b = encoder.lz77_tokens(d, R)
        assert len(a) == len(b) and (a == b).all(), name


def test_streams_crc_and_blocks_equal_the_reference(encoder, cases):
    for name, d in cases.items():
        rc, ref, ob = expect(d)
        rc2, out, crc2 = gpu(encoder, d)
        assert rc == rc2, name
        assert crc2 == crc_reg(d), name
        if rc == 0:
            assert out == ref, name
            assert zlib.decompress(out, -15) == d
            assert [tuple(int(x) for x in b) for b in encoder.last_blocks()] == ob, name


def test_device_entry_point_equals_host(encoder):
    import torch
    for d in (silesia_mix(3 << 20, version=2), silesia_mix(40000, class_mask=1)):
        rc, ref, crc = gpu(encoder, d)
        t_in = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
        t_out = torch.zeros(len(d) + 4096, dtype=torch.uint8, device="cuda")
        rc2, ol, crc2 = encoder.deflate_device(t_in.data_ptr(), len(d), t_out.data_ptr(), len(d) + 4096, R)
        torch.cuda.synchronize()
        assert rc == rc2 == 0 and crc == crc2 and bytes(t_out[:ol].cpu().numpy()) == ref


def test_batch_equals_single_calls_and_the_model(encoder):
    src = silesia_mix(300000, version=2)
    datas = [src[1000:1000 + k] for k in (0, 1, 2, 3, 8191, 8192, 8193, 40000, 70000)] + [bytes(50000), b"ab" * 20000]
    got = encoder.deflate_batch(datas, R)
    for d, (rc2, out, crc2) in zip(datas, got):
        rc, ref, _ = expect(d)
        rc1, out1, crc1 = gpu(encoder, d)
        assert rc == rc1 == rc2 and crc2 == crc1 == crc_reg(d), len(d)
        if rc == 0:
            assert out == out1 == ref, len(d)


def test_64_mib_in_1_mib_shards_through_the_streaming_host_path(encoder):
    d = silesia_mix(64 << 20, version=2)
    toks, _ = _rich.restate(d)
    rc, ref, _ = expect(d, toks)
    encoder.set_knob("shard_kib", 1024)
    try:
        rc2, out, crc2 = gpu(encoder, d)                # (64 MiB and more: the input arrives while the LZ stage runs)
    finally:
        encoder.set_knob("shard_kib", 1 << 20)
    assert rc == rc2 == 0 and out == ref and crc2 == crc_reg(d)


def test_spans_equal_one_call():
    za = product()
    d = silesia_mix((9 << 20) + 12345, version=2)
    enc = za.Encoder(0)
    try:
        rc, ref, crc = gpu(enc, d)
        enc2 = za.Encoder(0)                              # a fresh context: spans book their workspace once
        try:
            enc2.set_knob("span_mib", 4)
            rc2, out, crc2 = gpu(enc2, d)
        finally:
            enc2.close()
    finally:
        enc.close()
    rc0, ref0, _ = expect(d)
    assert rc == rc2 == rc0 == 0 and out == ref == ref0 and crc == crc2 == crc_reg(d)


def test_three_ranges_equal_one_call(encoder):
    from test_ranges import deflate_over_contexts
    for d in (silesia_mix((3 << 20) + 4567, version=2), bytes(1 << 20), b"ab" * 400000):
        rc, ref, crc = gpu(encoder, d)
        ob = [tuple(int(x) for x in b) for b in encoder.last_blocks()]
        rc2, out, crc2, results = deflate_over_contexts(d, 3, R)
        assert rc == rc2 == 0 and out == ref and crc2 == crc, len(d)
        assert [b for res in results for b in res["blocks"]] == ob


def test_feedback_and_abort(encoder):
    za = product()
    d = silesia_mix(2 << 20, version=2)
    seen = []
    encoder.deflate(d, R, feedback=lambda pct: seen.append(pct) or False)
    assert seen[0] == 0 and seen[-1] == 100 and seen == sorted(seen)
    with pytest.raises(za.UserAbort):
        encoder.deflate(d, R, feedback=lambda pct: pct >= 5)


def test_archive_equals_the_oracles_writer(encoder):
    za = product()
    names = ["a.txt", "empty", "one", "zeros.bin", "mix.dat", "rnd.bin"]
    rs = np.random.RandomState(5)
    datas = [silesia_mix(30000, class_mask=1), b"", b"x", bytes(90000), silesia_mix(200000, version=2), bytes(rs.randint(0, 256, 5000).astype(np.uint8))]
    entries = []
    for nm, d in zip(names, datas):
        rc, payload, _ = expect(d)
        if rc == 0:
            entries.append((nm, payload, zlib.crc32(d), len(d), 8))
        else:
            entries.append((nm, d, zlib.crc32(d), len(d), 0))       # Compress_Data's Store fallback
    ref = oracle_zip_compressed(entries)
    for batched in (False, True):
        z = za.ZipCreate(encoder, za.Method.Deflate_R)
        if batched:
            z.add_streams(names, datas)
        else:
            for nm, d in zip(names, datas):
                z.add_stream(nm, d)
        blob = z.finish()
        assert blob == ref, batched
        with zipfile.ZipFile(io.BytesIO(blob)) as zf:
            for nm, d in zip(names, datas):
                assert zf.read(nm) == d
