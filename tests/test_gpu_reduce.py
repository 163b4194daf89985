"""Reduce_1 .. _4 on the device (zada_reduce, zada_reduce_device, zada_reduce_batch) against the CPU model's closed form (tests/legacy/reduce_model.c,
which test_legacy_model.py holds against the stated form and the decoder): streams, lengths, rc and CRC registers byte for byte, and -- through
zada_reduce_last_record -- the raw bytes behind the matcher, Slen and the followers in use."""
import ctypes
import zlib

import pytest

import _legacy as L
from _devbuf import GUARD, device_call, guarded_batch

gpu = pytest.mark.gpu
FF = 0xFFFFFFFF
E_INVALID = -1
_cache = {}


def _model(data, method):
    """(rc, stream, register, raw bytes, Slen, followers in use) of the model, kept: the tests share them."""
    key = (method, len(data), zlib.crc32(data))
    if key not in _cache:
        s, raw, slen, foll, _ = L.reduce(data, method - 1)
        _cache[key] = (1 if len(s) >= len(data) else 0, s, zlib.crc32(data) ^ FF, raw, bytes(slen), L.followers_in_use(slen, foll))
    return _cache[key]


def _reg(data, start):
    return zlib.crc32(data, start ^ FF) ^ FF


def _check_batch(enc, datas, method, what, records=True):
    got = enc.reduce_batch(datas, method)
    assert len(got) == len(datas)
    for i, (d, (rc, s, reg)) in enumerate(zip(datas, got)):
        wrc, ws, wreg = _model(d, method)[:3]
        assert rc == wrc and reg == wreg, (what, method, i, len(d), rc, wrc)
        assert s == (ws if wrc == 0 else None), (what, method, i, len(d))
    if records:                                            # (one launch group: the records are those of the whole list)
        for i, d in enumerate(datas):
            raw, slen, foll = enc.reduce_last_record(i)
            _, _, _, wraw, wslen, wfoll = _model(d, method)
            assert raw == wraw, (what, method, i, "raw bytes")
            assert bytes(slen) == wslen and L.followers_in_use(slen, foll) == wfoll, (what, method, i, "follower sets")


@gpu
@pytest.mark.parametrize("method", [2, 3, 4, 5])
def test_reduce_edge_sizes(encoder, method):
    """Sizes 0, 1, 2, look-ahead - 1, look-ahead, look-ahead + 1, 4 095, 4 096, 4 097 and 4 096 + look-ahead of the factor, one batch; some also alone."""
    datas = [L.edge_input(n) for n in L.edge_sizes(method - 1)]
    _check_batch(encoder, datas, method, "edges")
    for d in datas[:4] + datas[-1:]:
        rc, s, ol, reg = encoder.reduce(d, method)
        wrc, ws, wreg = _model(d, method)[:3]
        assert (rc, ol, reg) == (wrc, len(ws), wreg) and s == (ws if wrc == 0 else None), len(d)
    assert encoder.reduce(b"", method)[:3] == (1, None, 192)                              # 256 empty follower sets for nothing


@gpu
@pytest.mark.parametrize("method", [2, 3, 4, 5])
def test_reduce_named_inputs(encoder, method):
    """Literal 144s, pairs expanded for their distance, two-byte lengths, every Slen (the censuses: test_legacy_model.py), and one input whose raw
    stream passes the 256 KiB of the reference's cache."""
    ins = L.reduce_inputs()
    _check_batch(encoder, list(ins.values()), method, "named")


def _device(enc, method, data, cap, a_in=0, a_out=0, crc=FF, crc_null=False):
    ol, c = ctypes.c_uint64(0), ctypes.c_uint32(crc)
    (rc, out) = device_call(lambda d_in, n, d_out, k: enc.lib.zada_reduce_device(enc.ctx, method, d_in, n, d_out, k, ctypes.byref(ol), None if crc_null else ctypes.byref(c)),
                            data, cap, a_in, a_out)
    return rc, ol.value, c.value, out


@gpu
def test_reduce_device_contract(encoder):
    """zada_reduce_device: input and output at every byte alignment, the input tensor ending at its last byte, guard bytes on both sides of the
    output, cap exact and one byte short, the register started anywhere or absent."""
    d = L.contract_input(5)                                          # (short: one wave walks the matcher's tree byte after byte, 256 times)
    for k in range(256):
        method = 2 + k % 4
        wrc, ws = _model(d, method)[:2]
        assert wrc == 0
        a_in, a_out = k % 16, k // 16
        cap = len(ws) if k % 3 == 0 else len(d) + 64
        start = FF if k % 2 else (0x9E3779B9 * (k + 1)) & FF
        rc, ol, reg, out = _device(encoder, method, d, cap, a_in, a_out, start)
        assert (rc, ol, reg) == (0, len(ws), _reg(d, start)) and out[:ol] == ws and out[ol:] == bytes([GUARD]) * (cap - ol), (method, a_in, a_out)
    ws = _model(d, 5)[1]
    for a in (0, 1, 7):
        rc, ol, reg, out = _device(encoder, 5, d, len(ws) - 1, a, 15 - a)
        assert rc == E_INVALID and b"too small" in encoder.lib.zada_last_error(encoder.ctx) and out == bytes([GUARD]) * (len(ws) - 1)
    rc, ol, reg, out = _device(encoder, 5, d, len(ws), 3, 5, crc_null=True)
    assert rc == 0 and out == ws
    for e in L.contract_small_inputs(5):                              # rc as the model says, at odd alignments, with cap = n
        n = len(e)
        wrc, ws2 = _model(e, 5)[:2]
        rc, ol, reg, out = _device(encoder, 5, e, n, 5, 9, 0xCAFEBABE)
        assert (rc, ol, reg) == (wrc, len(ws2), _reg(e, 0xCAFEBABE)), n
        assert (out[:ol] == ws2) if rc == 0 else (out == bytes([GUARD]) * n), n
    assert encoder.lib.zada_reduce_device(encoder.ctx, 1, None, 0, None, 0, None, None) == E_INVALID      # Shrink_1 is not a Reduce method
    assert encoder.lib.zada_reduce_device(encoder.ctx, 6, None, 0, None, 0, None, None) == E_INVALID


@gpu
def test_reduce_batch_contract_mixed_sizes_and_groups(encoder):
    """zada_reduce_batch on a guarded arena -- cap exact, one byte short, none --; the 300 entries of mixed sizes 0 .. 9 000 under Reduce_4, and
    again with "reduce_group_mib" low enough for several launch groups: the same bytes."""
    datas = L.batch_contract_inputs(5)
    want = [_model(d, 5) for d in datas]
    caps = [len(want[0][1]), len(want[1][1]) - 1, 0, len(datas[3]), 1, 0, 2000]
    worst, rcs, ols, crcs, outs = guarded_batch(lambda *a: encoder.lib.zada_reduce_batch(encoder.ctx, 5, *a), datas, caps)
    assert worst == E_INVALID and list(rcs) == [0, E_INVALID, 1, 0, 1, E_INVALID, 1], list(rcs)
    assert [int(x) for x in ols] == [len(w[1]) for w in want] and [int(c) for c in crcs] == [w[2] for w in want]
    assert outs[0] == want[0][1] and outs[3][:len(want[3][1])] == want[3][1]
    assert outs[1] == bytes([GUARD]) * caps[1] and outs[6] == bytes([GUARD]) * 2000 and outs[4] == bytes([GUARD])
    mixed = L.batch_inputs()
    _check_batch(encoder, mixed, 5, "mixed")
    try:
        encoder.set_knob("reduce_group_mib", 16)           # 328 KiB and the raw bytes per entry: about 47 entries a group
        _check_batch(encoder, mixed, 5, "mixed, several groups", records=False)
    finally:
        encoder.set_knob("reduce_group_mib", 4096)
