"""Shrink_1 on the device (zada_shrink, zada_shrink_device, zada_shrink_batch) against the CPU model's closed form (tests/legacy/shrink_model.c, which
test_legacy_model.py holds against the stated form and the decoder): streams, lengths, rc and CRC registers byte for byte."""
import ctypes
import zlib

import pytest

import _legacy as L
from _devbuf import GUARD, device_call, guarded_batch

gpu = pytest.mark.gpu
FF = 0xFFFFFFFF
E_INVALID = -1
_cache = {}


def _want(data):
    key = (len(data), zlib.crc32(data))
    if key not in _cache:
        _cache[key] = L.model_result(data, 1)
    return _cache[key]


def _reg(data, start):
    return zlib.crc32(data, start ^ FF) ^ FF


def _check_batch(enc, datas, what):
    got = enc.shrink_batch(datas)
    assert len(got) == len(datas)
    for i, (d, (rc, s, reg)) in enumerate(zip(datas, got)):
        wrc, ws, wreg = _want(d)
        assert rc == wrc and reg == wreg, (what, i, len(d), rc, wrc)
        assert s == (ws if wrc == 0 else None), (what, i, len(d))


@gpu
def test_shrink_edge_sizes(encoder):
    """Sizes 0, 1, 2, around every look-ahead of Reduce and around 4 096 (the sizes the two methods' tests share), one batch; each also alone."""
    datas = [L.edge_input(n) for n in L.edge_sizes()]
    _check_batch(encoder, datas, "edges")
    for d in datas[:6] + datas[-2:]:
        rc, s, ol, reg = encoder.shrink(d)
        wrc, ws, wreg = _want(d)
        assert (rc, ol, reg) == (wrc, len(ws), wreg) and s == (ws if wrc == 0 else None), len(d)
    assert encoder.shrink(b"")[:3] == (1, None, 0) and encoder.shrink(b"x")[0] == 1        # nothing written; 2 bytes for 1


@gpu
def test_shrink_clears_rises_and_duplicates(encoder):
    """The inputs whose census (test_legacy_model.py) shows partial clears, the four rises of the code size and duplicate adds behind a clear;
    16 KiB of random bytes give a stream that is longer than the input: rc 1, its length reported."""
    ins = L.shrink_inputs()
    _check_batch(encoder, list(ins.values()), "named")
    rc, s, ol, reg = encoder.shrink(ins["random_16k"])
    assert rc == 1 and s is None and ol == 24317
    rc, s, ol, reg = encoder.shrink(ins["abcd_48k"], crc=0x12345678)
    assert rc == 0 and len(s) == 14248 and s == _want(ins["abcd_48k"])[1] and reg == _reg(ins["abcd_48k"], 0x12345678)
    assert len(encoder.shrink(ins["abcd_128k"])[1]) == 37328


def _device(enc, data, cap, a_in=0, a_out=0, crc=FF, crc_null=False):
    ol, c = ctypes.c_uint64(0), ctypes.c_uint32(crc)
    (rc, out) = device_call(lambda d_in, n, d_out, k: enc.lib.zada_shrink_device(enc.ctx, d_in, n, d_out, k, ctypes.byref(ol), None if crc_null else ctypes.byref(c)),
                            data, cap, a_in, a_out)
    return rc, ol.value, c.value, out


@gpu
def test_shrink_device_contract(encoder):
    """zada_shrink_device: input and output at every byte alignment, the input tensor ending at its last byte, guard bytes on both sides of the
    output, cap exact and one byte short, the register started anywhere or absent."""
    d = L.contract_input(1)
    wrc, ws, _ = _want(d)
    assert wrc == 0
    for k in range(256):
        a_in, a_out = k % 16, k // 16
        cap = len(ws) if k % 3 == 0 else len(d) + 64
        start = FF if k % 2 else (0x9E3779B9 * (k + 1)) & FF
        rc, ol, reg, out = _device(encoder, d, cap, a_in, a_out, start)
        assert (rc, ol, reg) == (0, len(ws), _reg(d, start)) and out[:ol] == ws and out[ol:] == bytes([GUARD]) * (cap - ol), (a_in, a_out)
    for a in (0, 1, 7):
        rc, ol, reg, out = _device(encoder, d, len(ws) - 1, a, 15 - a)
        assert rc == E_INVALID and b"too small" in encoder.lib.zada_last_error(encoder.ctx) and out == bytes([GUARD]) * (len(ws) - 1)
    rc, ol, reg, out = _device(encoder, d, len(ws), 3, 5, crc_null=True)
    assert rc == 0 and out == ws
    for e in L.contract_small_inputs(1):                              # rc 1 or 0 as the model says, at odd alignments, with cap = n
        n = len(e)
        wrc, ws2, wreg = _want(e)
        rc, ol, reg, out = _device(encoder, e, n, 5, 9, 0xCAFEBABE)
        assert (rc, ol, reg) == (wrc, len(ws2), _reg(e, 0xCAFEBABE)), n
        assert out[:ol] == ws2 if rc == 0 else out == bytes([GUARD]) * n, n
    r = L.contract_random_input()
    rc, ol, reg, out = _device(encoder, r, len(r), 1, 2)
    assert rc == 1 and ol == len(_want(r)[1]) >= len(r) and out == bytes([GUARD]) * len(r)


@gpu
def test_shrink_batch_contract_and_mixed_sizes(encoder):
    """zada_shrink_batch on a guarded arena -- cap exact, one byte short, none -- and the 300 entries of mixed sizes 0 .. 9 000."""
    datas = L.batch_contract_inputs(1)
    want = [_want(d) for d in datas]
    caps = [len(want[0][1]), len(want[1][1]) - 1, 0, len(datas[3]), 1, 0, 2000]
    worst, rcs, ols, crcs, outs = guarded_batch(lambda *a: encoder.lib.zada_shrink_batch(encoder.ctx, *a), datas, caps)
    assert worst == E_INVALID and list(rcs) == [0, E_INVALID, 1, 0, 1, E_INVALID, 1], list(rcs)
    assert [int(x) for x in ols] == [len(w[1]) for w in want] and [int(c) for c in crcs] == [w[2] for w in want]
    assert outs[0] == want[0][1] and outs[3][:len(want[3][1])] == want[3][1]
    assert outs[1] == bytes([GUARD]) * caps[1] and outs[6] == bytes([GUARD]) * 2000 and outs[4] == bytes([GUARD])
    _check_batch(encoder, L.batch_inputs(), "mixed")
