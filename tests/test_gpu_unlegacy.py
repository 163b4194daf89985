"""The Shrink / Reduce / Implode readers on the device (zada_unlegacy*, one wave per entry) against the logic header on the CPU
(tests/unlegacy/unlegacy_host.cpp; test_unlegacy_model.py holds it equal to the decoders as the reference states them, to PKZIP's streams and to
Info-ZIP's unzip)."""
import ctypes
import hashlib
import random
import zlib

import numpy as np
import pytest

import _legacy as L
import _unlegacy as U
from _common import product
from _devbuf import GUARD, device_call, guard_damage

pytestmark = pytest.mark.gpu
E_DATA, E_INVALID, E_TOO_LARGE = -7, -1, -4


def _guarded_batch(enc, cases, out=True):
    """zada_unlegacy_batch on [(method, flags, stream, cap)] with 16 guard bytes on both sides of every output buffer
    -> (worst, rcs, out_lens, in_useds, crcs, outputs); asserts the guards."""
    cnt = len(cases)
    lens = np.array([len(c[2]) for c in cases], dtype=np.uint64)
    caps = np.array([c[3] for c in cases], dtype=np.uint64)
    meth = np.array([c[0] for c in cases], dtype=np.uint16)
    flg = np.array([c[1] for c in cases], dtype=np.uint8)
    keep = [c[2] if len(c[2]) else b"\0" for c in cases]
    ins = np.array([ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p).value for s in keep], dtype=np.uint64)
    offs = (np.concatenate(([0], np.cumsum(caps + np.uint64(32))[:-1])) + 16).astype(np.uint64)
    arena = np.full(int((caps + np.uint64(32)).sum()), GUARD, dtype=np.uint8)
    outp = (arena.ctypes.data + offs).astype(np.uint64)
    ols, ius = np.full(cnt, 77, np.uint64), np.full(cnt, 77, np.uint64)
    crcs = np.full(cnt, 0xFFFFFFFF, dtype=np.uint32)
    rcs = np.full(cnt, 99, dtype=np.int32)
    worst = enc.lib.zada_unlegacy_batch(enc.ctx, cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data if out else None, caps.ctypes.data, meth.ctypes.data,
                                        flg.ctypes.data, ols.ctypes.data, ius.ctypes.data, crcs.ctypes.data, rcs.ctypes.data)
    assert worst in (0, E_DATA), (worst, enc.lib.zada_last_error(enc.ctx))
    outs = []
    for k in range(cnt):
        o, cap = int(offs[k]), int(caps[k])
        assert not guard_damage(arena[o - 16:o + cap + 16], 16, cap), "entry %d: bytes outside its output buffer were written" % k
        outs.append(arena[o:o + int(ols[k])].tobytes() if rcs[k] == 0 else None)
    if not out:
        assert (arena == GUARD).all()
    return worst, rcs, ols, ius, crcs, outs


def _equal_the_model(enc, cases):
    """One batch: rc, out_len, in_used, CRC, bytes and last_records equal the logic header on the CPU for every entry."""
    worst, rcs, ols, ius, crcs, outs = _guarded_batch(enc, cases)
    recs = enc.unlegacy_last_records()
    assert recs.shape == (len(cases), 4)
    n_ok = 0
    for k, (m, f, s, cap) in enumerate(cases):
        rc, out, ol, used, reg, rec = U.host_decode(m, f, s, cap)
        assert (int(rcs[k]), int(ols[k]), int(ius[k]), int(crcs[k])) == (rc, ol, used, reg), (k, m, f, cap, rec, [int(x) for x in recs[k]])
        assert tuple(int(x) for x in recs[k]) == rec, (k, m, f, cap, rec, [int(x) for x in recs[k]])
        if rc == 0:
            assert outs[k] == out, (k, m, f)
            n_ok += 1
    assert worst == (E_DATA if n_ok < len(cases) else 0)
    return n_ok


def test_fixtures_three_ways(encoder):
    for row, payload in U.fixtures():
        m, f, size, reg = row["format"], row["flags"], row["size"], int(row["crc32"], 16) ^ 0xFFFFFFFF
        out, used, crc = encoder.unlegacy(payload, size, m, f)
        assert hashlib.sha256(out).hexdigest() == row["sha256"] and used == len(payload) and crc == reg, row["file"]
        (ol, used, crc), dev = device_call(lambda di, n, do, cap: encoder.unlegacy_device(di, n, do, cap, m, f), payload, size, 3, 5)
        assert (ol, used, crc) == (size, len(payload), reg) and dev == out, row["file"]
    res = encoder.unlegacy_batch([p for _, p in U.fixtures()], [r["size"] for r, _ in U.fixtures()], [r["format"] for r, _ in U.fixtures()],
                                 [r["flags"] for r, _ in U.fixtures()])
    for (row, payload), (rc, out, ol, used, crc) in zip(U.fixtures(), res):
        assert rc == 0 and hashlib.sha256(out).hexdigest() == row["sha256"] and (ol, used) == (row["size"], len(payload)), row["file"]
        assert crc == int(row["crc32"], 16) ^ 0xFFFFFFFF


@pytest.mark.parametrize("method", [1, 2, 3, 4, 5])
def test_device_round_trip(encoder, method):
    """The device's own encoders, read back on the device."""
    ins = L.gpu_test_inputs(method)
    packed = encoder.shrink_batch(ins) if method == 1 else encoder.reduce_batch(ins, method)
    kept = [(d, s) for d, (rc, s, _) in zip(ins, packed) if rc == 0]
    assert len(kept) >= len(ins) // 2
    res = encoder.unlegacy_batch([s for _, s in kept], [len(d) for d, _ in kept], method)
    for (d, s), (rc, out, ol, used, crc) in zip(kept, res):
        assert rc == 0 and out == d and used == len(s) and crc == zlib.crc32(d) ^ 0xFFFFFFFF, (method, len(d), rc, ol, used)


_cache = {}


def _mixed_entries(count=300):
    """(method, flags, stream, cap, data): all six methods and the four Implode flag combinations, edge sizes and the streams made for the branches."""
    if count not in _cache:
        _cache[count] = _make_mixed_entries(count)
    return _cache[count]


def _make_mixed_entries(count):
    r = random.Random(77)
    out = []
    for k in range(count):
        n = r.choice((0, 1, 2, 3, 64, 65, 4096, 4097)) if k % 7 == 0 else r.randint(0, 9000)
        d = L.edge_input(n, seed=200 + k) if k % 3 else L.rnd(k, n, bytes(range(256)))
        m = 1 + k % 6
        if m == 6:
            f = U.IMPLODE_FLAGS[(k // 6) % 4]
            d = d or b"x"
            out.append((6, f, U.implode(d, f), len(d), d))
        else:
            out.append((m, 0, U.encode(d, m), len(d), d))
    for f in U.IMPLODE_FLAGS:
        out += [(6, f, U.implode(d, f, reach), len(d), d) for _, d, reach in U.implode_inputs()]
    d = U.full_table_input()
    out.append((1, 0, U.shrink_no_clear(d), len(d), d))
    for name in ("shrink_orphans_valid", "reduce_zero_fill", "reduce_slen_63", "shrink_cap_0"):
        m, f, s, cap, _ = U.crafted()[name]
        out.append((m, f, s, cap, U.host_decode(m, f, s, cap)[1]))
    return out


def test_mixed_batch_of_all_six_methods(encoder):
    ents = _mixed_entries()
    assert {e[0] for e in ents} == {1, 2, 3, 4, 5, 6}
    res = encoder.unlegacy_batch([e[2] for e in ents], [e[3] for e in ents], [e[0] for e in ents], [e[1] for e in ents])
    for k, ((m, f, s, cap, d), (rc, out, ol, used, crc)) in enumerate(zip(ents, res)):
        assert rc == 0 and out == d and ol == len(d) and crc == zlib.crc32(d) ^ 0xFFFFFFFF, (k, m, f, cap, rc, ol)
        assert used == U.host_decode(m, f, s, cap)[3], (k, m, f)
    # the test-only form: nothing comes back but the records
    worst, rcs, ols, ius, crcs, _ = _guarded_batch(encoder, [e[:4] for e in ents], out=False)
    assert worst == 0 and [int(x) for x in crcs] == [r[4] for r in res] and [int(x) for x in ols] == [len(e[4]) for e in ents]


def test_several_launch_groups(encoder):
    """batch_mib = 1: the entries go through several groups, each with a launch per format present."""
    ents = _mixed_entries()
    assert sum(len(e[2]) + e[3] for e in ents) > 2 << 20
    encoder.set_knob("batch_mib", 1)
    try:
        res = encoder.unlegacy_batch([e[2] for e in ents], [e[3] for e in ents], [e[0] for e in ents], [e[1] for e in ents])
        recs = encoder.unlegacy_last_records()
    finally:
        encoder.set_knob("batch_mib", 512)
    assert recs.shape == (len(ents), 4) and not recs[:, 0].any()
    for k, ((m, f, s, cap, d), (rc, out, ol, used, crc)) in enumerate(zip(ents, res)):
        assert rc == 0 and out == d and crc == zlib.crc32(d) ^ 0xFFFFFFFF, (k, m, f)


def test_damaged_streams_equal_the_cpu_model(encoder):
    """A seeded 2 000 of the damaged corpus of test_unlegacy_model.py, and the crafted streams, in ONE batch."""
    corpus = U.damaged_corpus()
    cases = random.Random(5).sample(corpus[:20000], 2000) + corpus[20000:]
    n_ok = _equal_the_model(encoder, cases)
    assert 100 <= n_ok <= len(cases) - 500
    rules = {int(x) for x in encoder.unlegacy_last_records()[:, 0]}
    assert rules == set(range(len(U.RULES)))


def _contract_stream(kind):
    """(method, flags, stream, data): about a thousand bytes whose last token is a string / a copy, so that cap one short is not a valid stream."""
    d = L.edge_input(1000, seed=91) + L.rnd(92, 24, bytes(range(256))) * 3 + b"z" * 50
    if kind == 6:
        return 6, 6, U.implode(d, 6), d
    return kind, 0, U.encode(d, kind), d


@pytest.mark.parametrize("kind", [1, 5, 6])
def test_device_contract(encoder, kind):
    """The input and the output at every byte alignment 0 .. 15, the input ending at its tensor's last byte, guards on both sides of the output, cap
    exact; cap one short is ZADA_E_DATA and delivers nothing (the decoders write as they go: what the cap bytes hold then is not specified, the bytes
    around them are untouched); the register started anywhere; out = NULL."""
    m, f, s, d = _contract_stream(kind)
    want = (len(d), len(s), zlib.crc32(d) ^ 0xFFFFFFFF)
    assert U.host_decode(m, f, s, len(d))[:4] == (0, d, len(d), len(s)) and U.host_decode(m, f, s, len(d) - 1)[5][0] == 2
    fn = lambda di, n, do, cap: encoder.unlegacy_device(di, n, do, cap, m, f)
    for a_in in range(16):
        for a_out in range(16):
            got, out = device_call(fn, s, len(d), a_in, a_out)
            assert got == want and out == d, (kind, a_in, a_out, got)
    # cap one short, through the C ABI, so that the guards are looked at behind the refusal
    import torch
    t_in = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).cuda()
    t_out = torch.full((len(d) - 1 + 48,), GUARD, dtype=torch.uint8, device="cuda")
    ol, iu, reg = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(0x1234)
    rc = encoder.lib.zada_unlegacy_device(encoder.ctx, m, f, t_in.data_ptr(), len(s), t_out.data_ptr() + 9, len(d) - 1, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg))
    torch.cuda.synchronize()
    assert rc == E_DATA and (ol.value, iu.value, reg.value) == (0, 0, 0x1234)
    assert not guard_damage(t_out.cpu().numpy(), 9, len(d) - 1)
    err = encoder.lib.zada_last_error(encoder.ctx)
    assert b"unlegacy: entry 0: output beyond cap at input byte " in err, err
    # the register started anywhere
    (ol_, iu_, crc_), _ = device_call(lambda di, n, do, cap: encoder.unlegacy_device(di, n, do, cap, m, f, crc=0x1234ABCD), s, len(d), 1, 2)
    assert crc_ == zlib.crc32(d, 0x1234ABCD ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
    assert encoder.unlegacy(s, len(d), m, f, crc=0x1234ABCD)[2] == crc_
    # out = NULL: the test-only form
    rcs = encoder.unlegacy_batch([s, s], [len(d), len(d) - 1], m, f, deliver=False)
    assert [(r[0], r[1], r[2], r[3]) for r in rcs] == [(0, None, len(d), len(s)), (E_DATA, None, 0, 0)] and rcs[0][4] == want[2] and rcs[1][4] == 0xFFFFFFFF


def test_argument_checks_come_first(encoder):
    import torch
    lib, ctx = encoder.lib, encoder.ctx
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    for method in (0, 7, -1, 14):
        assert lib.zada_unlegacy_device(ctx, method, 0, p, 8, p + 32, 8, None, None, None) == E_INVALID
        assert lib.zada_unlegacy(ctx, method, 0, None, 0, None, 0, None, None, None) == E_INVALID
    assert b"method outside 1 .. 6" in lib.zada_last_error(ctx)
    assert lib.zada_unlegacy_device(ctx, 1, 0, p, 8, p + 32, (1 << 64) - 8, None, None, None) == E_TOO_LARGE
    assert lib.zada_unlegacy_device(ctx, 1, 0, p, 1 << 40, p + 32, 8, None, None, None) == E_TOO_LARGE
    assert lib.zada_unlegacy_device(ctx, 1, 0, None, 5, p, 5, None, None, None) == E_INVALID
    assert lib.zada_unlegacy_device(ctx, 1, 0, p, 5, None, 5, None, None, None) == E_INVALID
    assert lib.zada_unlegacy(ctx, 6, 0, None, 5, None, 0, None, None, None) == E_INVALID
    assert lib.zada_unlegacy_batch(ctx, 1, None, None, None, None, None, None, None, None, None, None) == E_INVALID
    za = product()
    with pytest.raises(za.ZadaError):
        encoder.unlegacy_batch([b"ab"], [4], [9])
    with pytest.raises(za.ZadaError):
        encoder.unlegacy_batch([b"ab", b"ab"], [(1 << 64) - 8, 40], 1)
    assert encoder.unlegacy_batch([], [], 1) == []
    # cap = 0: Shrink reads nothing, Reduce and Implode read their tables
    assert encoder.unlegacy(b"", 0, 1) == (b"", 0, 0xFFFFFFFF)
    assert encoder.unlegacy(bytes(192), 0, 3) == (b"", 192, 0xFFFFFFFF)
    with pytest.raises(za.DataError):
        encoder.unlegacy(bytes(100), 0, 3)
