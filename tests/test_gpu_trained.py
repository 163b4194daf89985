"""Trained_Compression on the device (zada_trained_*, TrainedCompression): the stub and the messages against the oracle's LZMA.Encoding.Encode with
Trained_Compression's parameters, byte for byte; the decoding side -- the stub decoded once, every entry's wave started from that state -- against
the data, liblzma and the CPU model of the same decoder (tests/trained/trained_host.cpp); where the decoder's fork lies; skip at its edges; the
pointer contract with guard bytes; damaged messages in one batch; contexts with no history.
Both sides fork: the encoding side codes the trainer once up to fork_pos and every entry of a batch goes on from there (an entry beyond one window
fill, and every entry of a trainer below 8 738 bytes, codes its whole stream in the same launch); the decoding side decodes the stub once."""
import numpy as np
import pytest

import _trained
from _common import product, silesia_mix
from _devbuf import GUARD, TAIL, device_call, guard_damage
from _lzmah import lzma_decode
from _trained import E_DATA, FORK_MARGIN, MARGIN, common_prefix, fixture, message_of, model_decode, stub_of, tc_stream

pytestmark = pytest.mark.gpu
E_INVALID = -1
KEEP_AFTER = _trained.KEEP_AFTER                       # 4 369: the coder stops that far in front of the trainer's end; trainers below twice that are not forked
ONE_FILL = 1 << 20                                     # String_buffer_size for the dictionary of 2 ** 19: a longer stream is not forked


def _forks(T, n):
    return T >= 2 * KEEP_AFTER and T + n <= ONE_FILL


def _both_sides(za, enc, trainer, skip=None, noise=b""):
    tc = za.TrainedCompression(enc, trainer, skip=skip, noise=noise)
    return tc, za.TrainedCompression.for_decoding(enc, tc.stub, tc.skip, tc.trainer_len)


def _round_trip(za, enc, trainer, datas, skip=None):
    """encode, compare with the oracle, decode on the device and with liblzma -> (the encoding side, the decoding side), both still open"""
    tc, td = _both_sides(za, enc, trainer, skip)
    assert tc.stub == stub_of(trainer)
    msgs = tc.encode(datas)
    for d, m in zip(datas, msgs):
        assert m == message_of(trainer, d, tc.skip), (len(trainer), len(d), tc.skip)
        if tc.skip <= common_prefix(tc.stub, tc_stream(trainer + d)):
            assert lzma_decode(tc.stub[:tc.skip] + m) == trainer + d
    want = sum(_forks(len(trainer), len(d)) for d in datas)
    assert (tc.info()["forked"], tc.info()["unforked"]) == (want, len(datas) - want)
    assert td.decode(msgs, [len(d) for d in datas]) == [bytes(d) for d in datas]
    return tc, td


def test_fixtures(encoder):
    za = product()
    noise = fixture("rnd_10.bin")
    forked = 0
    for t in ("gs1.xls", "wsbase.csv"):
        trainer = fixture(t) + noise
        datas = [fixture(d) for tt, d in _trained.PAIRS if tt == t]
        tc = za.TrainedCompression(encoder, fixture(t), noise=noise)
        assert tc.stub == stub_of(trainer) and tc.skip == len(tc.stub) - MARGIN and tc.trainer_len == len(trainer)
        msgs = tc.encode(datas)
        assert msgs == [message_of(trainer, d, tc.skip) for d in datas]
        td = za.TrainedCompression.for_decoding(encoder, tc.stub, tc.skip, tc.trainer_len)
        assert td.decode(msgs, [len(d) for d in datas]) == datas
        assert tc.info()["forked"] == 2 and tc.info()["unforked"] == 0
        i = td.info()
        forked += i["forked"]
        assert i["unforked"] == 0 and 0 <= tc.skip - i["dec_fork_in"] <= FORK_MARGIN and 0 < i["dec_fork_out"] <= len(trainer)
        # the decoder's snapshot is where the CPU model stops
        assert model_decode(tc_stream(trainer + datas[0]), len(trainer) + len(datas[0]), in_limit=tc.skip)[1] == (i["dec_fork_in"], i["dec_fork_out"])
        tc.close(); td.close()
    assert forked == 4


def test_the_join(encoder):
    za = product()
    trainer = bytes(silesia_mix(11800, class_mask=1)) + b"a" * 200
    rng = np.random.default_rng(5)
    datas = [b"", b"q", b"a" * 400, trainer[-300:] + bytes(silesia_mix(500, class_mask=1, seed=9)), trainer, bytes(rng.integers(0, 256, 2000, dtype=np.uint8))]
    tc, td = _round_trip(za, encoder, trainer, datas)
    assert td.info()["forked"] == len(datas) and tc.info()["forked"] == len(datas)
    # the same handles without their snapshots (the knob of the measurements): the same bytes
    msgs = tc.encode(datas)
    encoder.set_knob("trained_fork", 0)
    try:
        assert tc.encode(datas) == msgs and tc.info()["unforked"] == len(datas)
        assert td.decode(msgs, [len(d) for d in datas]) == datas and td.info()["unforked"] == len(datas)
    finally:
        encoder.set_knob("trained_fork", 1)
    tc.close(); td.close()


@pytest.mark.parametrize("T", [0, 1, 300, 4368, 4369, 4370, 9000, 16384, 20000])
def test_trainer_lengths(encoder, T):
    """Trainers around the matcher's look-ahead (4 369 bytes) and below it: the bytes are the oracle's whichever way an entry takes, and the decoder's
    snapshot lies within 64 bytes in front of skip wherever there is one."""
    za = product()
    trainer = bytes(silesia_mix(T, class_mask=1, seed=3))
    data = bytes(silesia_mix(700, class_mask=1, seed=4))
    tc, td = _round_trip(za, encoder, trainer, [data, data[:1], b""])
    i = td.info()
    if tc.skip >= 10:
        assert i["forked"] == 3 and 0 <= tc.skip - i["dec_fork_in"] <= FORK_MARGIN and i["dec_fork_out"] <= T
    else:
        assert i["unforked"] == 3 and (i["dec_fork_in"], i["dec_fork_out"]) == (0, 0)
    if T >= 16384:
        assert tc.skip >= 10 and i["dec_fork_in"] > 0
    # the coder's fork is taken and is where it may be: at most twice the look-ahead in front of the trainer's end, and the stream bytes written
    # there are bytes every stream of this trainer has
    e = tc.info()
    if T >= 2 * KEEP_AFTER:
        assert e["forked"] == 3 and 0 < T - e["fork_pos"] <= 2 * KEEP_AFTER
        other = bytes(silesia_mix(900, seed=77))
        assert 0 < e["fork_out"] <= min(common_prefix(tc_stream(trainer + data), tc_stream(trainer + other)), common_prefix(tc.stub, tc_stream(trainer + other)))
    else:
        assert e["unforked"] == 3 and (e["fork_pos"], e["fork_out"]) == (0, 0)
    tc.close(); td.close()


def test_skip_at_its_edges(encoder):
    za = product()
    trainer = fixture("wsbase.csv")[:9000]
    datas = [fixture("wm1ns.csv")[2000:3500], fixture("wm2ns.csv")[:900]]
    stub = stub_of(trainer)
    common = min(common_prefix(stub, tc_stream(trainer + d)) for d in datas)
    assert common >= len(stub) - MARGIN
    probe = za.TrainedCompression(encoder, trainer)
    fork_out = probe.info()["fork_out"]
    probe.close()
    assert 0 < fork_out < common
    for skip in (0, 4, 9, 10, 11, 73, 74, fork_out - 1, fork_out, fork_out + 1, len(stub) - MARGIN, common - 1, common):
        tc, td = _round_trip(za, encoder, trainer, datas, skip=skip)
        assert td.info()["forked" if skip >= 10 else "unforked"] == 2
        tc.close(); td.close()
    # one byte beyond what the streams have in common: both sides do what the reference does with those bytes -- the message is the oracle's slice,
    # and the decoder's verdict on stub [: skip] + message is the CPU model's
    tc, td = _both_sides(za, encoder, trainer, skip=common + 1)
    msgs = tc.encode(datas)
    assert msgs == [message_of(trainer, d, common + 1) for d in datas]
    got = td.decode(msgs, [len(d) for d in datas], errors="return")
    for d, m, g in zip(datas, msgs, got):
        rec, _ = model_decode(stub[:common + 1] + m, len(trainer) + len(d))
        assert (g == rec[1][len(trainer):]) if rec[0] == 0 else isinstance(g, za.DataError)
    tc.close(); td.close()


def test_a_large_trainer(encoder):
    """300 KiB of trainer -- beyond 2 ** 18, the decoder's snapshot far into the stream -- and two messages."""
    za = product()
    trainer = bytes(silesia_mix(300 * 1024, seed=12))
    datas = [bytes(silesia_mix(5000, seed=13)), trainer[1000:4000]]
    tc, td = _round_trip(za, encoder, trainer, datas)
    assert td.info()["dec_fork_out"] > 200 * 1024
    tc.close(); td.close()


def test_an_entry_beyond_one_window_fill(encoder):
    """300 KiB of trainer and a message that takes the stream beyond String_buffer_size = 2 ** 20 bytes: the entry codes its whole stream, in the same
    launch as a forked neighbour.  The message is silesia_mix's seed 40: the first of 40 .. 45 tried on the CPU, the oracle's stream decodes under
    liblzma for all six."""
    za = product()
    T = 300 * 1024
    trainer = bytes(silesia_mix(T, seed=12))
    long = bytes(silesia_mix(ONE_FILL - T + 4321, seed=40))
    tc = za.TrainedCompression(encoder, trainer)
    assert tc.stub == stub_of(trainer)
    import torch
    dev = torch.device("cuda", encoder.device)
    datas = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to(dev) for d in (long, long[:3000])]
    outs = [torch.empty(len(long) // 2, dtype=torch.uint8, device=dev), torch.empty(4000, dtype=torch.uint8, device=dev)]
    torch.cuda.synchronize()
    rc, ols, rcs = tc.encode_raw([(d.data_ptr(), d.numel(), o.data_ptr(), o.numel()) for d, o in zip(datas, outs)])
    assert (rc, rcs) == (0, [0, 0]) and (tc.info()["forked"], tc.info()["unforked"]) == (1, 1)
    for d, o, n in zip((long, long[:3000]), outs, ols):
        m = bytes(o[:n].cpu().numpy().tobytes())
        assert m == message_of(trainer, d, tc.skip)
    assert lzma_decode(tc.stub[:tc.skip] + message_of(trainer, long, tc.skip)) == trainer + long
    tc.close()


def test_pointer_contract(encoder):
    za = product()
    trainer = bytes(silesia_mix(2000, class_mask=1, seed=6))
    data = bytes(silesia_mix(777, class_mask=1, seed=7))
    tc, td = _both_sides(za, encoder, trainer)
    want = message_of(trainer, data, tc.skip)
    for a in range(16):
        a_out = (a * 5 + 3) % 16
        (rc, ols, rcs), out = device_call(lambda d_in, n, d_out, cap: tc.encode_raw([(d_in, n, d_out, cap)]), data, len(want), a, a_out)
        assert (rc, ols, rcs) == (0, [len(want)], [0]) and out == want, a
        (rc, ols, rcs), out = device_call(lambda d_in, n, d_out, cap: tc.encode_raw([(d_in, n, d_out, cap)]), data, len(want) - 1, a_out, a)
        assert (rc, ols, rcs) == (E_INVALID, [len(want)], [E_INVALID]) and out == want[:-1], a
        assert b"output buffer too small" in encoder.lib.zada_last_error(encoder.ctx)
        (rc, ols, rcs), out = device_call(lambda d_in, n, d_out, cap: td.decode_raw([(d_in, n, d_out, cap)]), want, len(data), a, a_out)
        assert (rc, ols, rcs) == (0, [len(data)], [0]) and out == data, a
        (rc, ols, rcs), out = device_call(lambda d_in, n, d_out, cap: td.decode_raw([(d_in, n, d_out, cap)]), want, len(data) - 1, a_out, a)
        assert (rc, ols, rcs) == (E_DATA, [0], [E_DATA]) and out == bytes([GUARD]) * (len(data) - 1), a
        assert b"output beyond cap" in encoder.lib.zada_last_error(encoder.ctx)
    # count = 0, and the argument checks before anything touches the device
    assert tc.encode_raw([]) == (0, [], []) and td.decode_raw([]) == (0, [], [])
    assert tc.decode_raw([])[0] == E_INVALID and td.encode_raw([])[0] == E_INVALID               # (a handle of the other side)
    assert tc.encode_raw([(0, 5, 0, 0)])[0] == E_INVALID and td.decode_raw([(0, 0, 0, 5)])[0] == E_INVALID
    tc.close(); td.close()


def test_damaged_messages_in_one_batch(encoder):
    import torch
    za = product()
    trainer = fixture("gs1.xls")[:9000]
    data = fixture("gs2.xls")[1000:3500]
    tc, td = _both_sides(za, encoder, trainer)
    good = message_of(trainer, data, tc.skip)
    rng = np.random.default_rng(33)
    msgs = []
    for k in range(64):
        b = bytearray(good)
        if k % 4 == 1:
            b[int(rng.integers(0, len(b)))] ^= int(rng.integers(1, 256))
        elif k % 4 == 2:
            b = b[:int(rng.integers(0, len(b)))]
        elif k % 16 == 3:
            b = bytearray()
        msgs.append(bytes(b))
    cap, G = len(data), 32
    blob = b"".join(msgs)
    t_in = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    t_out = torch.full((64 * (cap + G) + G,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rows, off = [], 0
    for k, m in enumerate(msgs):
        rows.append((t_in.data_ptr() + off if m else 0, len(m), t_out.data_ptr() + G + k * (cap + G), cap))
        off += len(m)
    rc, ols, rcs = td.decode_raw(rows)
    torch.cuda.synchronize()
    host = t_out.cpu().numpy()
    assert bytes(t_in.cpu().numpy().tobytes()) == blob
    bad = 0
    for k, m in enumerate(msgs):
        rec, _ = model_decode(tc.stub[:tc.skip] + m, len(trainer) + cap)
        o = G + k * (cap + G)
        assert not guard_damage(host[o - G:o + cap + G], G, cap), k
        if rec[0] == 0:
            assert (rcs[k], ols[k]) == (0, len(rec[1]) - len(trainer)) and host[o:o + ols[k]].tobytes() == rec[1][len(trainer):], k
        else:
            bad += 1
            assert (rcs[k], ols[k]) == (E_DATA, 0) and not guard_damage(host[o:o + cap], 0, 0), k     # (nothing of a refused entry is delivered)
        if k % 4 == 0:
            assert rcs[k] == 0 and host[o:o + cap].tobytes() == data, k
    assert rc == E_DATA and bad >= 30
    first = next(k for k in range(64) if rcs[k])
    assert ("entry %d:" % first).encode() in encoder.lib.zada_last_error(encoder.ctx)
    got = td.decode(msgs, [cap] * 64, errors="return")
    assert [isinstance(g, za.DataError) for g in got] == [r != 0 for r in rcs]
    with pytest.raises(za.DataError):
        td.decode(msgs, [cap] * 64)
    tc.close(); td.close()


def test_a_fresh_context():
    """The first calls on a new context are open_decoder and decode_device; two handles on one context used alternately; a Deflate call between open
    and encode does not disturb the handle."""
    import zlib
    za = product()
    t1, t2 = fixture("wsbase.csv")[:6000], bytes(silesia_mix(5000, class_mask=1, seed=8))
    d1, d2 = fixture("wm1ns.csv")[500:1500], bytes(silesia_mix(900, class_mask=1, seed=9))
    s1, s2 = stub_of(t1), stub_of(t2)
    k1, k2 = len(s1) - MARGIN, len(s2) - MARGIN
    m1, m2 = message_of(t1, d1, k1), message_of(t2, d2, k2)
    enc = za.Encoder(0)
    try:
        a = za.TrainedCompression.for_decoding(enc, s1, k1, len(t1))
        assert a.decode([m1], [len(d1)]) == [d1]
        b = za.TrainedCompression.for_decoding(enc, s2, k2, len(t2))
        for _ in range(2):
            assert b.decode([m2, m2], [len(d2)] * 2) == [d2, d2]
            assert a.decode([m1], [len(d1)]) == [d1]
        a.close(); b.close()
    finally:
        enc.close()
    enc = za.Encoder(0)
    try:
        e1 = za.TrainedCompression(enc, t1)
        e2 = za.TrainedCompression(enc, t2)
        mix = bytes(silesia_mix(200000))
        out, _ = enc.deflate(mix, za.Method.Deflate_3)
        assert zlib.decompress(out, -15) == mix
        assert e1.encode([d1]) == [m1] and e2.encode([d2, d2]) == [m2, m2] and e1.encode([d1, b""]) == [m1, message_of(t1, b"", k1)]
        assert e1.stub == s1 and e2.stub == s2
        e1.close(); e2.close()
    finally:
        enc.close()
