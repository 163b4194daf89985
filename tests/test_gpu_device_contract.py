"""The device-pointer contract of the WRITERS -- zada_deflate_device, zada_bzip2_device, zada_lzma_device, zada_crc32_device and the three
zada_*_batch calls -- as the reader tests check it for zada_inflate_device and its kin: input and output at every byte alignment, the input
tensor ending at its last byte, guard bytes on both sides of the output (tests/_devbuf.py), cap exact and one byte short, the CRC register
started anywhere.  The expected bytes are the oracle's (Deflate_R: the oracle's entropy stage fed the CPU model's tokens, _rich.deflate_r),
the expected registers zlib's; no other entry point of the product is asked.  Every write past `cap` these tests can see lands in guard bytes
of the test's own allocation."""
import ctypes
import zlib

import numpy as np
import pytest

import _rich
from _bzip2 import oracle_encode
from _common import oracle_deflate, silesia_mix
from _devbuf import GUARD, device_call, guard_damage, guarded_batch
from _lzmah import oracle_lzma

gpu = pytest.mark.gpu
E_INVALID = -1
FF = 0xFFFFFFFF
EDGE_LENGTHS = (0, 1, 15, 16, 17, 32767, 32768, 32769, 65535, 65537, 40000)
COPY_LENGTHS = ((1 << 20) + 5, (1 << 20) + 16, (1 << 20) + 32)      # range_lz: k_copy16 or hipMemcpyAsync, by n % 16 on a buffer of exactly n bytes
SPAN_LENGTH = (3 << 20) + 77
_cache = {}


def test_guard_comparison_sees_every_edge():
    """guard_damage (plain numpy) reports a change of one byte at each of the four guard edges, and nothing else."""
    for a_out, cap in ((0, 0), (0, 7), (5, 0), (5, 100), (15, 33), (16, 16)):
        buf = np.full(cap + 48, GUARD, dtype=np.uint8)
        buf[a_out:a_out + cap] = np.arange(cap, dtype=np.uint8) ^ 0x5A      # (the output itself may hold anything, GUARD included)
        assert guard_damage(buf, a_out, cap) == []
        edges = [a_out + cap, len(buf) - 1] + ([0, a_out - 1] if a_out else [])
        for e in edges:
            for v in (GUARD ^ 1, 0, 0xFF):
                b = buf.copy()
                b[e] = v
                assert guard_damage(b, a_out, cap) == [e], (a_out, cap, e, v)
        b = buf.copy()
        for e in edges:
            b[e] = 0
        assert guard_damage(b, a_out, cap) == sorted(set(edges))
    buf = np.full(64, GUARD, dtype=np.uint8)
    assert guard_damage(buf, 16, 16, fill=0) == list(range(16)) + list(range(32, 64))


def test_guarded_batch_sees_a_byte_beside_an_output():
    """guarded_batch on a stand-in for a zada_*_batch call that copies every entry into its output: clean when it keeps to the caps, an
    AssertionError naming the entry when it writes one byte before or behind one of them."""
    datas = [b"abc", b"", b"0123456789", b"xy"]

    def fake(stray):
        def fn(cnt, ins, lens, outp, caps, ols, crcs, rcs):
            u64 = ctypes.POINTER(ctypes.c_uint64)
            ins, lens, outp, caps, ols = (ctypes.cast(p, u64) for p in (ins, lens, outp, caps, ols))
            for i in range(cnt):
                k = min(lens[i], caps[i])
                ctypes.memmove(outp[i], ins[i], k)
                ols[i] = k
                ctypes.cast(rcs, ctypes.POINTER(ctypes.c_int32))[i] = 0
            if stray is not None:
                i, off = stray
                ctypes.memset(outp[i] + (caps[i] if off >= 0 else 0) + off, 0, 1)
            return 0
        return fn
    worst, rcs, ols, crcs, outs = guarded_batch(fake(None), datas, [3, 0, 4, 16])
    assert worst == 0 and list(rcs) == [0] * 4 and list(ols) == [3, 0, 4, 2] and outs[2] == b"0123" and outs[3][:2] == b"xy"
    # (the guard in front of an entry is the guard behind the entry before it, which is the one named)
    for i, off, named in ((0, 0, 0), (1, 0, 1), (2, 15, 2), (3, 0, 3), (3, 15, 3), (0, -1, 0), (0, -16, 0), (3, -1, 2)):
        with pytest.raises(AssertionError, match="entry %d:" % named):
            guarded_batch(fake((i, off)), datas, [3, 0, 4, 16])


# ---- inputs and references, made once ----
def _text():
    if "text" not in _cache:
        _cache["text"] = silesia_mix((1 << 20) + 64, class_mask=1)
    return _cache["text"]


def _mix():
    if "mix" not in _cache:
        _cache["mix"] = silesia_mix(SPAN_LENGTH)
    return _cache["mix"]


def _random(n, seed=5):
    if ("rnd", n, seed) not in _cache:
        _cache["rnd", n, seed] = bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))
    return _cache["rnd", n, seed]


def _deflate_input(n):
    """n bytes of the synthetic corpus: its text class and the mix of all classes take turns along the list of lengths."""
    src = _mix() if (EDGE_LENGTHS + COPY_LENGTHS).index(n) % 2 else _text()
    return src[64:64 + n] if n + 64 <= len(src) else src[:n]


def _lzma_expected(data, method):
    from test_gpu_lzma_variants import expected          # (the data-type methods: the oracle's LZMA.Encoding.Encode with the method's lc, lp, pb)
    return expected(data, method)


def _ref(family, data, method):
    """(rc, stream) of the reference for `data`, kept: the tests share them."""
    key = (family, method, len(data), zlib.crc32(data))
    if key not in _cache:
        if family == "deflate":
            _cache[key] = _rich.deflate_r(data) if method == 11 else oracle_deflate(data, method)[:2]
        elif family == "bzip2":
            s = oracle_encode(data, method - 12)[0]
            _cache[key] = (1 if len(s) >= len(data) else 0, s)
        else:
            _cache[key] = (_lzma_expected if method > 18 else oracle_lzma)(data, method)[:2]
    return _cache[key]


def _reg(data, start):
    return zlib.crc32(data, start ^ FF) ^ FF


def _device(enc, family, method, data, cap, a_in=0, a_out=0, crc=FF, crc_null=False):
    """zada_<family>_device through the C ABI (a refused call is an rc, not an exception) -> (rc, out_len, CRC register, the cap output bytes)"""
    ol, c = ctypes.c_uint64(0), ctypes.c_uint32(crc)
    f = getattr(enc.lib, "zada_%s_device" % family)
    (rc, out) = device_call(lambda d_in, n, d_out, k: f(enc.ctx, method, d_in, n, d_out, k, ctypes.byref(ol), None if crc_null else ctypes.byref(c)),
                            data, cap, a_in, a_out)
    return rc, ol.value, c.value, out


def _check(enc, family, method, data, cap, a_in, a_out, crc=FF, what=None):
    """One device call that has to give the reference's result: rc, out_len, the bytes when they are delivered, zlib's register."""
    what = what or (family, method, len(data), cap, a_in, a_out)
    wrc, want = _ref(family, data, method)
    rc, ol, reg, out = _device(enc, family, method, data, cap, a_in, a_out, crc)
    assert rc == wrc, (what, rc, enc.lib.zada_last_error(enc.ctx))
    assert reg == _reg(data, crc), what
    delivered = rc == 0 or (family != "deflate" and len(want) <= cap)           # (zada.h: BZip2 and LZMA deliver an inefficient stream that fits)
    if delivered:
        assert ol == len(want) and ol <= cap and out[:ol] == want, what
    else:
        assert ol >= len(data), what                                              # (inefficient: not smaller than the input)
        if family == "bzip2":                                                     # (assembled only when it fits; Deflate may have written spans, LZMA writes as it goes)
            assert out == bytes([GUARD]) * cap, what
    return rc, ol


def _refused(enc, family, method, data, cap, a_in, a_out, what=None):
    """One device call with a cap the reference's stream -- smaller than the input -- does not fit: ZADA_E_INVALID, "too small"."""
    what = what or (family, method, len(data), cap, a_in, a_out)
    wrc, want = _ref(family, data, method)
    assert wrc == 0 and cap < len(want), what
    rc, ol, reg, out = _device(enc, family, method, data, cap, a_in, a_out)
    assert rc == E_INVALID and b"too small" in enc.lib.zada_last_error(enc.ctx), (what, rc)
    if family == "bzip2":                                                         # (assembled only when it fits; Deflate may have written spans, LZMA writes as it goes)
        assert out == bytes([GUARD]) * cap, what


# ---- 1 ----
@gpu
def test_deflate_device_alignments_and_guards(encoder):
    """Deflate_3 on 40 000 bytes at all 256 (a_in, a_out); every edge length and the incompressible input under methods 6 .. 11 at sixteen pairs each;
    the lengths around the 16-byte pieces of the shard copy on a caller's buffer of exactly n bytes, with the stream in one shard and in 1 MiB shards."""
    d = _deflate_input(40000)
    for k in range(256):
        assert _check(encoder, "deflate", 10, d, len(d) + 64, k % 16, (k // 16) % 16)[0] == 0
    cases = [_deflate_input(n) for n in EDGE_LENGTHS] + [_random(5000)]
    for i, d in enumerate(cases):
        for method in range(6, 12):
            for j in range(16):
                rc, _ = _check(encoder, "deflate", method, d, len(d) + 64, j, (7 * j + 3 + i + method) % 16)
                assert rc == 1 or d is not cases[-1]
    try:
        for shard_kib in (1 << 20, 1024):
            encoder.set_knob("shard_kib", shard_kib)
            for i, n in enumerate(COPY_LENGTHS):
                d = _deflate_input(n)
                for method in range(6, 12):
                    # (an aligned input is read where it lies: the buffer ends at n; an unaligned one goes through the context's own copy)
                    for a_in, a_out in ((0, (5 * method + i) % 16), (0, 0), (1 + (method + i) % 15, 3)):
                        assert _check(encoder, "deflate", method, d, n + 64, a_in, a_out, what=("shard_kib", shard_kib, method, n, a_in, a_out))[0] == 0
    finally:
        encoder.set_knob("shard_kib", 1 << 20)


# ---- 2 ----
@gpu
def test_deflate_device_exact_and_short_cap(encoder):
    """cap = the stream's length is enough and one byte less is ZADA_E_INVALID, with nothing written at or beyond cap and the context good for the
    next call; an incompressible input with cap = n is rc 1.  The same through deflate_spans (span_mib = 1, an aligned input of 3 MiB + 77: the
    spans are written into d_out one after the other) and through deflate_core on an unaligned input of that length."""
    k = 0
    for n in EDGE_LENGTHS + COPY_LENGTHS:
        d = _deflate_input(n)
        for method in (6, 10, 11):
            wrc, want = _ref("deflate", d, method)
            a_in, a_out = (0 if n >= 1 << 20 and k % 3 else k % 16), (k // 3) % 16
            k += 1
            if wrc == 0:
                _refused(encoder, "deflate", method, d, len(want) - 1, a_in, a_out)
                assert _check(encoder, "deflate", method, d, len(want), a_in, a_out)[0] == 0
            else:
                assert _check(encoder, "deflate", method, d, n, a_in, a_out)[0] == 1
    rnd = _random(5000)
    for method in (6, 10, 11):
        for a in range(0, 16, 5):
            assert _check(encoder, "deflate", method, rnd, len(rnd), a, 15 - a)[0] == 1
    try:
        encoder.set_knob("span_mib", 1)
        d = _mix()
        assert len(d) == SPAN_LENGTH
        for method in (6, 10, 11):
            wrc, want = _ref("deflate", d, method)
            assert wrc == 0
            for a_in in (0, 3):                               # deflate_spans, deflate_core
                a_out = (5 * method + a_in) % 16
                assert _check(encoder, "deflate", method, d, len(d) + 64, a_in, a_out)[0] == 0
                _refused(encoder, "deflate", method, d, len(want) - 1, a_in, a_out + 1)      # (spans already written are allowed, a byte at cap is not)
                assert _check(encoder, "deflate", method, d, len(want), a_in, a_out + 2)[0] == 0
        rnd = _random((1 << 20) + 4097)
        for method in (6, 10):
            for a_in in (0, 9):
                assert _check(encoder, "deflate", method, rnd, len(rnd), a_in, 7)[0] == 1
    finally:
        encoder.set_knob("span_mib", 2048)
    # the knob is back: the same stream in one pass
    assert _check(encoder, "deflate", 6, _mix(), len(_ref("deflate", _mix(), 6)[1]), 0, 13)[0] == 0


# ---- 3 ----
CRC_CASES = (("deflate", 10), ("bzip2", 14), ("lzma", 16))


@gpu
def test_crc_register_is_running(encoder):
    """crc_inout is the running register: started anywhere it ends where zlib's does; with n = 0 it stays; NULL is allowed."""
    for family, method in CRC_CASES:
        for n in (0, 4097, 40000):
            d = _mix()[1000:1000 + n]
            for k, start in enumerate((0, 0x12345678, FF)):
                rc, ol, reg, out = _device(encoder, family, method, d, n + n // 4 + 4096, 3 * k, 5 * k + 1, crc=start)
                wrc, want = _ref(family, d, method)
                assert rc == wrc and reg == _reg(d, start), (family, n, hex(start))
                if n == 0:
                    assert reg == start
                if rc == 0 or family != "deflate":
                    assert out[:ol] == want, (family, n, hex(start))
            rc, ol, reg, out = _device(encoder, family, method, d, n + n // 4 + 4096, 2, 9, crc=0x600DF00D, crc_null=True)
            assert rc == wrc and reg == 0x600DF00D, (family, n)
            if rc == 0 or family != "deflate":
                assert ol == len(want) and out[:ol] == want, (family, n)


# ---- 4 ----
def _bz_inputs(method):
    """Four small texts whose streams' lengths take all four values modulo 4, random bytes, and one long input: three blocks under BZip2_1,
    a block that BZip2_3 cuts into sub-blocks."""
    if ("bz", method) not in _cache:
        small = {}
        for j in range(40):
            d = _text()[:1000 + 37 * j]
            small.setdefault(len(_ref("bzip2", d, method)[1]) % 4, d)
        assert sorted(small) == [0, 1, 2, 3]
        rng = np.random.default_rng(11)
        seg = bytes(np.concatenate([rng.integers(97, 123, 100000, dtype=np.uint8), rng.integers(48, 58, 100000, dtype=np.uint8),
                                    rng.integers(97, 101, 60000, dtype=np.uint8)]))
        _cache["bz", method] = ([small[r] for r in range(4)], _random(3000), seg)
    return _cache["bz", method]


@gpu
@pytest.mark.parametrize("method", [12, 13, 14])
def test_bzip2_device_alignments_and_caps(encoder, method):
    """bz_assemble_range writes whole words into a 4-byte aligned d_out that holds them and copies the bytes otherwise: every alignment of the
    output under a generous cap, the stream's length rounded up to 4, the length itself and one byte less."""
    small, rnd, seg = _bz_inputs(method)
    ev = oracle_encode(seg, method - 12)[1]
    assert (len(ev) == 3) if method == 12 else (len(ev) == 1 and (ev[0][3] > 1) == (method == 14)), ev
    exact_residues = set()
    k = 0
    for a_out in range(16):
        for kind in range(4):
            # the long input at eight of the sixty-four places, among them aligned and unaligned outputs under every kind of cap
            d = seg if (a_out, kind) in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 2), (2, 1), (4, 2), (7, 3)) else small[(a_out + kind) % 4]
            a_in = (0, 1, 7, 15)[k % 4]
            k += 1
            n_out = len(_ref("bzip2", d, method)[1])
            if kind == 3:
                _refused(encoder, "bzip2", method, d, n_out - 1, a_in, a_out)
                continue
            cap = (len(d) + len(d) // 4 + 4096, (n_out + 3) & ~3, n_out)[kind]
            assert _check(encoder, "bzip2", method, d, cap, a_in, a_out)[0] == 0
            if kind == 2 and a_out % 4 == 0:
                exact_residues.add(n_out % 4)
    # (aligned output, exact cap: the direct branch when the length is a multiple of 4, the copy branch for the other three)
    for r in range(4):
        assert _check(encoder, "bzip2", method, small[r], len(_ref("bzip2", small[r], method)[1]), (0, 1, 7, 15)[r], 8)[0] == 0
        exact_residues.add(r)
    assert exact_residues == {0, 1, 2, 3}
    # random bytes: the stream is longer than the input -- rc 1, delivered where it fits and not otherwise
    n_out = len(_ref("bzip2", rnd, method)[1])
    assert n_out > len(rnd)
    for a_out in range(16):
        a_in = (0, 1, 7, 15)[a_out % 4]
        for cap in (n_out + 100, n_out, n_out - 1, len(rnd)):
            assert _check(encoder, "bzip2", method, rnd, cap, a_in, a_out)[0] == 1
    # a cap below 64 bytes is a cap like any other: the stream of an empty entry and of one byte (rc 1: not smaller than the input) is delivered
    # into exactly its length, and cap = n is enough for the verdict
    for d in (b"", b"z"):
        n_out = len(_ref("bzip2", d, method)[1])
        assert n_out < 64
        for a_out in (0, 1, 2, 3, 4, 9):
            assert _check(encoder, "bzip2", method, d, n_out, a_out, a_out)[0] == 1
            assert _check(encoder, "bzip2", method, d, n_out - 1, 0, a_out)[0] == 1
            assert _check(encoder, "bzip2", method, d, len(d), 0, a_out)[0] == 1
    d = small[0][:400]                                         # ... and for a stream smaller than its input that needs more, 63 bytes are "too small"
    wrc, want = _ref("bzip2", d, method)
    assert wrc == 0 and len(want) > 64
    _refused(encoder, "bzip2", method, d, 63, 0, 0)
    assert _check(encoder, "bzip2", method, d, len(want), 0, 0)[0] == 0


# ---- 5 ----
# LZMA_0, LZMA_1, LZMA_3 (BT4), LZMA_for_JPEG (level 2, literal table of lc = 8 in HBM), LZMA_3_for_Zip_in_Zip (BT4, 6 MiB table in HBM),
# LZMA_for_WAV (level 2, lc + lp = 1: the data-type methods' table in LDS)
LZMA_CASES = (15, 16, 18, 23, 20, 32)


@gpu
@pytest.mark.parametrize("method", LZMA_CASES)
def test_lzma_device_alignments_and_caps(encoder, method):
    """The coder writes into the caller's d_out byte by byte; put_byte counts the bytes beyond cap and does not write them.  Sixteen
    (a_in, a_out) pairs under a generous cap, the payload's length, one byte less (ZADA_E_INVALID) and, on random bytes, cap = n (rc 1 with
    the oracle's length reported)."""
    level3 = method in (18, 20)
    small = _mix()[5000:5000 + (3001 if level3 else 9001)]
    rnd = _random(2000)
    n_small, n_rnd = len(_ref("lzma", small, method)[1]), len(_ref("lzma", rnd, method)[1])
    assert _ref("lzma", small, method)[0] == 0 and n_rnd > len(rnd)
    for j in range(16):
        a_in, a_out = j, (7 * j + 3 + method) % 16
        assert _check(encoder, "lzma", method, small, len(small) + 4096, a_in, a_out)[0] == 0
        assert _check(encoder, "lzma", method, small, n_small, a_in, a_out)[0] == 0
        _refused(encoder, "lzma", method, small, n_small - 1, a_in, a_out)
        rc, ol = _check(encoder, "lzma", method, rnd, len(rnd), a_in, a_out)
        assert rc == 1 and ol == n_rnd
    assert _check(encoder, "lzma", method, rnd, n_rnd, 5, 11)[0] == 1                 # (it fits: delivered)
    assert _check(encoder, "lzma", method, b"", 64, 0, 5) == (1, len(_ref("lzma", b"", method)[1]))
    assert _check(encoder, "lzma", method, b"", 0, 0, 6)[0] == 1
    # the longest input of the family, at two pairs: one stream runs at one wave's pace, so level 3 gets 20 000 bytes and the others 100 000
    big = _mix()[:20000 if level3 else 100000]
    n_big = len(_ref("lzma", big, method)[1])
    assert _check(encoder, "lzma", method, big, n_big, 0, 9)[0] == 0
    _refused(encoder, "lzma", method, big, n_big - 1, 13, 2)


# ---- 6 ----
@gpu
def test_crc32_device(encoder):
    """The raw register of zada_crc32_device, chained with zada_crc32_combine (pinned against zlib on the host, test_host_asan.py), against zlib:
    around every fold level (256 B, 4 KiB, 64 KiB, 1 MiB, and the host's chain beyond 16 MiB), around the 16 KiB tile of k_crc_chunks, every
    n % 16 at the end of a tile; the buffer ends at n."""
    import torch
    lengths = [0, 1, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 65535, 65536, 65537, (1 << 20) - 1, 1 << 20, (1 << 20) + 1,
               (16 << 20) + 255, (17 << 20) + 4096 + 3]
    lengths += [2 * 16384 + r for r in range(1, 16)] + [3 * 16384 - 16 + r for r in range(1, 16)]
    base = silesia_mix(max(lengths))
    g_base = torch.frombuffer(bytearray(base), dtype=torch.uint8).cuda()
    raw = ctypes.c_uint32(0)

    def crc_of(t, n):
        torch.cuda.synchronize()
        raw.value = 0xDEADBEEF
        rc = encoder.lib.zada_crc32_device(encoder.ctx, t.data_ptr() if n else None, n, ctypes.byref(raw))
        assert rc == 0, (n, rc, encoder.lib.zada_last_error(encoder.ctx))
        return encoder.lib.zada_crc32_combine(FF, raw.value, n) ^ FF
    for n in lengths:
        t = g_base[:n].clone()                                 # an allocation of its own: the buffer ends at n
        assert t.numel() == n and t.data_ptr() % 16 == 0
        assert crc_of(t, n) == zlib.crc32(base[:n]), n
        if n == 0:
            assert raw.value == 0
    for n in (257, 65537, (1 << 20) + 1):
        for v in (0, 0xFF):
            t = torch.full((n,), v, dtype=torch.uint8, device="cuda")
            assert crc_of(t, n) == zlib.crc32(bytes([v]) * n), (n, v)
    # an address that is not 16-byte aligned is refused before anything is read
    t = g_base[:4096 + 16].clone()
    for a in (1, 4, 8, 15):
        raw.value = 0x5EED
        assert encoder.lib.zada_crc32_device(encoder.ctx, t.data_ptr() + a, 4096, ctypes.byref(raw)) == E_INVALID and raw.value == 0x5EED, a
    assert encoder.lib.zada_crc32_device(encoder.ctx, t.data_ptr(), 4096, None) == E_INVALID
    assert crc_of(t, 4096) == zlib.crc32(base[:4096])


# ---- 7 ----
def _batch_entries():
    """About 200 entries of 0 .. 40 000 bytes: texts and mixes of all sizes with empty, one-byte and random entries between them."""
    if "batch" not in _cache:
        rng = np.random.default_rng(23)
        sizes = [0, 1, 2, 7, 100, 333, 1000, 2048, 3000, 4097, 800, 5000, 64, 12000, 1500, 600] * 12 + [40000, 32768, 32769, 20000]
        out = []
        for i, n in enumerate(sizes):
            if i % 5 == 3:
                out.append(bytes(rng.integers(0, 256, max(n, 40) if i % 10 == 3 else n, dtype=np.uint8)))
            else:
                src = _text() if i % 2 else _mix()
                o = int(rng.integers(0, len(src) - 40000))
                out.append(src[o:o + n])
        _cache["batch"] = out
    return _cache["batch"]


@gpu
@pytest.mark.parametrize("family,method", [("deflate", 10), ("bzip2", 14), ("lzma", 18), ("lzma", 16)])
def test_batches_respect_their_caps(encoder, family, method):
    """zada_deflate_batch / zada_bzip2_batch / zada_lzma_batch (LZMA_3: lzma_batch_core, LZMA_1: lzma_batch_iz) on an arena with guard bytes on both
    sides of every output, the caps cycling through generous, exact and one byte short: rc per entry as zada.h states it, every delivered entry
    the oracle's, the return value the worst rc."""
    datas = _batch_entries()
    assert len(datas) == 196
    refs = [_ref(family, d, method) for d in datas]
    caps = [(len(d) + len(d) // 4 + 1024, len(s), max(len(s) - 1, 0))[i % 3] for i, (d, (_, s)) in enumerate(zip(datas, refs))]
    f = getattr(encoder.lib, "zada_%s_batch" % family)
    worst, rcs, ols, crcs, outs = guarded_batch(lambda *a: f(encoder.ctx, method, *a), datas, caps)
    seen = set()
    for i, (d, (wrc, want), cap) in enumerate(zip(datas, refs, caps)):
        fits = len(want) <= cap
        if family == "deflate":
            # 0, or 1 = inefficient (nothing delivered, whatever cap is), or ZADA_E_INVALID for a stream smaller than the input that does not fit
            exp = 1 if wrc == 1 else 0 if fits else E_INVALID
            delivered = exp == 0
        else:
            # zada_bzip2's / zada_lzma's code: the verdict 0 / 1 with the stream delivered whenever it fits cap; smaller than the input and not fitting is ZADA_E_INVALID
            exp = wrc if (fits or wrc == 1) else E_INVALID
            delivered = fits
        assert rcs[i] == exp, (i, len(d), cap, int(rcs[i]), exp)
        assert crcs[i] == _reg(d, FF), i
        if delivered:
            assert int(ols[i]) == len(want) and outs[i][:len(want)] == want, (i, len(d), cap)
        seen.add((i % 3, exp))
    assert worst == min(min(int(r) for r in rcs), 0)
    assert {(0, 0), (1, 0), (2, E_INVALID), (0, 1), (1, 1), (2, 1)} <= seen          # every kind of cap met compressible and incompressible entries
