"""What the tests of the stream readers share (test_gpu_inflate.py, test_gpu_bunzip2.py, test_gpu_unlzma.py; test_reader_plan.py): the group plan of
the batch calls restated in Python, the argument checks of the three entry points of a reader through the C ABI, and one batch that takes several
launch groups.  The readers are told apart by name: "inflate", "bunzip2", "unlzma"."""
import bz2
import ctypes
import zlib

import numpy as np
import pytest

from _common import product, silesia_mix

E_DATA, E_INVALID, E_TOO_LARGE = -7, -1, -4
TIB = 1 << 40


# ---- the group plan (csrc/zada_reader_plan.h), restated ----
def pad16(x):
    return (x + 15) & ~15


def plan_groups(n_in, caps, limit):
    """[(g0, g1, in_bytes, out_bytes)]: a group takes entries g0 .. g1 - 1, its inputs then its outputs in one arena, every buffer at a multiple of
    16; the first entry is always taken, the group ends in front of the entry with which inputs and outputs would exceed `limit`."""
    groups, g0, count = [], 0, len(n_in)
    while g0 < count:
        g1, in_bytes, out_bytes = g0, 0, 0
        while g1 < count:
            a, b = pad16(int(n_in[g1])), pad16(int(caps[g1]))
            if g1 > g0 and in_bytes + out_bytes + a + b > limit:
                break
            in_bytes, out_bytes, g1 = in_bytes + a, out_bytes + b, g1 + 1
        groups.append((g0, g1, in_bytes, out_bytes))
        g0 = g1
    return groups


def plan_offsets(n_in, caps, group):
    """([io], [oo]) of the entries of one group of plan_groups: where the input and the output of each lie in the group's arena."""
    g0, g1, in_bytes, _ = group
    io, oo, a, b = [], [], 0, in_bytes
    for i in range(g0, g1):
        io.append(a)
        oo.append(b)
        a, b = a + pad16(int(n_in[i])), b + pad16(int(caps[i]))
    return io, oo


def plan_extent(oo, in_bytes, ok_len):
    """The bytes of a group's outputs that come back in one piece: up to the last byte any entry wrote (ok_len [k]: what entry k wrote, 0 where it
    failed), counted from the first output."""
    hi = 0
    for o, n in zip(oo, ok_len):
        if n:
            hi = o + n - in_bytes
    return hi


# ---- one reader's three entry points of the C ABI, the format-specific arguments spliced in ----
class ABI:
    def __init__(self, lib, name):
        self.lib, self.name = lib, name

    def device(self, ctx, d_in, n_in, d_out, cap, ol, iu, crc, extra=None):
        return self._one(getattr(self.lib, "zada_%s_device" % self.name), ctx, d_in, n_in, d_out, cap, ol, iu, crc, extra)

    def single(self, ctx, p_in, n_in, p_out, cap, ol, iu, crc, extra=None):
        return self._one(getattr(self.lib, "zada_%s" % self.name), ctx, p_in, n_in, p_out, cap, ol, iu, crc, extra)

    def _one(self, fn, ctx, p_in, n_in, p_out, cap, ol, iu, crc, extra):
        if self.name == "inflate":
            return fn(ctx, 8 if extra is None else extra, p_in, n_in, p_out, cap, ol, iu, crc)
        if self.name == "unlzma":
            return fn(ctx, p_in, n_in, p_out, cap, 1 if extra is None else extra, ol, iu, crc)
        return fn(ctx, p_in, n_in, p_out, cap, ol, iu, crc)

    def batch(self, ctx, count, ins, lens, outs, caps, extra, ols, ius, crcs, rcs):
        fn = getattr(self.lib, "zada_%s_batch" % self.name)
        if self.name == "inflate":
            return fn(ctx, count, extra, ins, lens, outs, caps, ols, ius, crcs, rcs)
        if self.name == "unlzma":
            return fn(ctx, count, ins, lens, outs, caps, extra, ols, ius, crcs, rcs)
        return fn(ctx, count, ins, lens, outs, caps, ols, ius, crcs, rcs)


FORMAT_TEXT = ": format must be 8 (Deflate) or 9 (Deflate64)"
NULL_TEXT, TIB_TEXT = ": null buffer", ": a stream or an output of 1 TiB or more"


def argument_checks(encoder, name):
    """Every refusal of zada_<name>_device, zada_<name>_batch and zada_<name> that comes before any work: return code, exact error text, the order of
    the checks, and what the refused call leaves in out_len, in_used, the CRC register and the per-entry arrays.  No stream is decoded."""
    import torch
    lib, ctx = encoder.lib, encoder.ctx
    abi = ABI(lib, name)
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    host = ctypes.create_string_buffer(64)
    err = lambda: lib.zada_last_error(ctx).decode()
    who = {"device": "zada_%s_device" % name, "single": "zada_%s" % name, "batch": "zada_%s_batch" % name}

    def one(kind, c, p_in, n_in, p_out, cap, extra=None):
        ol, iu, reg = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(0x1234)
        rc = getattr(abi, kind)(c, p_in, n_in, p_out, cap, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg), extra)
        return rc, ol.value, iu.value, reg.value

    untouched = (77, 77, 0x1234)
    for kind, p in (("device", t.data_ptr()), ("single", ctypes.addressof(host))):
        w = who[kind]
        assert one(kind, None, p, 8, p + 32, 8) == (E_INVALID,) + untouched
        assert one(kind, ctx, None, 5, p, 5) == (E_INVALID,) + untouched and err() == w + NULL_TEXT
        assert one(kind, ctx, p, 5, None, 5) == (E_INVALID,) + untouched and err() == w + NULL_TEXT
        assert one(kind, ctx, None, TIB, p, 5) == (E_INVALID,) + untouched and err() == w + NULL_TEXT               # the null buffer before the size
        if name == "inflate":
            for fmt in (0, 7, 10, -8):
                assert one(kind, ctx, p, 8, p + 32, 8, fmt) == (E_INVALID,) + untouched and err() == w + FORMAT_TEXT
            assert one(kind, ctx, None, 5, None, 5, 7) == (E_INVALID,) + untouched and err() == w + FORMAT_TEXT     # the format before the null buffer
            assert one(kind, None, p, 8, p + 32, 8, 7) == (E_INVALID,) + untouched
        # 1 TiB: the device call refuses before it clears out_len and in_used, the single call clears them and hears it from the batch call
        for n_in, cap in ((TIB, 8), (8, TIB), ((1 << 64) - 8, 8)):
            if kind == "device":
                assert one(kind, ctx, p, n_in, p + 32, cap) == (E_TOO_LARGE,) + untouched and err() == w + TIB_TEXT
            else:
                assert one(kind, ctx, p, n_in, p + 32, cap) == (E_TOO_LARGE, 0, 0, 0x1234) and err() == who["batch"] + TIB_TEXT
        # every result pointer may be null
        assert getattr(abi, kind)(ctx, None, 5, p, 5, None, None, None) == E_INVALID and err() == w + NULL_TEXT

    w = who["batch"]
    good = ctypes.addressof(host)

    def batch(c, count, ins, lens, outs, caps, extra="default", drop=()):
        """-> rc; asserts that the refused call wrote to none of the per-entry arrays.  ins / outs: addresses or None per entry; outs = None: no
        array; drop: names of the arrays to pass as null."""
        n = len(ins)
        a = {"ins": np.array([x or 0 for x in ins], dtype=np.uint64), "lens": np.array(lens, dtype=np.uint64),
             "outs": None if outs is None else np.array([x or 0 for x in outs], dtype=np.uint64), "caps": np.array(caps, dtype=np.uint64),
             "ols": np.full(n, 77, np.uint64), "ius": np.full(n, 77, np.uint64), "crcs": np.full(n, 0x1234, np.uint32), "rcs": np.full(n, 99, np.int32)}
        if name == "inflate":
            a["extra"] = np.full(n, 8, np.int32) if isinstance(extra, str) else np.array(extra, dtype=np.int32)
        elif name == "unlzma":
            a["extra"] = np.ones(n, np.int32)
        else:
            a["extra"] = None
        ptr = {k: (None if v is None or k in drop else v.ctypes.data) for k, v in a.items()}
        rc = abi.batch(c, count, ptr["ins"], ptr["lens"], ptr["outs"], ptr["caps"], ptr["extra"], ptr["ols"], ptr["ius"], ptr["crcs"], ptr["rcs"])
        assert (a["ols"] == 77).all() and (a["ius"] == 77).all() and (a["crcs"] == 0x1234).all() and (a["rcs"] == 99).all()
        return rc

    o = [good + 32]
    assert batch(None, 1, [good], [8], o, [8]) == E_INVALID
    assert batch(ctx, 1, [None], [5], o, [5]) == E_INVALID and err() == w + NULL_TEXT
    before = err()
    assert batch(ctx, -1, [good], [8], o, [8]) == E_INVALID and err() == before                    # (no text of its own)
    assert abi.batch(ctx, 0, None, None, None, None, None, None, None, None, None) == 0 and err() == before
    assert batch(ctx, 0, [good], [TIB], o, [8]) == 0                                                # count = 0 looks at no entry
    mandatory = ("ins", "lens", "caps", "rcs") + (("extra",) if name != "bunzip2" else ())
    for k in mandatory:
        assert batch(ctx, 1, [None], [5], o, [5], drop=(k,)) == E_INVALID and err() == w + ": null argument", k
    assert abi.batch(ctx, 1, None, None, None, None, None, None, None, None, None) == E_INVALID and err() == w + ": null argument"
    # out, out_len, in_used and crc may be null: the call goes on to the entries
    assert batch(ctx, 1, [None], [5], None, [5], drop=("ols", "ius", "crcs")) == E_INVALID and err() == w + NULL_TEXT
    assert batch(ctx, 1, [good], [8], [None], [5]) == E_INVALID and err() == w + NULL_TEXT
    for lens, caps in (([TIB], [8]), ([8], [TIB]), ([8], [(1 << 64) - 8])):
        assert batch(ctx, 1, [good], lens, o, caps) == E_TOO_LARGE and err() == w + TIB_TEXT
    assert batch(ctx, 1, [good], [8], None, [TIB]) == E_TOO_LARGE and err() == w + TIB_TEXT         # no output array: the cap is still looked at
    # the order: entry by entry, and in an entry the format, the null buffer, the size
    two_o = [good + 32, good + 48]
    assert batch(ctx, 2, [good, None], [TIB, 5], two_o, [8, 8]) == E_TOO_LARGE and err() == w + TIB_TEXT
    assert batch(ctx, 2, [None, good], [5, TIB], two_o, [8, 8]) == E_INVALID and err() == w + NULL_TEXT
    assert batch(ctx, 1, [None], [TIB], o, [8]) == E_INVALID and err() == w + NULL_TEXT
    if name == "inflate":
        for fmt in (0, 7, 10, -8):
            assert batch(ctx, 2, [good, good], [8, 8], two_o, [8, 8], extra=[8, fmt]) == E_INVALID and err() == w + FORMAT_TEXT
        assert batch(ctx, 1, [None], [TIB], o, [8], extra=[7]) == E_INVALID and err() == w + FORMAT_TEXT
        assert batch(ctx, 2, [None, good], [5, 8], two_o, [8, 8], extra=[8, 7]) == E_INVALID and err() == w + NULL_TEXT
        assert batch(ctx, 2, [good, good], [TIB, 8], two_o, [8, 8], extra=[9, 7]) == E_TOO_LARGE and err() == w + TIB_TEXT

    # the Python wrappers
    za = product()
    call = getattr(encoder, name + "_batch")
    assert call([], []) == []
    size_text = {"inflate": "inflate_batch: one size and one format per payload", "bunzip2": "bunzip2_batch: one size per payload",
                 "unlzma": "unlzma_batch: one cap per payload"}[name]
    for sizes in ([4], [4, 4, 4]):
        with pytest.raises(za.ZadaError) as e:
            call([b"ab", b"ab"], sizes)
        assert str(e.value) == size_text
    if name == "inflate":
        with pytest.raises(za.ZadaError) as e:
            call([b"ab", b"ab"], [4, 4], [8])
        assert str(e.value) == size_text
    if name == "unlzma":
        with pytest.raises(za.ZadaError) as e:
            call([b"ab", b"ab"], [4, 4], [True])
        assert str(e.value) == "unlzma_batch: one eos flag per payload"
    for deliver in (True, False):
        with pytest.raises(za.ZadaError) as e:
            call([b"ab", b"ab"], [1 << 39, 1 << 39], deliver=deliver)
        assert str(e.value) == "%s_batch: %d bytes of output are promised -- more than this machine holds" % (name, TIB)


# ---- one batch through several launch groups ----
START = 0x1234ABCD                # the register every entry starts from
_groups_cache = {}


def _encode(name, data):
    if name == "inflate":
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        return c.compress(data) + c.flush()
    if name == "bunzip2":
        return bz2.compress(data, 1)
    import _unlzma
    return _unlzma.raw_payload(data)


def _reference(name, payload, cap):
    """zlib / bz2 / lzma on one payload -> (bytes, input bytes used), or None where the library refuses it (or it writes more than cap)."""
    try:
        if name == "inflate":
            d = zlib.decompressobj(-15)
            out = d.decompress(payload)
        elif name == "bunzip2":
            d = bz2.BZ2Decompressor()
            out = d.decompress(payload) if payload else b""
        else:
            import _unlzma
            v = _unlzma.lzma_verdict(payload, cap, True) if len(payload) >= 9 else ("error",)
            return (v[1], v[2]) if v[0] == "accepted" else None
    except (zlib.error, OSError, ValueError, EOFError):
        return None
    if not d.eof or len(out) > cap:
        return None
    return out, len(payload) - len(d.unused_data)


def group_entries(name):
    """(limit, payloads, caps, expected, damaged): 42 entries with small caps, one whose own cap exceeds the group limit, a zero-length payload at the
    end and one damaged stream in the second group.  expected [i] = (bytes, input bytes used) by the reference library, None where it refuses."""
    if name in _groups_cache:
        return _groups_cache[name]
    limit, small = ((8 << 20), (512 << 10)) if name == "bunzip2" else ((1 << 20), (64 << 10))
    top = 60000 if name == "bunzip2" else small
    datas = [silesia_mix(1 + (k * 7919 + 13) % top, offset=k * 70001) for k in range(42)]
    caps = [small] * 42
    datas.insert(20, silesia_mix(100003, offset=5 << 20))
    caps.insert(20, limit + 4096)
    payloads = [_encode(name, d) for d in datas] + [b""]
    caps.append(small)
    groups = plan_groups([len(p) for p in payloads], caps, limit)
    assert len(groups) >= 3 and sum(pad16(len(p)) + c for p, c in zip(payloads, caps)) > 3 * limit
    assert (20, 21) in [g[:2] for g in groups], "the entry whose cap exceeds the limit is a group by itself"
    damaged = groups[1][0] + 1
    assert damaged < groups[1][1] and damaged != 20
    s = bytearray(payloads[damaged])
    if name == "inflate":
        s[0] = 0x07                                   # a final block of the reserved type
    elif name == "bunzip2":
        s[len(s) // 2] ^= 0x10                        # inside the block: its CRC no longer holds
    else:
        s[9] = 0x01                                   # the range coder's first byte is not zero
    payloads[damaged] = bytes(s)
    expected = [_reference(name, p, c) for p, c in zip(payloads, caps)]
    assert expected[damaged] is None and expected[-1] is None and all(e is not None and e[0] == d for e, d in list(zip(expected, datas))[:damaged])
    assert [i for i, e in enumerate(expected) if e is None] == [damaged, len(payloads) - 1]
    _groups_cache[name] = (limit, payloads, caps, expected, damaged)
    return _groups_cache[name]


def several_launch_groups(encoder, name):
    limit, payloads, caps, expected, damaged = group_entries(name)
    knob, small, usual = ("bunzip_batch_mib", 16, 8192) if name == "bunzip2" else ("batch_mib", 1, 512)
    assert (small << 20) // (2 if name == "bunzip2" else 1) == limit
    call = getattr(encoder, name + "_batch")
    word = name.encode() + b": entry %d: " % damaged
    encoder.set_knob(knob, small)
    try:
        for deliver in (True, False):
            res = call(payloads, caps, crc=START, deliver=deliver)
            err = encoder.lib.zada_last_error(encoder.ctx)
            entry_recs = getattr(encoder, name + "_last_records")() if name != "inflate" else None
            block_recs = encoder.bunzip2_last_records(blocks=True) if name == "bunzip2" else None
            assert len(res) == len(payloads)
            for i, (want, (rc, out, ol, used, reg)) in enumerate(zip(expected, res)):
                if want is None:
                    assert (rc, out, ol, used, reg) == (E_DATA, None, 0, 0, START), (i, deliver)
                else:
                    assert (rc, ol, used) == (0, len(want[0]), want[1]) and reg == zlib.crc32(want[0], START ^ 0xFFFFFFFF) ^ 0xFFFFFFFF, (i, deliver)
                    assert out == (want[0] if deliver else None), (i, deliver)
            assert word in err, err                   # the first entry that failed, under its number in the call and not in its group
            if entry_recs is not None:
                assert entry_recs.shape == (len(payloads), 4)
                assert [i for i in range(len(payloads)) if entry_recs[i, 0]] == [i for i, e in enumerate(expected) if e is None]
            if block_recs is not None:
                # (the damaged entry's block was read before its CRC failed: it may be among them)
                assert {int(x) for x in block_recs[:, 0]} - {damaged} == {i for i, e in enumerate(expected) if e is not None and len(e[0])}
    finally:
        encoder.set_knob(knob, usual)
