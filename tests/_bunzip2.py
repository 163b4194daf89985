"""Helpers of the BZip2 reader's tests: loader of the CPU model (tests/bunzip2/bunzip2_host.cpp = zip-ada_amd/csrc/zada_bunzip2_logic.h with one lane
and serial later stages), the corpora of valid and damaged streams, libbz2's verdict on a stream, and a small block writer for crafted streams."""
import bz2
import ctypes
import json
import os
import subprocess

import numpy as np

from _common import GOLDEN, ROOT, edge_inputs

E_DATA = -7
_cache = {}
_DIR = os.path.join(ROOT, "tests", "bunzip2")
_SRC = os.path.join(_DIR, "bunzip2_host.cpp")
_HDR = os.path.join(ROOT, "zip-ada_amd", "csrc", "zada_bunzip2_logic.h")
BLOCK_MAGIC, FOOTER_MAGIC = 0x314159265359, 0x177245385090


def build_model(asan=False):
    p = os.path.join(_DIR, "libbunzip2_host_asan.so" if asan else "libbunzip2_host.so")
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if asan else ["-O2"]
        subprocess.run(["g++"] + flags + ["-std=c++17", "-fPIC", "-shared", "-o", p, _SRC], check=True)
    return p


def load_model(path):
    M = ctypes.CDLL(path)
    M.bm_bunzip2.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    M.bm_rule_name.restype = ctypes.c_char_p
    M.bm_rule_name.argtypes = [ctypes.c_uint]
    return M


def model():
    if "m" not in _cache:
        _cache["m"] = load_model(build_model())
    return _cache["m"]


def model_bunzip2(stream, cap, crc=0xFFFFFFFF, M=None, records=0):
    """-> (rc, bytes, out_len, in_used, crc register, rule name[, per-block records (symbols, origin, stored CRC, end bit)]).  The buffers are
    exact-size heap copies, so that a sanitizer sees a byte too many."""
    M = M or model()
    src = np.frombuffer(bytes(stream), dtype=np.uint8).copy() if len(stream) else np.zeros(0, np.uint8)
    out = np.empty(cap, dtype=np.uint8)
    res = (ctypes.c_uint64 * 8)()
    rec = np.zeros((max(records, 1), 4), dtype=np.uint64)
    rc = M.bm_bunzip2(src.ctypes.data if len(src) else None, len(src), out.ctypes.data if cap else None, cap, crc, res, rec.ctypes.data if records else None, records)
    r = (rc, out[:res[0]].tobytes(), int(res[0]), int(res[1]), int(res[4]), M.bm_rule_name(int(res[2])).decode())
    return r + (rec[:min(int(res[6]), records)],) if records else r


def bz2_verdict(stream, cap):
    """libbz2 on one stream -> ("accepted", bytes, in_used) | ("error",) | ("not_eof",) | ("over_cap",)"""
    d = bz2.BZ2Decompressor()
    try:
        out = d.decompress(stream, cap + 1)
    except OSError:
        return ("error",)
    if len(out) > cap:
        return ("over_cap",)
    if not d.eof:
        return ("not_eof",)
    return ("accepted", out, len(stream) - len(d.unused_data))


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def reference_payload():
    """The BZip2 payload of the reference's test/many_formats.zip: (payload, size, crc32, sha256)."""
    with open(os.path.join(GOLDEN, "many_formats_bzip2.json")) as f:
        e = json.load(f)["entries"][0]
    return golden(e["file"]), e["size"], int(e["crc32"], 16), e["sha256"]


def valid_inputs():
    """name -> bytes: the inputs the issue lists."""
    d = {"sample.xls": golden("sample.xls"), "sample.jpg": golden("sample.jpg"), "sample_pgm_100k.bin": golden("sample_pgm_100k.bin")}
    d.update(edge_inputs())
    for k in range(6):
        d["size%d" % k] = bytes(range(65, 65 + k))
    for k in (3, 4, 5, 258, 259, 260, 520):
        d["run%d" % k] = b"r" * k
    d.update({"count_is_value_1x5": b"\x01" * 5, "count_is_value_0x4": b"\x00" * 4, "count_is_value_fbx255": b"\xfb" * 255,
              "all256": bytes(range(256)) * 3, "one_value": b"q" * 70000})
    return d


def three_blocks():
    """250 000 bytes whose level-1 stream has three blocks that start off byte boundaries."""
    from _common import silesia_mix
    return silesia_mix(250000)


def valid_streams(oracle=True, product_encoder=None):
    """Yields (label, original bytes, BZip2 stream): every input through bz2.compress at levels 1 and 9 and the three BZip2 methods -- of the
    oracle, or of the product (on the GPU, bit for bit the oracle's: test_gpu_bzip2.py) where an encoder is given."""
    for name, data in valid_inputs().items():
        for lv in (1, 9):
            yield "%s/bz2.%d" % (name, lv), data, bz2.compress(data, lv)
        if len(data) == 0:                             # (the reference's writer makes a block with no symbols of no bytes: empty_block_streams)
            continue
        if product_encoder is not None:
            for m in (12, 13, 14):
                rc, s, _ = product_encoder.bzip2(data, m)
                assert rc in (0, 1) and s is not None      # (1: not smaller than the input -- the stream is there all the same)
                yield "%s/BZip2_%d" % (name, m - 11), data, s
        elif oracle:
            from _bzip2 import oracle_encode
            for opt in (0, 1, 2):
                yield "%s/BZip2_%d" % (name, opt + 1), data, oracle_encode(data, opt)[0]
    d = three_blocks()
    yield "three_blocks/bz2.1", d, bz2.compress(d, 1)
    p, size, crc, sha = reference_payload()
    yield "reference/$15_bzp2.tmp", None, p


def empty_block_streams():
    """What the reference's three BZip2 methods write for an entry of no bytes: a stream with one block of no symbols and no byte value in use, which
    libbz2 refuses (nInUse = 0) -- and so does this reader, by the same rule."""
    from _bzip2 import oracle_encode
    return [oracle_encode(b"", opt)[0] for opt in (0, 1, 2)]


def damaged_corpus():
    """The 20 000 damaged streams of the issue, deterministic: list of (stream, cap, kind); kind 3 is a pure truncation."""
    from _bzip2 import oracle_encode
    bases = []
    for name in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin"):
        d = golden(name)[:30000]
        for lv in (1, 9):
            bases.append((bz2.compress(d, lv), 2 * len(d)))
        for opt in (0, 1, 2):
            bases.append((oracle_encode(d, opt)[0], 2 * len(d)))
    rng = np.random.default_rng(1)
    cases = []
    for k in range(20000):
        s, cap = bases[k % len(bases)]
        kind = k % 4
        if kind == 3:
            cases.append((s[:int(rng.integers(0, len(s)))], cap, kind))
            continue
        pos = int(rng.integers(0, min(len(s), 200))) if kind == 0 else int(rng.integers(0, len(s)))
        bit = int(rng.integers(0, 8))
        b = bytearray(s)
        b[pos] ^= 1 << bit
        cases.append((bytes(b), cap, kind))
    return cases, [b[0] for b in bases]


# ---- crafted blocks ----
def bz_crc(data, r=0xFFFFFFFF):
    if "tab" not in _cache:
        tab = []
        for t in range(256):
            v = t << 24
            for _ in range(8):
                v = ((v << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if v & 0x80000000 else (v << 1) & 0xFFFFFFFF
            tab.append(v)
        _cache["tab"] = tab
    tab = _cache["tab"]
    for b in data:
        r = ((r << 8) & 0xFFFFFFFF) ^ tab[(r >> 24) ^ b]
    return r


def inverse_block(L, origin):
    """The serial reading of a block (BWT_Detransform, then RLE_1 along the chase) for ANY last column and origin: the output bytes."""
    n = len(L)
    cf, t = [0] * 256, 0
    cnt = [0] * 256
    for b in L:
        cnt[b] += 1
    for i in range(256):
        cf[i], t = t, t + cnt[i]
    nxt = [0] * n
    for p, b in enumerate(L):
        nxt[cf[b]] = p
        cf[b] += 1
    out = bytearray()
    idx, state, old = nxt[origin], 0, 0
    for _ in range(n):
        d, idx = L[idx], nxt[idx]
        if state == 4:
            out += bytes([old]) * d
            state = 0
            continue
        state = 1 if state > 0 and d != old else state + 1
        out.append(d)
        old = d
    return bytes(out)


def mtf_symbols(L):
    """(in-use byte values, the MTF / RUNA / RUNB symbols of a last column with the end-of-block symbol behind)."""
    used = sorted(set(L))
    lst = list(range(len(used)))
    where = {b: i for i, b in enumerate(used)}
    syms, run = [], 0
    for b in L:
        v = where[b]
        j = lst.index(v)
        if j == 0:
            run += 1
            continue
        r = run
        while r > 0:                                   # bijective base 2: RUNA = 1, RUNB = 2
            syms.append(0 if r & 1 else 1)
            r = (r - 1) >> 1
        run = 0
        lst.pop(j)
        lst.insert(0, v)
        syms.append(j + 1)
    r = run
    while r > 0:
        syms.append(0 if r & 1 else 1)
        r = (r - 1) >> 1
    syms.append(len(used) + 1)
    return used, syms


def column_of_symbols(syms, used=None):
    """The last column that a sequence of MTF symbols (no RUNA / RUNB) decodes to, all 256 byte values in use."""
    lst = list(range(256))
    out = bytearray()
    for s in syms:
        v = lst.pop(s - 1)
        lst.insert(0, v)
        out.append(v)
    return bytes(out)


class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, k):
        self.v = (self.v << k) | (value & ((1 << k) - 1))
        self.n += k

    def bytes(self):
        pad = (-self.n) % 8
        return (self.v << pad).to_bytes((self.n + pad) // 8, "big")


def craft_stream(blocks, level=9, trailing=b"", stored_crcs=None):
    """A stream of crafted blocks: each a dict(L = last column, origin, lens = code lengths of the alphabet as given (None: 8 bits for all, as far as
    the alphabet allows), randomised = False, symbols = the symbol list instead of the MTF of L).  The stored CRCs are those of the serial reading.
    -> (stream, expected bytes, bit offset of every block's first coded symbol)."""
    w = _Bits()
    w.put(int.from_bytes(b"BZh", "big"), 24)
    w.put(ord("0") + level, 8)
    comb, expect, data_bits = 0, bytearray(), []
    for bi, blk in enumerate(blocks):
        L, origin = blk["L"], blk["origin"]
        used, syms = mtf_symbols(L)
        if blk.get("all256"):
            used = list(range(256))
        if blk.get("symbols") is not None:
            syms = list(blk["symbols"]) + [len(used) + 1]
        alpha = len(used) + 2
        lens = blk.get("lens")
        if lens is None:
            k = max(1, (alpha - 1).bit_length())
            lens = [k] * alpha
        assert len(lens) == alpha
        plain = inverse_block(L, origin) if origin < len(L) else b""
        crc = bz_crc(plain) ^ 0xFFFFFFFF
        if stored_crcs is not None and stored_crcs[bi] is not None:
            crc = stored_crcs[bi]
        comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ crc
        expect += plain
        w.put(BLOCK_MAGIC, 48)
        w.put(crc, 32)
        w.put(1 if blk.get("randomised") else 0, 1)
        w.put(origin, 24)
        groups = [any(16 * i <= b < 16 * i + 16 for b in used) for i in range(16)]
        for g in groups:
            w.put(int(g), 1)
        for i, g in enumerate(groups):
            if g:
                for j in range(16):
                    w.put(int(16 * i + j in used), 1)
        nsel = (len(syms) + 49) // 50
        w.put(2, 3)
        w.put(nsel, 15)
        for _ in range(nsel):
            w.put(0, 1)
        for _ in range(2):
            cur = lens[0]
            w.put(cur, 5)
            for ln in lens:
                while cur < ln:
                    w.put(0b10, 2)
                    cur += 1
                while cur > ln:
                    w.put(0b11, 2)
                    cur -= 1
                w.put(0, 1)
        codes, vec = [0] * alpha, 0                    # hbAssignCodes: in order of length, then of symbol
        for ln in range(min(lens), max(lens) + 1):
            for s in range(alpha):
                if lens[s] == ln:
                    codes[s] = vec
                    vec += 1
            vec <<= 1
        data_bits.append(w.n)
        for s in syms:
            w.put(codes[s], lens[s])
    w.put(FOOTER_MAGIC, 48)
    w.put(comb, 32)
    return w.bytes() + trailing, bytes(expect), data_bits


MAGIC_LENS = [9, 9] + [8] * 254 + [9, 9]               # 254 codes of length 8 (symbols 2 .. 255: code = symbol - 2) and 4 of length 9


def magic_inside_block(shift):
    """Crafted case (b): a block whose coded data hold the six bytes of the block magic as six symbols, `shift` symbols of 9 bits in front of
    them.  -> (stream, expected bytes, bit position of the false magic)."""
    rng = np.random.default_rng(5)
    front = [int(x) for x in rng.integers(2, 256, 40)] + [256] * shift
    magic = [b + 2 for b in BLOCK_MAGIC.to_bytes(6, "big")]
    back = [int(x) for x in rng.integers(2, 256, 60)]
    syms = front + magic + back
    L = column_of_symbols(syms)
    stream, expect, bits = craft_stream([dict(L=L, origin=7, lens=MAGIC_LENS, symbols=syms, all256=True)])
    return stream, expect, bits[0] + 8 * 40 + 9 * shift


def crafted_cases():
    """name -> (stream, expected bytes or None when the stream is to be refused, rule name when refused)."""
    rng = np.random.default_rng(3)
    cases = {}
    # (a) a last column that is no BWT of anything: its permutation has several cycles
    L = bytes(rng.integers(97, 105, 3000, dtype=np.uint8))
    s, exp, _ = craft_stream([dict(L=L, origin=1234)])
    cases["a_cycles"] = (s, exp, None)
    L2 = bytes(rng.integers(0, 256, 700, dtype=np.uint8))
    s, exp, _ = craft_stream([dict(L=L2, origin=0), dict(L=L, origin=2999), dict(L=b"zzzzz\x03", origin=2)])
    cases["a_cycles_three_blocks"] = (s, exp, None)
    # (b) the block magic inside a block's coded data, at three bit offsets
    for shift in (0, 3, 7):
        s, exp, at = magic_inside_block(shift)
        cases["b_magic_inside_%d" % shift] = (s, exp, None)
    # (c) both magics in trailing garbage behind the footer
    s, exp, _ = craft_stream([dict(L=L2, origin=5)], trailing=b"\x00" + BLOCK_MAGIC.to_bytes(6, "big") + b"abc" + FOOTER_MAGIC.to_bytes(6, "big") + b"\x00" * 9)
    cases["c_magic_behind_footer"] = (s, exp, None)
    # (d) a set randomised flag, (e) origin = symbol count
    cases["d_randomised"] = (craft_stream([dict(L=L2, origin=5, randomised=True)])[0], None, "randomised block")
    cases["e_origin_is_count"] = (craft_stream([dict(L=L2, origin=len(L2))])[0], None, "origin not below the block's symbol count")
    return cases
