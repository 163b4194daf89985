"""zada_unzip_device (csrc/zada_unzip.hip): an archive that lies in device memory, extracted into device memory -- the C ABI on hand-built archive
buffers, the stored entries through their pieces, encrypted entries, damage, refusals, grouping -- and UnZip.extract_device against UnZip.extract.
The references are zlib, bz2, liblzma (tests/_lzmah.py), zlib.crc32 and the byte-serial ZipCrypto model (tests/crypt/crypt_model.c); the code under
test is never one."""
import bz2
import ctypes
import io
import zipfile
import zlib

import numpy as np
import pytest

import _crypt
import _inflate
from _common import product, silesia_mix
from _devbuf import GUARD, guard_damage
from _lzmah import lzma_decode
from test_gpu_inflate import PW, _entries
from test_inflate_model import deflate64_cases, deflate64_fixed

pytestmark = pytest.mark.gpu
E_INVALID, E_TOO_LARGE, E_DATA, E_PASSWORD = -1, -4, -7, -8
FILL, G = 0x3C, 16
LENGTHS = (0, 1, 15, 16, 17, 255, 256, 257, 16383, 16384, 16385, 70000)
ALL1 = 0xFFFFFFFF


class Item:
    """One entry of a hand-built archive: the bytes in the archive, the method, what it decodes to."""

    def __init__(self, method, stream, plain, eos=0, label=""):
        self.method, self.stream, self.plain, self.eos, self.label = method, bytes(stream), bytes(plain), eos, label
        self.flags, self.check, self.data = eos << 1, 0, self.stream
        self.used = len(self.stream)                      # the bytes of the stream its decoder consumes (stream_used, where a library can say)

    def encrypted(self, keys, k, from_time):
        """The same entry behind an encryption header (zip-compress.adb:153-161), the check byte from the CRC or -- flag bit 3 -- from a time stamp."""
        it = Item(self.method, self.stream, self.plain, self.eos, self.label + "/pw")
        it.used = self.used + 12
        it.check = (0x5B + 7 * k) & 0xFF if from_time else (zlib.crc32(self.plain) >> 24) & 0xFF
        hdr, kept = _crypt.encode(keys, bytes((31 * k + j) & 0xFF for j in range(11)) + bytes([it.check]))
        it.data = hdr + _crypt.encode(kept, self.stream)[0]
        it.flags |= 1
        return it


def crc_after(reg, data):
    return zlib.crc32(data, reg ^ ALL1) ^ ALL1


def stream_used(method, stream):
    """The bytes of a stream that zlib, libbz2 or liblzma consume when seven more follow it."""
    import lzma
    if method == 8:
        return _inflate.zlib_in_used(stream)
    if method == 12:
        d = bz2.BZ2Decompressor()
        d.decompress(stream + b"\x55" * 7)
    else:
        s = stream[4:]
        props = s[0]
        d = lzma.LZMADecompressor(format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA1, "dict_size": int.from_bytes(s[1:5], "little"), "lc": props % 9,
                                                                    "lp": (props // 9) % 5, "pb": props // 45}])
        d.decompress(s[5:] + b"\x55" * 7)
    assert d.eof
    return len(stream) + 7 - len(d.unused_data)


def raw_deflate(d, level=6):
    return _inflate.zlib_raw(d, level, zlib.Z_DEFAULT_STRATEGY)


@pytest.fixture(scope="module")
def text():
    return silesia_mix(300000, class_mask=1) + silesia_mix(300000)


@pytest.fixture(scope="module")
def items(encoder, text):
    """Payloads of all five methods at the lengths of the issue: the product's writers and zipfile / zlib / bz2 / liblzma take turns."""
    za = product()
    plains = [text[1000 * k:1000 * k + n] for k, n in enumerate(LENGTHS)]
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as z:
        for k, d in enumerate(plains):
            for nm, m in (("d", zipfile.ZIP_DEFLATED), ("b", zipfile.ZIP_BZIP2), ("l", zipfile.ZIP_LZMA)):
                z.writestr(zipfile.ZipInfo("%s%d" % (nm, k)), d, compress_type=m)
    arc = b.getvalue()
    info = za.ZipInfo.load(arc)
    zf = {e.name: (arc[e.data_offset:e.data_offset + e.csize], (e.flags >> 1) & 1) for e in info.entries}
    bz = encoder.bzip2_batch(plains, 14)
    lz = encoder.lzma_batch(plains, 18)
    out = []
    for k, d in enumerate(plains):
        out.append(Item(0, d, d, label="store%d" % len(d)))
        try:
            s = encoder.deflate(d, za.Method.Deflate_3)[0] if k & 1 else zf["d%d" % k][0]
        except za.CompressionInefficient:
            s = raw_deflate(d, 9)
        out.append(Item(8, s, d, label="deflate%d" % len(d)))
        s = bz[k][1] if k & 1 and bz[k][1] is not None else zf["b%d" % k][0]
        out.append(Item(12, s, d, label="bzip2_%d" % len(d)))
        if not k & 1 and lz[k][1] is not None:
            out.append(Item(14, lz[k][1], d, eos=1, label="lzma%d" % len(d)))
        else:
            out.append(Item(14, zf["l%d" % k][0], d, eos=zf["l%d" % k][1], label="zlzma%d" % len(d)))
    for name, (tokens, far) in deflate64_cases().items():
        s, exp = deflate64_fixed(tokens)
        out.append(Item(9, s, exp, label="d64_" + name))
    # what the references make of them
    for it in out:
        if it.method == 8:
            assert zlib.decompress(it.stream, -15) == it.plain
        elif it.method == 12:
            assert bz2.decompress(it.stream) == it.plain
        elif it.method == 14:
            assert lzma_decode(it.stream, 4) == it.plain
        if it.method in (8, 12, 14):
            it.used = stream_used(it.method, it.stream)
    assert {it.method for it in out} == {0, 8, 9, 12, 14} and len(out) >= 50
    return out


def layout(items, rot=0):
    """The archive buffer (FILL between the entries, every in_off mod 16 in turn) and the table, outputs G guard bytes apart at every out_off mod 16."""
    tab = np.zeros(len(items), dtype=product().Encoder.unzip_dtypes()[0])
    pos, opos, parts = 0, G, []
    for k, it in enumerate(items):
        pad = ((k + rot) % 16 - pos) % 16
        parts.append(bytes([FILL]) * pad + it.data)
        pos += pad
        opos += (((7 * k + 3 + rot) % 16) - opos) % 16
        tab[k] = (pos, len(it.data), opos, len(it.plain), it.method, it.flags, it.check, 0)
        pos += len(it.data)
        opos += len(it.plain) + G
    arc = np.frombuffer(b"".join(parts) + bytes([FILL]) * 5, dtype=np.uint8).copy()
    assert len({int(x) % 16 for x in tab["in_off"]}) == 16 and len({int(x) % 16 for x in tab["out_off"]}) == 16 or len(items) < 16
    return arc, tab, opos


def run(enc, arc, tab, out_bytes, keys0=None, crc=ALL1, test_only=False):
    """One call on fresh tensors.  -> (rc, results, the output buffer as numpy); the archive tensor is unchanged and every byte outside the entries'
    ranges is still GUARD afterwards."""
    import torch
    t_arc = torch.from_numpy(arc).cuda()
    t_out = torch.full((out_bytes,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, res = enc.unzip_device(t_arc.data_ptr(), len(arc), None if test_only else t_out.data_ptr(), 0 if test_only else out_bytes, tab, keys0, crc)
    torch.cuda.synchronize()
    host = t_out.cpu().numpy()
    assert np.array_equal(t_arc.cpu().numpy(), arc), "the archive was written"
    mask = np.ones(out_bytes, dtype=bool)
    for r in tab:
        mask[int(r["out_off"]):int(r["out_off"]) + int(r["cap"])] = False
    if test_only:
        mask[:] = True
    assert not np.flatnonzero(host[mask] != GUARD).size, "bytes outside the entries' output ranges were written"
    for r in tab if not test_only else ():
        o, cap = int(r["out_off"]), int(r["cap"])
        assert not guard_damage(host[o - G:o + cap + G], G, cap)
    return rc, res, host


def check_ok(items, tab, res, host, regs, test_only=False):
    for k, it in enumerate(items):
        r, o = res[k], int(tab["out_off"][k])
        assert int(r["rc"]) == 0, (it.label, int(r["rc"]))
        assert int(r["out_len"]) == len(it.plain) and int(r["in_used"]) == it.used, it.label
        assert int(r["crc"]) == crc_after(regs[k], it.plain), it.label
        if not test_only:
            assert host[o:o + len(it.plain)].tobytes() == it.plain, it.label


def test_every_method_at_every_alignment(encoder, items):
    rng = np.random.default_rng(1)
    regs = [int(x) for x in rng.integers(0, 1 << 32, len(items))]
    regs[::3] = [ALL1] * len(regs[::3])
    arc, tab, ob = layout(items)
    rc, res, host = run(encoder, arc, tab, ob, crc=np.array(regs, dtype=np.uint32))
    assert rc == 0
    check_ok(items, tab, res, host, regs)
    names = dict(encoder.last_timing())
    assert "unzip:k_uz_store" in names and "inflate:k_inflate" in names and "unlzma:k_unlzma" in names
    rc, res, host = run(encoder, arc, tab, ob, crc=np.array(regs, dtype=np.uint32), test_only=True)       # the same once more with d_out = NULL
    assert rc == 0
    check_ok(items, tab, res, host, regs, test_only=True)
    # the other rotation of the alignments, trailing bytes behind every stream (not an error; in_used stays) and a larger cap
    its = [it for it in items if it.method != 0]
    for it in its:
        it.data = it.stream + b"\x55" * 3
    try:
        arc, tab, ob = layout(its, rot=5)
        rc, res, host = run(encoder, arc, tab, ob)
        for k, it in enumerate(its):
            assert (int(res["rc"][k]), int(res["out_len"][k]), int(res["in_used"][k])) == (0, len(it.plain), it.used), it.label
    finally:
        for it in its:
            it.data = it.stream
    assert encoder.unzip_device(None, 0, None, 0, tab[:0])[0] == 0


@pytest.mark.parametrize("plog", (8, 14))
def test_store_through_the_pieces(encoder, plog):
    import torch
    lens = [256 * k + d for k in (1, 2, 63, 64, 65, 4097) for d in (-1, 0, 1)]
    rng = np.random.default_rng(plog)
    blob = rng.integers(0, 256, sum(lens) * 3 + 64, dtype=np.uint8)
    regs0 = (0, ALL1, 0x9E3779B9)
    items, regs = [], []
    pos = 0
    for reg in regs0:
        for n in lens:
            d = blob[pos:pos + n].tobytes()
            items.append(Item(0, d, d, label="store%d" % n)); regs.append(reg)
            pos += n
    arc, tab, ob = layout(items)
    arc = arc[:int(tab["in_off"][-1]) + int(tab["n_in"][-1])].copy()          # the last piece ends on the buffer's last byte
    encoder.set_knob("unzip_piece", plog)
    try:
        rc, res, host = run(encoder, arc, tab, ob, crc=np.array(regs, dtype=np.uint32))
        assert rc == 0
        check_ok(items, tab, res, host, regs)
        names = dict(encoder.last_timing())
        assert ("unzip:k_uz_fold" in names) and "unzip:k_uz_store" in names
        # ... and so does the last output: a tensor that ends where the last range ends
        ob2 = int(tab["out_off"][-1]) + int(tab["cap"][-1])
        t_arc = torch.from_numpy(arc).cuda()
        t_out = torch.full((ob2,), GUARD, dtype=torch.uint8, device="cuda")
        rc, res2 = encoder.unzip_device(t_arc.data_ptr(), len(arc), t_out.data_ptr(), ob2, tab, None, np.array(regs, dtype=np.uint32))
        assert rc == 0 and np.array_equal(res2, res)
        assert np.array_equal(t_out.cpu().numpy(), host[:ob2])
    finally:
        encoder.set_knob("unzip_piece", 14)
    za = product()
    for v in (7, 15):
        with pytest.raises(za.ZadaError):
            encoder.set_knob("unzip_piece", v)


def model_header_passes(keys, data, check):
    """Whether the 12 header bytes of `data` decode to something that ends in `check` from `keys`, by crypt_model.c alone: the code byte is what
    Encode makes of a zero byte, and Encode of the plain byte moves the keys on (and must give the cipher byte back)."""
    k = tuple(keys)
    p = 0
    for c in data[:12]:
        code = _crypt.encode(k, b"\0")[0][0]
        p = c ^ code
        back, k = _crypt.encode(k, bytes([p]))
        assert back[0] == c
    return p == check


def test_encrypted(encoder, items):
    keys = _crypt.init_keys(PW)
    assert encoder.crypt_init_keys(PW) == keys
    plain = ([it for it in items if it.method == 9] + [it for it in items if len(it.plain) in (0, 1, 15, 17, 256, 257, 16383, 16385, 70000) and it.method != 9])[:40]
    assert len(plain) == 40 and {it.method for it in plain} == {0, 8, 9, 12, 14}
    coded = [it.encrypted(keys, k, from_time=bool(k & 1)) for k, it in enumerate(plain)]
    assert all(model_header_passes(keys, it.data, it.check) for it in coded)
    arc, tab, ob = layout(coded, rot=3)
    regs = [ALL1] * len(coded)
    rc, res, host = run(encoder, arc, tab, ob, keys0=keys)                      # (run: the archive is unchanged -- in-place decoding would not give that)
    assert rc == 0
    check_ok(coded, tab, res, host, regs)
    assert "unzip:k_uz_decode" in dict(encoder.last_timing())
    arc_p, tab_p, ob_p = layout(plain, rot=3)
    rc, res_p, host_p = run(encoder, arc_p, tab_p, ob_p)
    assert rc == 0 and np.array_equal(res_p["crc"], res["crc"]) and np.array_equal(res_p["out_len"], res["out_len"])
    for k in range(len(plain)):
        o, op, n = int(tab["out_off"][k]), int(tab_p["out_off"][k]), len(plain[k].plain)
        assert np.array_equal(host[o:o + n], host_p[op:op + n])
    rc, res, _ = run(encoder, arc, tab, ob, keys0=keys, test_only=True)
    assert rc == 0
    check_ok(coded, tab, res, host, regs, test_only=True)
    # a wrong password: every entry is ZADA_E_PASSWORD but those whose header passes the check byte by chance -- by the model, fewer than 4 of 40
    wrong = _crypt.init_keys("not it 11")
    lucky = [model_header_passes(wrong, it.data, it.check) for it in coded]
    assert sum(lucky) < 4
    rc, res, host = run(encoder, arc, tab, ob, keys0=wrong)
    assert rc == E_PASSWORD
    for k, it in enumerate(coded):
        assert (int(res["rc"][k]) == E_PASSWORD) == (not lucky[k]), it.label
        if not lucky[k]:
            o = int(tab["out_off"][k])
            assert (int(res["out_len"][k]), int(res["in_used"][k]), int(res["crc"][k])) == (0, 0, ALL1)
            assert not np.flatnonzero(host[o:o + len(it.plain)] != GUARD).size, "the output range of a refused entry was written"
    assert "entry" in encoder.lib.zada_last_error(encoder.ctx).decode()
    # an entry shorter than its encryption header
    short = Item(8, b"", b"x" * 5)
    short.data, short.flags = coded[1].data[:11], 1
    arc, tab, ob = layout([coded[0], short, coded[2]])
    rc, res, host = run(encoder, arc, tab, ob, keys0=keys)
    assert rc == E_DATA and [int(x) for x in res["rc"]] == [0, E_DATA, 0]
    assert (int(res["out_len"][1]), int(res["in_used"][1]), int(res["crc"][1])) == (0, 0, ALL1)


def device_rc(enc, it):
    """What the method's own *_device call says to the entry's bytes: 0 or ZADA_E_DATA."""
    import torch
    za = product()
    t_in = torch.from_numpy(np.frombuffer(it.data + b"\0", dtype=np.uint8).copy()).cuda()
    t_out = torch.zeros(len(it.plain) + 16, dtype=torch.uint8, device="cuda")
    try:
        if it.method in (8, 9):
            enc.inflate_device(t_in.data_ptr(), len(it.data), t_out.data_ptr(), len(it.plain), it.method)
        elif it.method == 12:
            enc.bunzip2_device(t_in.data_ptr(), len(it.data), t_out.data_ptr(), len(it.plain))
        else:
            enc.unlzma_device(t_in.data_ptr(), len(it.data), t_out.data_ptr(), len(it.plain), bool(it.eos))
    except za.DataError:
        return E_DATA
    return 0


def test_damage(encoder, items):
    base = [it for it in items if len(it.plain) in (257, 16385)] + [it for it in items if it.method == 9][:2]
    seen = set()
    for method in (8, 9, 12, 14, 0):
        k = next(i for i, it in enumerate(base) if it.method == method and len(it.data) > 40)
        its = list(base)
        bad = Item(method, base[k].stream, base[k].plain, base[k].eos, base[k].label + "/flipped")
        b = bytearray(bad.data)
        b[len(b) // 2] ^= 0x10
        bad.data = bytes(b)
        its[k] = bad
        arc, tab, ob = layout(its, rot=method)
        rc, res, host = run(encoder, arc, tab, ob)
        said = encoder.lib.zada_last_error(encoder.ctx).decode()
        want = 0 if method == 0 else device_rc(encoder, bad)
        assert int(res["rc"][k]) == want, bad.label
        seen.add(want)
        if want:
            o = int(tab["out_off"][k])
            assert rc == E_DATA and (int(res["out_len"][k]), int(res["in_used"][k]), int(res["crc"][k])) == (0, 0, ALL1)
            assert "entry %d" % k in said, said
        elif method == 0:
            o = int(tab["out_off"][k])
            assert host[o:o + len(bad.plain)].tobytes() == bad.data and int(res["crc"][k]) == crc_after(ALL1, bad.data)
        others = [i for i in range(len(its)) if i != k]
        check_ok([its[i] for i in others], tab[others], res[others], host, [ALL1] * len(others))
    assert E_DATA in seen
    # a stored entry with more bytes than the directory promises
    its = [base[0], Item(0, b"abcdef", b"abcde"), base[1]]
    arc, tab, ob = layout(its)
    rc, res, host = run(encoder, arc, tab, ob)
    assert rc == E_DATA and [int(x) for x in res["rc"]] == [0, E_DATA, 0] and int(res["out_len"][1]) == 0
    o = int(tab["out_off"][1])
    assert host[o:o + 5].tobytes() == bytes([GUARD]) * 5
    # ... and with fewer: out_len is what is stored
    its = [Item(0, b"abc", b"abcde")]
    arc, tab, ob = layout(its)
    rc, res, host = run(encoder, arc, tab, ob)
    assert rc == 0 and (int(res["out_len"][0]), int(res["in_used"][0])) == (3, 3) and host[int(tab["out_off"][0]):][:5].tobytes() == b"abc" + bytes([GUARD]) * 2


def test_refusals(encoder, items):
    import torch
    za = product()
    its = [it for it in items if len(it.plain) == 257]
    keys = _crypt.init_keys(PW)
    its = its + [its[1].encrypted(keys, 1, False)]
    arc, tab, ob = layout(its)
    t_arc = torch.from_numpy(arc).cuda()
    t_out = torch.full((ob,), GUARD, dtype=torch.uint8, device="cuda")

    def call(tab, alen=len(arc), obytes=ob, k0=keys):
        kk = (ctypes.c_uint32 * 3)(*k0) if k0 else None
        res = np.zeros(len(tab), dtype=za.Encoder.unzip_dtypes()[1])
        rc = encoder.lib.zada_unzip_device(encoder.ctx, t_arc.data_ptr(), alen, t_out.data_ptr(), obytes, len(tab), tab.ctypes.data, kk, res.ctypes.data)
        return rc, encoder.lib.zada_last_error(encoder.ctx).decode()

    last = len(its) - 1
    cases = []
    for field, value, who in (("in_off", len(arc), 2), ("n_in", len(arc) + 1, 0), ("out_off", ob, 3), ("cap", ob, 1), ("method", 1, 2), ("method", 98, 0)):
        t = tab.copy()
        t[field][who] = value
        cases.append((t, {}, who, E_INVALID))
    cases.append((tab, {"k0": None}, last, E_INVALID))
    cases.append((tab, {"alen": int(tab["in_off"][last]) + 5}, last, E_INVALID))
    cases.append((tab, {"obytes": int(tab["out_off"][2])}, 2, E_INVALID))
    t = tab.copy(); t["out_off"][3] = int(t["out_off"][1]) + 1
    cases.append((t, {}, None, E_INVALID))
    t = tab.copy(); t["cap"][1] = 1 << 40
    cases.append((t, {}, 1, E_TOO_LARGE))
    t = tab.copy(); t["n_in"][0] = (1 << 64) - 8
    cases.append((t, {}, 0, E_TOO_LARGE))
    for t, kw, who, want in cases:
        rc, text = call(t, **kw)
        assert rc == want and (who is None or "entry %d:" % who in text), (rc, text)
        assert not np.flatnonzero(t_out.cpu().numpy() != GUARD).size                 # the checks come before anything touches the device
        rc, text = call(tab)                                                       # a following valid call works
        assert rc == 0, text
        host = t_out.cpu().numpy()
        for k, it in enumerate(its):
            o = int(tab["out_off"][k])
            assert host[o:o + len(it.plain)].tobytes() == it.plain
        t_out.fill_(GUARD)
    with pytest.raises(za.ZadaError):
        encoder.unzip_device(t_arc.data_ptr(), len(arc), t_out.data_ptr(), ob, tab, None)
    # ranges that only touch, and an empty range inside another's, are fine
    t = tab.copy()
    t["out_off"][1] = int(t["out_off"][0]) + int(t["cap"][0])
    t["out_off"][2] = int(t["out_off"][1]) + int(t["cap"][1])
    assert call(t)[0] == 0


def test_grouping(text):
    """batch_mib = 1, bunzip_batch_mib = 16 and lzma_lit_mib = 16 on 300 small entries, some of them of the LZMA methods whose literal tables live in
    HBM (6 MiB for lc = 8, lp = 4; 384 KiB for lc = 8): several groups and launches, the results of the defaults."""
    za = product()
    enc = za.Encoder(0)
    try:
        rng = np.random.default_rng(4)
        plains = [text[int(o):int(o) + int(n)] for o, n in zip(rng.integers(0, 500000, 300), rng.integers(0, 9000, 300))]
        lz = {m: enc.lzma_batch(plains[k::30][:n], m) for k, (m, n) in enumerate(((19, 5), (23, 8), (18, 10)))}
        bz = enc.bzip2_batch(plains[3::5], 14)
        items = []
        for k, d in enumerate(plains):
            hit = [(m, k // 30) for j, m in enumerate((19, 23, 18)) if k % 30 == j and k // 30 < len(lz[m]) and lz[m][k // 30][1] is not None]
            if hit:
                items.append(Item(14, lz[hit[0][0]][hit[0][1]][1], d, eos=1, label="lzma%d_%d" % (hit[0][0], k)))
                if hit[0][0] == 18:                            # (liblzma reads lc + lp <= 4 only: the data-type methods' streams are checked by their bytes)
                    assert lzma_decode(items[-1].stream, 4) == d
            elif k % 5 == 3 and bz[k // 5][1] is not None:
                items.append(Item(12, bz[k // 5][1], d, label="bzip2_%d" % k))
            elif k % 5 == 4:
                items.append(Item(0, d, d, label="store_%d" % k))
            else:
                items.append(Item(8, raw_deflate(d), d, label="deflate_%d" % k))
        for it in items:
            if it.method in (8, 12) or it.label.startswith("lzma18"):
                it.used = stream_used(it.method, it.stream)
        big = [it for it in items if it.method == 14 and it.stream[4] >= 9 * 4 + 8]      # lc + lp >= 4 by the properties byte
        assert len(big) >= 4 and sum(it.method == 14 for it in items) >= 15
        keys = _crypt.init_keys(PW)
        items = [it.encrypted(keys, k, False) if k % 7 == 0 else it for k, it in enumerate(items)]
        arc, tab, ob = layout(items)
        regs = [ALL1] * len(items)
        rc, res, host = run(enc, arc, tab, ob, keys0=keys)
        assert rc == 0
        check_ok(items, tab, res, host, regs)
        for name, v in (("batch_mib", 1), ("bunzip_batch_mib", 16), ("lzma_lit_mib", 16)):
            enc.set_knob(name, v)
        rc, res2, host2 = run(enc, arc, tab, ob, keys0=keys)
        assert rc == 0 and np.array_equal(res2, res) and np.array_equal(host2, host)
        rc, res3, _ = run(enc, arc, tab, ob, keys0=keys, test_only=True)            # (more than 1 MiB of outputs: several groups of the test-only form)
        assert sum(len(it.plain) for it in items) > 1 << 20
        assert rc == 0 and np.array_equal(res3, res)
    finally:
        enc.close()


# ---- UnZip.extract_device against UnZip.extract ----
def same(got, want):
    assert list(got) == list(want)
    for nm in want:
        g, w = got[nm], want[nm]
        if isinstance(w, Exception):
            assert type(g) is type(w) and str(g) == str(w), (nm, g, w)
        elif w is None:
            assert g is None, nm
        else:
            assert g.device.type == "cuda" and g.data_ptr() % 256 == 0 and bytes(g.cpu().numpy()) == w, nm


def both(uz, archive, password=None, **kw):
    import torch
    za = product()
    t = torch.from_numpy(np.frombuffer(archive, dtype=np.uint8).copy()).cuda()
    before = t.clone()
    want = uz.extract(za.ZipInfo.load(archive), password=password, errors="collect", **kw)
    info = za.ZipInfo.load_device(t)
    got = uz.extract_device(info, password=password, errors="collect", **kw)
    same(got, want)
    assert torch.equal(t, before)
    if any(isinstance(v, Exception) for v in want.values()) and not kw.get("test_only"):
        with pytest.raises(za.ZadaError) as a:
            uz.extract(za.ZipInfo.load(archive), password=password, **kw)
        with pytest.raises(za.ZadaError) as b:
            uz.extract_device(info, password=password, **kw)
        assert type(a.value) is type(b.value) and str(a.value) == str(b.value)
        same(b.value.results, a.value.results)
    return got, info


@pytest.fixture(scope="module")
def entries():
    return _entries(silesia_mix(600000))


@pytest.mark.parametrize("password", (None, PW))
def test_archives_of_the_writer(encoder, entries, password):
    za = product()
    uz = za.UnZip(encoder, bzip2=True, lzma=True)
    for method in (za.Method.Deflate_3, za.Method.Preselection_2):
        zc = za.ZipCreate(encoder, method)
        zc.add_streams([e[0] for e in entries], [e[1] for e in entries], password=password)
        arc = zc.finish()
        got, info = both(uz, arc, password)
        assert {nm: bytes(v.cpu().numpy()) for nm, v in got.items()} == dict(entries)
        both(uz, arc, password, test_only=True)
        both(uz, arc, password, what=entries[1][0])
        both(uz, arc, password, what=[entries[3][0], entries[0][0]])
        assert uz.extract_device(info, what=[], password=password) == {}
        if method == za.Method.Preselection_2:
            assert {e.method for e in info.entries} & {12, 14}
            gated, _ = both(za.UnZip(encoder), arc, password)                    # the gates: UnsupportedMethod in extract's words
            assert any(isinstance(v, za.UnsupportedMethod) for v in gated.values())
            both(za.UnZip(encoder, bzip2=True), arc, password)
            both(za.UnZip(encoder, lzma=True), arc, password)
        if password:
            wrong, _ = both(uz, arc, "not it")
            assert sum(isinstance(v, za.WrongPassword) for v in wrong.values()) >= len(entries) - 1
            none, _ = both(uz, arc, None)
            assert all(isinstance(v, za.WrongPassword) for v in none.values())
            both(uz, arc, "not it", test_only=True)


def test_archives_of_zipfile_and_damage(encoder, entries):
    za = product()
    uz = za.UnZip(encoder, bzip2=True, lzma=True)
    for method in (zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED, zipfile.ZIP_BZIP2, zipfile.ZIP_LZMA):
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w", method) as z:
            for nm, d in entries:
                z.writestr(nm, d)
            z.comment = b"made by zipfile"
        arc = b.getvalue()
        got, info = both(uz, arc)
        assert {nm: bytes(v.cpu().numpy()) for nm, v in got.items()} == dict(entries)
        both(uz, arc, test_only=True)
        # one flipped payload byte: the exception of extract, the other entries extracted
        e = info["mix.bin"]
        bad = bytearray(arc)
        bad[e.data_offset + min(1000, e.csize - 1)] ^= 0x10
        got, _ = both(uz, bytes(bad))
        assert isinstance(got["mix.bin"], za.ZadaError)
        both(uz, bytes(bad), test_only=True)
        # a directory that promises another size
        cd = arc.find(b"PK\x01\x02")
        lie = bytearray(arc)
        lie[cd + 24:cd + 28] = (len(entries[0][1]) + 1).to_bytes(4, "little")
        got, _ = both(uz, bytes(lie))
        assert isinstance(got[entries[0][0]], za.ZadaError)
    b = io.BytesIO()
    zipfile.ZipFile(b, "w").close()
    import torch
    info = za.ZipInfo.load_device(torch.from_numpy(np.frombuffer(b.getvalue(), dtype=np.uint8).copy()).cuda())
    assert uz.extract_device(info) == {}
    with pytest.raises(za.ZadaError):
        uz.extract_device(za.ZipInfo.load(arc))
    with pytest.raises(za.ZadaError):                                              # a tensor that is not on the encoder's device
        uz.extract_device(za.ZipInfo.load_device(torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy())))
