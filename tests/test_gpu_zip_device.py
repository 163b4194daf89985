"""zada_zip_device (csrc/zada_zip.hip): entries that lie in device memory written as one Zip archive into device memory -- the C ABI at every
alignment and at the exact capacity, the groups, Zip64, the refusals -- and ZipCreate.write_device read back by ZipInfo.load_device /
UnZip.extract_device and by zipfile.  The reference throughout is the host path on the same encoder, ZipCreate.add_streams + finish, which
test_oracle.py pins to the oracle; the code under test is never one."""
import ctypes
import io
import zipfile
import zlib

import numpy as np
import pytest

from _common import product, silesia_mix
from _devbuf import GUARD, guard_damage

pytestmark = pytest.mark.gpu
E_INVALID, E_TOO_LARGE = -1, -4
FILL, G = 0x3C, 64
LENGTHS = (0, 1, 2, 3, 31, 255, 4095, 32767, 32768, 32769, 65537, 100000)
METHODS = (0, 6, 7, 8, 9, 10, 11)
MIB4 = 4 << 20


@pytest.fixture(scope="module")
def text():
    return silesia_mix(300000, class_mask=1) + silesia_mix(300000)


@pytest.fixture(scope="module")
def plains(text):
    """The lengths of the issue cut from the generators' text, 4 KiB of random bytes (which must come out stored) and an all-zero entry."""
    out = [text[1000 * k:1000 * k + n] for k, n in enumerate(LENGTHS)]
    out.append(np.random.default_rng(7).integers(0, 256, 4096, dtype=np.uint8).tobytes())
    out.append(bytes(50000))
    return out


def names_for(datas):
    return ["dir/e%03d_%d.bin" % (k, len(d)) for k, d in enumerate(datas)]


_host = {}


def host_archive(enc, method, names, datas, base=0, key=None, **kw):
    """The reference: ZipCreate (enc, method).add_streams + finish.  -> (archive bytes, entries); kept under `key` for the tests that share it."""
    if key is not None and key in _host:
        return _host[key]
    zc = product().ZipCreate(enc, method, _offset_bias=base)
    zc.add_streams(names, datas, **kw)
    r = (zc.finish(), zc.entries)
    if key is not None:
        _host[key] = r
    return r


class Call:
    """One zada_zip_device call on fresh tensors: input k at offset a_in [k] modulo 16 in one arena of FILL, the archive buffer at offset G + a_arc of
    a tensor of GUARD with at least G guard bytes on both sides.  run () asserts that no guard byte and no byte of the arena changed."""

    def __init__(self, enc, names, datas, a_arc=0, a_in=None, time=None, unicode=True):
        import torch
        za = product()
        self.enc, self.n = enc, len(datas)
        a_in = a_in if a_in is not None else [(5 * k + 3) % 16 for k in range(self.n)]
        pos, offs = 0, []
        for k, d in enumerate(datas):
            pos += (a_in[k] - pos) % 16
            offs.append(pos)
            pos += len(d) + 1
        self.h_in = np.full(pos + 16, FILL, dtype=np.uint8)
        for o, d in zip(offs, datas):
            self.h_in[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
        self.t_in = torch.from_numpy(self.h_in).cuda()
        self.nms = [nm.encode("utf-8") for nm in names]
        self.blob = np.frombuffer(b"".join(self.nms) + b"\0", dtype=np.uint8)
        self.tab = np.zeros(self.n, dtype=za.Encoder.zip_dtypes()[0])
        at = 0
        for k, (o, d) in enumerate(zip(offs, datas)):
            self.tab[k] = (self.t_in.data_ptr() + o if len(d) else 0, len(d), self.blob.ctypes.data + at, len(self.nms[k]), za.ZipCreate.DEFAULT_TIME if time is None else time,
                           1 if unicode else 0, 0)
            at += len(self.nms[k])
        self.a_arc = G + a_arc
        self.t_arc = None

    def bound(self, base=0):
        return self.enc.zip_bound(self.tab, base)

    def run(self, method, cap, base=0, tab=None):
        """-> (rc, archive_len, results, the cap bytes of the archive buffer, the error text)"""
        import torch
        tab = self.tab if tab is None else tab
        self.t_arc = torch.full((self.a_arc + cap + G,), GUARD, dtype=torch.uint8, device="cuda")
        res = np.zeros(len(tab), dtype=product().Encoder.zip_dtypes()[1])
        alen = ctypes.c_uint64(0)
        torch.cuda.synchronize()
        rc = self.enc.lib.zada_zip_device(self.enc.ctx, method, len(tab), tab.ctypes.data if len(tab) else None, self.t_arc.data_ptr() + self.a_arc, cap, base,
                                          ctypes.byref(alen), res.ctypes.data if len(tab) else None)
        said = self.enc.lib.zada_last_error(self.enc.ctx).decode()
        torch.cuda.synchronize()
        host = self.t_arc.cpu().numpy()
        bad = guard_damage(host, self.a_arc, cap)
        assert not bad, "bytes outside the archive buffer were written: offsets %r relative to d_archive, cap %d" % ([b - self.a_arc for b in bad[:8]], cap)
        assert np.array_equal(self.t_in.cpu().numpy(), self.h_in), "the inputs were written"
        return rc, alen.value, res, host[self.a_arc:self.a_arc + cap], said


def same_results(res, entries, datas):
    for k, (r, e) in enumerate(zip(res, entries)):
        assert (int(r["rc"]), int(r["zip_type"]), int(r["crc"]), int(r["csize"]), int(r["offset"])) == (0, e["zip_type"], e["crc"], e["csize"], e["offset"]), k
        assert int(r["crc"]) == zlib.crc32(datas[k])


@pytest.mark.parametrize("method", METHODS)
def test_archive_equality(encoder, plains, method):
    names = names_for(plains)
    want, entries = host_archive(encoder, method, names, plains, key=("plains", method))
    c = Call(encoder, names, plains)
    cap = c.bound()
    assert cap >= len(want)
    rc, alen, res, buf, said = c.run(method, cap)
    assert rc == 0, said
    assert alen == len(want) and buf[:alen].tobytes() == want
    same_results(res, entries, plains)
    zt = [int(x) for x in res["zip_type"]]
    assert zt[0] == 0 and zt[-2] == 0, "an empty entry and 4 KiB of random bytes are stored"
    assert method == 0 or (zt[-1] == 8 and zt[-3] == 8 and int(res["csize"][-1]) < 10000)
    marks = dict(encoder.last_timing())
    assert "zip:k_zw_place" in marks and (("zip:k_zw_pack" in marks) == (method != 0)) and (("unzip:k_uz_store" in marks) == (method == 0))
    with zipfile.ZipFile(io.BytesIO(buf[:alen].tobytes())) as z:
        assert z.testzip() is None and [z.read(nm) for nm in names] == plains


@pytest.mark.parametrize("k", range(16))
def test_every_alignment_and_the_exact_capacity(encoder, plains, k):
    """Archive k: d_archive at offset k modulo 16, input j at offset (j + k) modulo 16 (fourteen entries: over the sixteen archives every entry meets
    every alignment), with Deflate_1 and with Store.  cap = archive_len exactly succeeds; one byte short is refused with the guards intact."""
    za = product()
    names = names_for(plains)
    for method in (za.Method.Deflate_1, za.Method.Store):
        want, entries = host_archive(encoder, method, names, plains, key=("plains", method))
        c = Call(encoder, names, plains, a_arc=k, a_in=[(j + k) % 16 for j in range(len(plains))])
        assert sorted(int(p) % 16 for p in c.tab["d_data"] if p) == sorted((j + k) % 16 for j, d in enumerate(plains) if len(d))
        rc, alen, res, buf, said = c.run(method, len(want))
        assert rc == 0 and alen == len(want), said
        assert buf.tobytes() == want
        same_results(res, entries, plains)
        rc, alen, res, buf, said = c.run(method, len(want) - 1)
        assert rc == E_INVALID and "archive buffer too small" in said
        # ... and where the directory alone does not fit, or not even the first header
        for cap in (entries[-1]["offset"] + 40, 10, 0):
            rc, alen, res, buf, said = c.run(method, cap)
            assert rc == E_INVALID and "archive buffer too small" in said, cap


def test_groups(encoder, text):
    """batch_mib = 1 on 100 entries of 16 KiB: four groups; an entry of 4 MiB + 1 between small ones: a group, the entry alone, a group; exactly one
    small entry: the single-stream path.  The bytes of the host path, whose own grouping the knob changes the same way."""
    za = product()
    m = za.Method.Deflate_1
    small = [text[3000 * k:3000 * k + 16384] for k in range(100)]
    big = (text * 8)[:MIB4 + 1]
    lists = {"small": small, "big between": small[:3] + [big] + small[3:6], "one": [small[7][:5000]], "one stored": [bytes(range(256))], "big first and last": [big, small[0], big[1:]]}
    want = {nm: host_archive(encoder, m, names_for(d), d) for nm, d in lists.items()}
    try:
        for mib in (1, 512):
            encoder.set_knob("batch_mib", mib)
            for nm, datas in lists.items():
                c = Call(encoder, names_for(datas), datas)
                rc, alen, res, buf, said = c.run(m, c.bound())
                assert rc == 0, (nm, said)
                assert alen == len(want[nm][0]) and buf[:alen].tobytes() == want[nm][0], (nm, mib)
                same_results(res, want[nm][1], datas)
            if mib == 1:                                   # the knob changes no byte of the host path either
                assert host_archive(encoder, m, names_for(small), small)[0] == want["small"][0]
    finally:
        encoder.set_knob("batch_mib", 512)
    assert [int(e["zip_type"]) for e in want["one stored"][1]] == [0]


def test_entries_that_run_alone_at_the_exact_capacity(encoder, text):
    """The single-stream path at cap = archive_len and below it: a small and a large (4 MiB + 1) incompressible entry, which come out stored, and a
    large compressible one; at an aligned and an unaligned address; with span_mib = 1 the aligned large entries go through deflate_spans, straight
    to their place.  One byte short, a capacity that ends inside the payload and one that ends ten bytes behind the header are all 'archive buffer
    too small' with the guards intact."""
    za = product()
    m = za.Method.Deflate_1
    rng = np.random.default_rng(11)
    lists = {"small random": rng.integers(0, 256, 4096, dtype=np.uint8).tobytes(), "big random": rng.integers(0, 256, MIB4 + 1, dtype=np.uint8).tobytes(),
             "big text": (text * 8)[:MIB4 + 1]}
    want = {nm: host_archive(encoder, m, names_for([d]), [d]) for nm, d in lists.items()}
    assert [want[nm][1][0]["zip_type"] for nm in lists] == [0, 0, 8]
    try:
        for span in (2048, 1):
            encoder.set_knob("span_mib", span)
            for nm, d in lists.items():
                arc, entries = want[nm]
                pay = 30 + len(names_for([d])[0])
                for a in (0, 5):
                    c = Call(encoder, names_for([d]), [d], a_arc=a, a_in=[a])
                    rc, alen, res, buf, said = c.run(m, len(arc))
                    assert rc == 0 and alen == len(arc), (nm, span, a, said)
                    assert buf.tobytes() == arc, (nm, span, a)
                    same_results(res, entries, [d])
                    for cap in (len(arc) - 1, pay + entries[0]["csize"] - 1, pay + 10):
                        rc, alen, res, buf, said = c.run(m, cap)
                        assert rc == E_INVALID and "archive buffer too small" in said, (nm, span, a, cap, said)
    finally:
        encoder.set_knob("span_mib", 2048)


def test_timing_of_all_groups(encoder, text):
    """last_timing after a call of several groups holds the launches of all of them, every name once: a group of three small entries in front of an
    entry of 4 MiB + 1, which runs alone and last, still shows the group's k_zw_pack and k_zw_place."""
    za = product()
    datas = [text[3000 * k:3000 * k + 16384] for k in range(3)] + [(text * 8)[:MIB4 + 1]]
    c = Call(encoder, names_for(datas), datas)
    rc, alen, res, buf, said = c.run(za.Method.Deflate_1, c.bound())
    assert rc == 0, said
    marks = encoder.last_timing()
    assert len(dict(marks)) == len(marks) and "zip:k_zw_pack" in dict(marks) and "zip:k_zw_place" in dict(marks)


def test_zip64(encoder, plains):
    za = product()
    # offsets across 2 ** 32 - 1: the entries beyond it get the extension, the archive the Zip64 end record and locator
    base = 2 ** 32 - 100
    datas = plains[3:9]
    for method in (za.Method.Deflate_1, za.Method.Store):
        want, entries = host_archive(encoder, method, names_for(datas), datas, base=base)
        c = Call(encoder, names_for(datas), datas)
        rc, alen, res, buf, said = c.run(method, c.bound(base), base=base)
        assert rc == 0, said
        assert alen == len(want) and buf[:alen].tobytes() == want and b"PK\x06\x06" in want and b"PK\x06\x07" in want
        same_results(res, entries, datas)
        assert entries[0]["offset"] == base and entries[-1]["offset"] >= 0xFFFFFFFF      # (the first header lies just below the limit, the later ones beyond it)
    # 65 535 empty entries: the promotion by the number of entries; method Store has no LZ buffer
    n = 65535
    names = ["%x" % k for k in range(n)]
    datas = [b""] * n
    want, entries = host_archive(encoder, za.Method.Store, names, datas)
    c = Call(encoder, names, datas)
    rc, alen, res, buf, said = c.run(za.Method.Store, c.bound())
    assert rc == 0, said
    assert alen == len(want) and buf[:alen].tobytes() == want and want.count(b"PK\x06\x06") == 1
    assert np.array_equal(res["offset"], np.array([e["offset"] for e in entries], dtype=np.uint64)) and not res["crc"].any() and not res["csize"].any()
    one_less, _ = host_archive(encoder, za.Method.Store, names[:-1], datas[:-1])
    assert b"PK\x06\x06" not in one_less
    rc, alen, res, buf, said = c.run(za.Method.Store, c.bound(), tab=c.tab[:-1])
    assert rc == 0 and buf[:alen].tobytes() == one_less


def test_refusals(encoder, plains):
    """Every refusal with its text and index; nothing is launched: the archive buffer is still its fill pattern.  A valid call follows each."""
    za = product()
    datas = plains[4:8]
    names = names_for(datas)
    m = za.Method.Deflate_1
    want, _ = host_archive(encoder, m, names, datas)
    c = Call(encoder, names, datas)
    cap = c.bound()
    c.run(m, cap)
    cases = []
    for who in range(len(datas)):
        t = c.tab.copy(); t["d_data"][who] = 0
        cases.append((m, t, E_INVALID, "entry %d: null d_data" % who))
        t = c.tab.copy(); t["name_len"][who] = 65536
        cases.append((m, t, E_INVALID, "entry %d: a name longer than 65 535" % who))
        t = c.tab.copy(); t["n"][who] = 1 << 40
        cases.append((m, t, E_TOO_LARGE, "entry %d: an entry of 1 TiB" % who))
    for bad, nm in ((za.Method.BZip2_1, "BZip2_1"), (za.Method.BZip2_3, "BZip2_3"), (za.Method.LZMA_0, "LZMA_0"), (za.Method.LZMA_3, "LZMA_3"), (za.Method.LZMA_for_PNG, "LZMA_for_PNG"),
                    (za.Method.Preselection_1, "Preselection_1"), (za.Method.Preselection_2, "Preselection_2"), (za.Method.Shrink_1, "Shrink_1"), (za.Method.Reduce_1, "Reduce_1"),
                    (za.Method.Reduce_4, "Reduce_4"), (99, "unknown"), (-1, "unknown")):
        cases.append((bad, c.tab, E_INVALID, "method %d (%s)" % (bad, nm)))
    for method, t, want_rc, want_text in cases:
        rc, alen, res, buf, said = c.run(method, cap, tab=t)
        assert rc == want_rc and want_text in said, (rc, said)
        assert not np.flatnonzero(buf != GUARD).size                               # the checks come before anything touches the device
    # an input that overlaps the archive buffer: its first byte, its last byte, all of it
    import torch
    t_arc = torch.full((cap + 2 * G,), GUARD, dtype=torch.uint8, device="cuda")
    d_arc = t_arc.data_ptr() + G
    for who, (a, n) in enumerate(((d_arc - 4, 5), (d_arc + cap - 1, 9), (d_arc + 100, 50), (d_arc - G, cap + 2 * G))):
        t = c.tab.copy(); t["d_data"][who] = a; t["n"][who] = n
        res = np.zeros(len(t), dtype=za.Encoder.zip_dtypes()[1])
        alen = ctypes.c_uint64(0)
        rc = encoder.lib.zada_zip_device(encoder.ctx, m, len(t), t.ctypes.data, d_arc, cap, 0, ctypes.byref(alen), res.ctypes.data)
        assert rc == E_INVALID and "entry %d: its input overlaps the archive buffer" % who in encoder.lib.zada_last_error(encoder.ctx).decode()
        assert not np.flatnonzero(t_arc.cpu().numpy() != GUARD).size
    for a, n in ((d_arc - 5, 5), (d_arc + cap, 9)):                                  # ranges that only touch it are fine
        t = c.tab.copy(); t["d_data"][0] = a; t["n"][0] = n
        res = np.zeros(len(t), dtype=za.Encoder.zip_dtypes()[1])
        assert encoder.lib.zada_zip_device(encoder.ctx, m, len(t), t.ctypes.data, d_arc, cap, 0, ctypes.byref(alen), res.ctypes.data) == 0
    # a valid call still works; count = 0 gives the 22-byte end record
    rc, alen, res, buf, said = c.run(m, cap)
    assert rc == 0 and buf[:alen].tobytes() == want
    rc, alen, res, buf, said = c.run(m, 22, tab=c.tab[:0])
    assert rc == 0 and alen == 22 and buf.tobytes() == host_archive(encoder, m, [], [])[0] and encoder.zip_bound(c.tab[:0]) >= 22
    rc, alen, res, buf, said = c.run(m, 21, tab=c.tab[:0])
    assert rc == E_INVALID and "archive buffer too small" in said
    with pytest.raises(za.ZadaError):
        encoder.zip_device(c.tab, d_arc, cap, za.Method.BZip2_2)


def test_write_device_round_trip(encoder, plains):
    import torch
    za = product()
    names = names_for(plains)
    uz = za.UnZip(encoder)
    for method in (za.Method.Deflate_3, za.Method.Store):
        want, entries = host_archive(encoder, method, names, plains, key=("plains", method))
        tensors = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() if len(d) else torch.empty(0, dtype=torch.uint8) for d in plains]
        zc = za.ZipCreate(encoder, method)
        arc = zc.write_device(names, tensors)
        assert arc.device.type == "cuda" and arc.dtype == torch.uint8 and bytes(arc.cpu().numpy()) == want
        assert zc.entries == entries
        with pytest.raises(ValueError):
            zc.write_device(names, tensors)
        info = za.ZipInfo.load_device(arc)
        got = uz.extract_device(info)
        assert list(got) == names and all(torch.equal(got[nm].cpu(), t.cpu()) for nm, t in zip(names, tensors))
        with zipfile.ZipFile(io.BytesIO(bytes(arc.cpu().numpy()))) as z:
            assert z.testzip() is None and z.namelist() == names
    # names are normalised as add_compressed does; the time and the flag bit are the caller's
    zc = za.ZipCreate(encoder, za.Method.Deflate_1, _offset_bias=77)
    arc = zc.write_device(["a\\b\\c.txt", "é.bin"], tensors[5:7], file_time=0x12345678, unicode_name=False)
    ref = za.ZipCreate(encoder, za.Method.Deflate_1, _offset_bias=77)
    ref.add_streams(["a\\b\\c.txt", "é.bin"], plains[5:7], file_time=0x12345678, unicode_name=False)
    assert bytes(arc.cpu().numpy()) == ref.finish() and zc.entries == ref.entries
    assert bytes(za.ZipCreate(encoder, za.Method.Deflate_1).write_device([], []).cpu().numpy()) == za.ZipCreate(encoder, za.Method.Deflate_1).finish()
    used = za.ZipCreate(encoder, za.Method.Deflate_1)
    used.add_streams(names[:1], plains[:1])
    with pytest.raises(ValueError):
        used.write_device(names, tensors)
    with pytest.raises(za.ZadaError):
        za.ZipCreate(encoder, za.Method.Deflate_1).write_device(names[:1], [torch.zeros(5, dtype=torch.uint8)])       # a tensor that is not on the encoder's device
    with pytest.raises(za.ZadaError):
        za.ZipCreate(encoder, za.Method.LZMA_1).write_device(names, tensors)


def test_order_independence_on_one_context(encoder, plains, text):
    """A zada_zip_device call between two zada_deflate_batch calls leaves their results equal: the workspace is shared."""
    za = product()
    datas = [text[5000 * k:5000 * k + 20000 + 977 * k] for k in range(12)]
    m = za.Method.Deflate_2
    first = encoder.deflate_batch(datas, m)
    names = names_for(plains)
    for method in (za.Method.Deflate_1, za.Method.Store, za.Method.Deflate_2):
        want, _ = host_archive(encoder, method, names, plains, key=("plains", method))
        c = Call(encoder, names, plains)
        rc, alen, res, buf, said = c.run(method, c.bound())
        assert rc == 0 and buf[:alen].tobytes() == want
        assert encoder.deflate_batch(datas, m) == first
    one = encoder.deflate(datas[3], m)
    c.run(za.Method.Deflate_2, c.bound())
    assert encoder.deflate(datas[3], m) == one
