"""Helpers of the zada_zip_device_ex tests: the inputs, the reference (ZipCreate.add_streams + finish on host bytes, which test_oracle.py and
test_gpu_crypt.py pin to the oracle and to the CPU model of ZipCrypto) and one call of the C entry point on guarded tensors."""
import ctypes
import zlib

import numpy as np

from _common import product, silesia_mix
from _devbuf import GUARD, guard_damage

E_INVALID, E_TOO_LARGE = -1, -4
FILL, G = 0x3C, 64
LENGTHS = (0, 1, 2, 3, 31, 255, 4095, 32767, 32768, 32769, 65537, 100000)

_text = []


def text():
    if not _text:
        _text.append(silesia_mix(300000, class_mask=1) + silesia_mix(300000))
    return _text[0]


def plain_list():
    """The lengths of the issue cut from the generators' text, 4 KiB of random bytes (which must come out stored) and an all-zero entry."""
    t = text()
    out = [t[1000 * k:1000 * k + n] for k, n in enumerate(LENGTHS)]
    out.append(np.random.default_rng(7).integers(0, 256, 4096, dtype=np.uint8).tobytes())
    out.append(bytes(50000))
    return out


def names_for(datas, ext="bin"):
    return ["dir/e%03d_%d.%s" % (k, len(d), ext) for k, d in enumerate(datas)]


def headers_for(n, seed=5):
    """eleven fixed 'random' bytes per entry"""
    return [np.random.default_rng(seed + k).integers(0, 256, 11, dtype=np.uint8).tobytes() for k in range(n)]


_host = {}


def host_archive(enc, method, names, datas, base=0, key=None, password=None, headers=None, **kw):
    """The reference: ZipCreate (enc, method).add_streams + finish.  -> (archive bytes, entries); kept under `key` for the tests that share it."""
    if key is not None and key in _host:
        return _host[key]
    zc = product().ZipCreate(enc, method, _offset_bias=base)
    zc.add_streams(names, datas, password=password, _headers=headers, **kw)
    r = (zc.finish(), zc.entries)
    if key is not None:
        _host[key] = r
    return r


class CallEx:
    """One zada_zip_device_ex call on fresh tensors: input k at offset a_in [k] modulo 16 -- (5 k + 3) mod 16 by default -- in one arena of FILL, the
    archive buffer at offset G + a_arc of a tensor of GUARD with at least G guard bytes on both sides.  run () asserts that no guard byte and no byte
    of the arena changed."""

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

    def bound(self, base=0, encrypted=False):
        return self.enc.zip_bound_ex(self.tab, base, encrypted)

    def run(self, method, cap, base=0, tab=None, password=None, headers=None, crypt=None, old=False):
        """-> (rc, archive_len, results, the cap bytes of the archive buffer, the error text).  crypt: a ready (password address, length, random11
        address) triple instead of password / headers; old: the call is zada_zip_device."""
        import torch
        tab = self.tab if tab is None else tab
        self.t_arc = torch.full((self.a_arc + cap + G,), GUARD, dtype=torch.uint8, device="cuda")
        res = np.zeros(len(tab), dtype=product().Encoder.zip_dtypes()[1])
        alen = ctypes.c_uint64(0)
        keep = None
        if password is not None:
            pw = password.encode("latin-1") if isinstance(password, str) else bytes(password)
            keep = (ctypes.create_string_buffer(pw, len(pw)), ctypes.create_string_buffer(b"".join(headers), max(11 * len(headers), 1)))
            crypt = (ctypes.addressof(keep[0]), len(pw), ctypes.addressof(keep[1]))
        cr = (ctypes.c_uint64 * 3)(*crypt) if crypt is not None else None
        torch.cuda.synchronize()
        lib, args = self.enc.lib, (self.enc.ctx, method, len(tab), tab.ctypes.data if len(tab) else None, self.t_arc.data_ptr() + self.a_arc, cap, base)
        if old:
            rc = lib.zada_zip_device(*args, ctypes.byref(alen), res.ctypes.data if len(tab) else None)
        else:
            rc = lib.zada_zip_device_ex(*args, ctypes.addressof(cr) if cr is not None else None, ctypes.byref(alen), res.ctypes.data if len(tab) else None)
        said = lib.zada_last_error(self.enc.ctx).decode()
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


def check_equal(enc, method, names, datas, a_arc=0, password=None, headers=None, key=None, base=0, too_small=True):
    """The whole contract of one list: the archive at cap = archive_len exactly equals the reference, so do the results; the bound is one; one byte
    less is 'archive buffer too small'.  -> (the reference's archive, its entries, the results)"""
    want, entries = host_archive(enc, method, names, datas, base=base, key=key, password=password, headers=headers)
    c = CallEx(enc, names, datas, a_arc=a_arc)
    assert c.bound(base, password is not None) >= len(want)
    if too_small:                                  # (first, so that last_timing afterwards is the good call's)
        rc, _, _, _, said = c.run(method, len(want) - 1, base=base, password=password, headers=headers)
        assert rc == E_INVALID and "archive buffer too small" in said, (rc, said)
    rc, alen, res, buf, said = c.run(method, len(want), base=base, password=password, headers=headers)
    assert rc == 0, said
    assert alen == len(want)
    assert buf.tobytes() == want, "first difference at byte %d of %d" % (next(i for i, (x, y) in enumerate(zip(buf.tobytes(), want)) if x != y), len(want))
    same_results(res, entries, datas)
    return want, entries, res


# the LZMA methods whose properties liblzma (zipfile) refuses: lc + lp > 4
NOT_FOR_LIBLZMA = (19, 20, 23, 24, 25, 26, 27, 28, 30)


def zipfile_reads_back(archive, names, datas, methods, pwd=None, least=1):
    """zipfile reads every entry back equal to its input -- but for compressed entries of an LZMA method whose properties liblzma does not take (the
    reference writes them, UnZip reads them; the callers check those through extract_device)."""
    import io
    import zipfile
    read = 0
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        for nm, d, m, info in zip(names, datas, methods, z.infolist()):
            if info.compress_type == 14 and m in NOT_FOR_LIBLZMA:
                continue
            assert z.read(info, pwd=pwd) == d, nm
            read += 1
    assert read >= least
