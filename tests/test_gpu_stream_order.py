"""Device calls behind work that is still queued on a torch stream.

Every device-side entry point takes memory that PyTorch produced, and in real use that memory is rarely settled when the call is made.  The contract
(include/zada.h, "Context = device + stream + workspace"): work queued on the legacy default stream before a call is ordered before the call's
accesses; work on any other stream is the caller's to finish, which the tensor-taking Python methods do for torch's current stream; every call
returns with its work complete.  Here every input of a call is made by tests/_streams.py::pending_fill -- a delay, a gate event, the copy of B over
the stale content A, a done event -- and the call is entered while the gate has provably not fired (a fired gate fails the case).  The result
must be B's, by references that do not come from the call under test: the source bytes, zipfile, zlib, bz2, lzma, the oracle and the CPU models
the sibling tests load, bytes.find's literal model of tests/_findzip.py.

  (a) the tensor-taking methods (_streams.TENSOR_METHODS) on a side stream, with no synchronisation of the test's own; the returned tensors are
      consumed on that stream at once, which pins that the call returns with its own work complete;
  (b) the raw-pointer entry points behind a producer on torch's default stream, with no host synchronisation, at input alignment 0 and 5;
  (c) the test of the test: write_device (Store) with the package's own synchronisation replaced by a no-op reads the stale content whole --
      a missing synchronisation is seen by the cases of (a).

A and B are valid inputs of the call, of one length, and differ in every entry that has a byte."""
import hashlib
import io
import zipfile
import zlib

import numpy as np
import pytest

import _streams as S
from _common import oracle_deflate, oracle_zip, product, silesia_mix

pytestmark = pytest.mark.gpu

FF = 0xFFFFFFFF
PW = b"stream order"
_cache = {}


def crc_reg(d):
    return zlib.crc32(d) ^ FF


@pytest.fixture(scope="module")
def side():
    import torch
    S.calibrate()
    return torch.cuda.Stream()


def _lists():
    if "lists" not in _cache:
        _cache["lists"] = S.entry_lists()
    return _cache["lists"]


def _names(datas, ext="bin"):
    return ["dir/e%02d_%d.%s" % (k, len(d), ext) for k, d in enumerate(datas)]


def _host(t):
    return t.cpu().numpy().tobytes()


def _enter(gate, what):
    assert not gate.query(), S.fired(what)


def _attach(info, t):
    """a ZipInfo read from host bytes, pointed at the tensor that will hold them: the method under test is the first to touch the tensor"""
    info.data, info.device_data = None, t
    return info


# ---- (a) the tensor-taking methods on a side stream ---------------------------------------------------------------------------------------------
def _read_back(archive, names, datas, pwd=None):
    """every entry as a CPU reader gives it: zipfile, and tests/legacy's model for the Shrink entries zipfile does not take"""
    import _legacy as L
    from _orders import parse_zip
    rows, _ = parse_zip(archive)
    assert [r["raw_name"] for r in rows] == [nm.encode() for nm in names]
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        for r, info, nm, d in zip(rows, z.infolist(), names, datas):
            if r["method"] == 1:
                assert (L.unshrink(r["payload"], r["usize"]), r["crc"]) == (d, zlib.crc32(d)), nm
            else:
                assert z.read(info, pwd=pwd) == d, nm
    return {r["method"] for r in rows}


def _write(enc, s, method, ex=False, want_equal=True, types=None, **kw):
    import torch
    from _zipdev import headers_for, host_archive
    za = product()
    A, B = _lists()
    names = _names(B, "txt")
    if kw.get("password"):
        kw["_headers"] = headers_for(len(B))
    want = None
    if want_equal:                                            # (the reference runs first: it uses the device, and waits for it)
        hk = {k.lstrip("_"): v for k, v in kw.items() if k != "legacy"}
        want, entries = host_archive(enc, method, names, B, key=("stream order", method, bool(kw)), **hk)
    zc = za.ZipCreate(enc, method)
    with torch.cuda.stream(s):
        tensors, gate, done = S.pending_entries(A, B, s)
        _enter(gate, "write_device")
        arc = zc.write_device_ex(names, tensors, **kw) if ex else zc.write_device(names, tensors)
        assert done.query(), "the method returned before the work queued on the current stream was complete"
        got = _host(arc.clone())
    if want is not None:
        assert got == want, "the archive is not the one add_streams + finish write for B"
        assert zc.entries == entries
    seen = _read_back(got, names, B, pwd=kw.get("password"))
    assert types is None or seen >= types, seen


def _archives(kind):
    """(A, B, the entries of B): two archives of one length by zipfile; kind "deflate": Store and Deflate entries, "bzlz": BZip2 and LZMA entries too"""
    if ("arc", kind) not in _cache:
        A, B = _lists()
        names = _names(B)
        if kind == "deflate":
            methods = [zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED] * 4
        else:
            methods = [zipfile.ZIP_BZIP2, zipfile.ZIP_LZMA, zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED] * 2
        a, b = S.padded_archives(lambda ents, comment: S.zipfile_archive(ents, methods, comment), list(zip(names, A)), list(zip(names, B)))
        _cache["arc", kind] = (a, b, list(zip(names, B)))
    return _cache["arc", kind]


def _extract(enc, s, kind, through_load, test_only=False):
    import torch
    za = product()
    a, b, entries = _archives(kind)
    host_info = za.ZipInfo.load(b)
    reader = za.UnZip(enc, bzip2=kind == "bzlz", lzma=kind == "bzlz")
    with torch.cuda.stream(s):
        t, gate, done = S.pending_tensor(a, b, s)
        if through_load:
            _enter(gate, "ZipInfo.load_device")
            info = za.ZipInfo.load_device(t)
            assert done.query(), "load_device returned before the work queued on the current stream was complete"
            assert [(e.name, e.crc, e.usize, e.data_offset) for e in info.entries] == [(e.name, e.crc, e.usize, e.data_offset) for e in host_info.entries]
        else:
            info = _attach(host_info, t)
            _enter(gate, "UnZip.extract_device")
        res = reader.extract_device(info, test_only=test_only)
        assert done.query(), "the method returned before the work queued on the current stream was complete"
        got = {nm: (v if v is None else _host(v.clone())) for nm, v in res.items()}
    assert got == {nm: (None if test_only else d) for nm, d in entries}


def _compare(enc, s):
    import torch
    import _rezip
    za = product()
    A, B = _lists()
    names = _names(B)
    k, at = 2, 3210                                           # the entry and the byte in which archive 2 differs once the fill has run
    changed = B[k][:at] + bytes([B[k][at] ^ 0x20]) + B[k][at + 1:]
    m1 = [zipfile.ZIP_DEFLATED] * len(B)
    m2 = [zipfile.ZIP_STORED if i == k else zipfile.ZIP_DEFLATED for i in range(len(B))]
    arc1 = S.zipfile_archive(list(zip(names, B)), m1)
    stale = S.zipfile_archive(list(zip(names, B)), m2)
    other = [changed if i == k else d for i, d in enumerate(B)]
    fresh = S.zipfile_archive(list(zip(names, other)), m2)
    assert len(stale) == len(fresh) and stale != fresh
    counters, verdicts = _rezip.comp_zip([(nm.encode(), d) for nm, d in zip(names, B)], [(nm.encode(), d) for nm, d in zip(names, other)])
    assert counters["compare_failures"] == 1 and (names[k].encode(), za.CZ_DIFFERENT, at + 1) in verdicts
    info2 = za.ZipInfo.load(fresh)
    t1 = torch.from_numpy(np.frombuffer(arc1, dtype=np.uint8).copy()).cuda()
    info1 = za.ZipInfo.load_device(t1)
    with torch.cuda.stream(s):
        t2, gate, done = S.pending_tensor(stale, fresh, s)
        _attach(info2, t2)
        _enter(gate, "CompZip.compare_device")
        r = za.CompZip(enc).compare_device(info1, info2)
        assert done.query(), "the method returned before the work queued on the current stream was complete"
    assert ({c: getattr(r, c) for c in counters}, [(e[5], e[1], e[2]) for e in r.entries], r.damaged) == (counters, verdicts, 0)


def _rezip_case(enc, s):
    import torch
    za = product()
    a, b, entries = _archives("deflate")
    info = za.ZipInfo.load(b)
    with torch.cuda.stream(s):
        t, gate, done = S.pending_tensor(a, b, s)
        _attach(info, t)
        _enter(gate, "ReZip.rezip_device")
        arc = za.ReZip(enc).rezip_device(info, approaches=("deflate_3", "bzip2_1"))
        assert done.query(), "the method returned before the work queued on the current stream was complete"
        got = _host(arc.clone())
    with zipfile.ZipFile(io.BytesIO(got)) as z:
        assert {i.filename: z.read(i) for i in z.infolist()} == dict(entries)


def _find(enc, s):
    import torch
    import _findzip
    za = product()
    A, B = _lists()
    names = _names(B)
    needle = b"Gate Event"

    def planted(datas, where):
        out = []
        for k, d in enumerate(datas):
            d = bytearray(d.replace(b"g", b"q").replace(b"G", b"Q"))        # (no occurrence of its own)
            for o in where.get(k, ()):
                d[o:o + len(needle)] = needle if o % 2 else needle.upper()
            out.append(bytes(d))
        return out
    ea, eb = planted(A, {0: (10,), 2: (100, 4090)}), planted(B, {0: (500, 1000), 4: (3,), 6: (4087, 4000, 17), 7: (1490,)})
    methods = [zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED] * 4
    stale, fresh = S.padded_archives(lambda ents, comment: S.zipfile_archive(ents, methods, comment), list(zip(names, ea)), list(zip(names, eb)))
    wa, wb = (_findzip.find_zip([(nm.encode(), d) for nm, d in zip(names, e)], needle, True) for e in (ea, eb))
    assert sum(o for _, o, _ in wa[0]) == 3 and sum(o for _, o, _ in wb[0]) == 7
    info = za.ZipInfo.load(fresh)
    with torch.cuda.stream(s):
        t, gate, done = S.pending_tensor(stale, fresh, s)
        _attach(info, t)
        _enter(gate, "FindZip.find_device")
        r = za.FindZip(enc).find_device(info, needle)
        assert done.query(), "the method returned before the work queued on the current stream was complete"
    assert ([(e[4], e[1], e[2]) for e in r.entries if e[1] > 0], r.in_names, r.lines(), r.damaged) == (wb[0], wb[1], wb[2], 0)


def trained_inputs():
    """(trainer, A data, B data): six entries each, pairwise of one length, one empty"""
    import _trained
    trainer = _trained.fixture("wsbase.csv")[:6000]
    src = _trained.fixture("wm1ns.csv")
    lens = (600, 1, 0, 450, 300, 77)
    B = [src[400 * k:400 * k + n] for k, n in enumerate(lens)]
    A = [src[20000 + 400 * k:20000 + 400 * k + n] for k, n in enumerate(lens)]
    assert all(a != b for a, b in zip(A, B) if a)
    return trainer, A, B


def stale_messages(trainer, skip, messages, caps):
    """Per message of B a valid message of the same length that holds other data of at most caps [i] bytes (the oracle's, tests/_trained.py); the
    empty entry's message has no other of its length: it stays."""
    import _trained
    if "stale messages" in _cache:
        return _cache["stale messages"]
    src = _trained.fixture("wm2ns.csv")
    out = []
    for k, (m, cap) in enumerate(zip(messages, caps)):
        found = m if cap == 0 else None
        for o in range(0, 30000, 1500):
            if found is not None:
                break
            for n in range(cap, max(cap - 200, 0), -1):
                c = _trained.message_of(trainer, src[o + 300 * k:o + 300 * k + n], skip)
                if len(c) == len(m) and c != m:
                    found = c
                    break
                if len(c) < len(m) - 8:
                    break
        assert found is not None, "no stale message of %d bytes for entry %d" % (len(m), k)
        out.append(found)
    _cache["stale messages"] = out
    return out


def _trained_case(enc, s):
    import torch
    za = product()
    trainer, A, B = trained_inputs()
    tc = td = None
    try:
        tc = za.TrainedCompression(enc, trainer)
        want = tc.encode(B)                                   # the host path, on settled bytes
        caps = [len(b) + 64 for b in B]
        stale = stale_messages(trainer, tc.skip, want, [len(b) + 64 if b else 0 for b in B])
        td = za.TrainedCompression.for_decoding(enc, tc.stub, tc.skip, tc.trainer_len)
        with torch.cuda.stream(s):
            tensors, gate, done = S.pending_entries(A, B, s)
            _enter(gate, "TrainedCompression.encode_device")
            msgs = tc.encode_device(tensors)
            assert done.query(), "the method returned before the work queued on the current stream was complete"
            got = [_host(m.clone()) for m in msgs]
        assert got == want, "the messages are not those of B"
        with torch.cuda.stream(s):
            tensors, gate, done = S.pending_entries(stale, want, s)
            _enter(gate, "TrainedCompression.decode_device")
            outs = td.decode_device(tensors, caps)
            assert done.query(), "the method returned before the work queued on the current stream was complete"
            back = [_host(o.clone()) for o in outs]
        assert back == B
    finally:
        for h in (tc, td):
            if h is not None:
                h.close()


RUNNERS = {
    "write_device(Store)": lambda enc, s: _write(enc, s, 0, types={0}),
    "write_device(Deflate_Fixed)": lambda enc, s: _write(enc, s, 6, types={0, 8}),
    "write_device(Deflate_1)": lambda enc, s: _write(enc, s, 8, types={0, 8}),
    "write_device_ex(BZip2_1)": lambda enc, s: _write(enc, s, 12, ex=True, types={0, 12}),
    "write_device_ex(LZMA_1)": lambda enc, s: _write(enc, s, 16, ex=True, types={0, 14}),
    "write_device_ex(Deflate_1, password)": lambda enc, s: _write(enc, s, 8, ex=True, types={0, 8}, password=PW),
    "write_device_ex(Shrink_1, legacy)": lambda enc, s: _write(enc, s, 1, ex=True, want_equal=False, types={0, 1}, legacy=True),
    "load_device + extract_device(Store, Deflate)": lambda enc, s: _extract(enc, s, "deflate", True),
    "load_device + extract_device(BZip2, LZMA)": lambda enc, s: _extract(enc, s, "bzlz", True),
    "extract_device(Store, Deflate)": lambda enc, s: _extract(enc, s, "deflate", False),
    "extract_device(Store, Deflate, test_only)": lambda enc, s: _extract(enc, s, "deflate", False, test_only=True),
    "extract_device(BZip2, LZMA)": lambda enc, s: _extract(enc, s, "bzlz", False),
    "extract_device(BZip2, LZMA, test_only)": lambda enc, s: _extract(enc, s, "bzlz", False, test_only=True),
    "compare_device(second archive pending)": _compare,
    "rezip_device(deflate_3, bzip2_1)": _rezip_case,
    "find_device(needle)": _find,
    "trained encode_device + decode_device": _trained_case,
}


@pytest.mark.parametrize("case", S.tensor_cases())
def test_tensor_methods_wait_for_the_current_stream(encoder, side, case):
    RUNNERS[case](encoder, side)


# ---- (c) the test of the test -------------------------------------------------------------------------------------------------------------------
class _NoSynchronisation:
    def synchronize(self):
        pass


def test_a_missing_synchronisation_is_seen(encoder, side, monkeypatch):
    """write_device (Store) with the package's own synchronisation taken away for that one call: the call returns while the producer's gate has
    still not fired -- the fill had not begun, so nothing races -- and the archive holds exactly the stale content A.  Store only: any stale bytes
    are valid input.  Every case of (a) would see the same: its result would be A's, not B's."""
    import torch
    from _zipdev import host_archive
    za = product()
    A, B = _lists()
    names = _names(B, "txt")
    want_a, _ = host_archive(encoder, 0, names, A, key=("stream order, stale", 0))
    want_b, _ = host_archive(encoder, 0, names, B, key=("stream order", 0, False))
    assert want_a != want_b and len(want_a) == len(want_b)
    zc = za.ZipCreate(encoder, 0)
    with torch.cuda.stream(side):
        tensors, gate, done = S.pending_entries(A, B, side)
        _enter(gate, "write_device without its synchronisation")
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "current_stream", lambda *a, **k: _NoSynchronisation())
            arc = zc.write_device(names, tensors)
        assert not gate.query(), S.fired("write_device without its synchronisation (after the call)")
        got = _host(arc.clone())
    assert got == want_a, "without the synchronisation the archive must hold the stale content, whole"


# ---- (b) the raw-pointer entry points behind the default stream ------------------------------------------------------------------------------------
ALIGN = (0, 5)


def _behind_default(fn, stale, fresh, cap, a_in, what):
    """fn (d_in, n, d_out, cap) with the input pending on torch's default stream and no host synchronisation -> (what fn returns, the cap output
    bytes, the input tensor's n bytes afterwards)"""
    import torch
    st = torch.cuda.default_stream()
    t_out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    t_in, gate, done = S.pending_tensor(stale, fresh, st, a_in)
    _enter(gate, what)
    r = fn(t_in.data_ptr() + a_in, len(fresh), t_out.data_ptr(), cap)
    assert done.query(), "%s returned before the work queued on the default stream in front of it was complete" % what
    return r, _host(t_out)[:cap], _host(t_in)[a_in:a_in + len(fresh)]


def _pair(n, k=0):
    """two pieces of n bytes of the mixed stream"""
    if "mix" not in _cache:
        _cache["mix"] = silesia_mix(1 << 20, version=2)
    mix = _cache["mix"]
    return mix[300000 + 7000 * k:300000 + 7000 * k + n], mix[10000 + 7000 * k:10000 + 7000 * k + n]


def _encoder_case(name):
    """-> (stale, fresh, cap, fn (enc) -> device call, want (rc, stream, CRC register))"""
    import _legacy as L
    if name.startswith("deflate"):
        m = {"deflate Deflate_Fixed": 6, "deflate Deflate_1": 8, "deflate Deflate_R": 11}[name]
        a, b = _pair(5000, m)
        if m == 11:
            import _rich
            rc, s = _rich.deflate_r(b)
            want = (rc, s, crc_reg(b))
        else:
            want = oracle_deflate(b, m)
        return a, b, len(b) + 64, lambda enc: (lambda di, n, do, cap: enc.deflate_device(di, n, do, cap, m)), want
    if name == "bzip2 BZip2_1":
        from _bzip2 import oracle_encode
        a, b = _pair(5000, 1)
        return a, b, len(b) + 4096, lambda enc: (lambda di, n, do, cap: enc.bzip2_device(di, n, do, cap, 12)), (0, oracle_encode(b, 0)[0], crc_reg(b))
    if name == "bzip2 BZip2_1, three blocks":
        # above one block of 100 000 bytes, "bz_pipeline" at its default: the entropy stage runs on a worker thread's non-blocking stream
        from _bzip2 import oracle_encode
        a, b = _pair(250001, 2)
        return a, b, len(b) + 4096, lambda enc: (lambda di, n, do, cap: enc.bzip2_device(di, n, do, cap, 12)), (0, oracle_encode(b, 0)[0], crc_reg(b))
    if name == "lzma LZMA_1":
        from _lzmah import oracle_lzma
        a, b = _pair(4500, 3)
        return a, b, len(b) + 4096, lambda enc: (lambda di, n, do, cap: enc.lzma_device(di, n, do, cap, 16)), oracle_lzma(b, 16)
    if name == "shrink":
        a, b = L.edge_input(5000, seed=81), L.edge_input(5000, seed=82)
        return a, b, len(b), lambda enc: (lambda di, n, do, cap: enc.shrink_device(di, n, do, cap)), L.model_result(b, 1)
    if name == "reduce Reduce_1":
        a, b = L.edge_input(1000, seed=83), L.edge_input(1000, seed=84)
        return a, b, len(b), lambda enc: (lambda di, n, do, cap: enc.reduce_device(di, n, do, cap, 2)), L.model_result(b, 2)
    raise KeyError(name)


ENCODERS = ("deflate Deflate_Fixed", "deflate Deflate_1", "deflate Deflate_R", "bzip2 BZip2_1", "lzma LZMA_1", "shrink", "reduce Reduce_1",
            "bzip2 BZip2_1, three blocks")


@pytest.mark.parametrize("a_in", ALIGN)
@pytest.mark.parametrize("name", ENCODERS)
def test_encoders_on_pointers_behind_the_default_stream(encoder, name, a_in):
    if (name, "case") not in _cache:
        _cache[name, "case"] = _encoder_case(name)
    stale, fresh, cap, fn, want = _cache[name, "case"]
    assert want[0] == 0 and len(stale) == len(fresh) and stale != fresh
    (rc, ol, crc), out, src = _behind_default(fn(encoder), stale, fresh, cap, a_in, name)
    assert (rc, out[:ol], crc) == tuple(want), "%s: the stream is not B's" % name
    assert src == fresh, "the input was written"


def _decoder_case(name):
    """-> (stale stream, fresh stream, cap, fn (enc) -> device call, (the data, input bytes used))"""
    import bz2
    import _inflate
    import _unlegacy as U
    import _unlzma
    text = silesia_mix(60000, class_mask=1)
    if name == "inflate":
        d = text[:5000]
        enc_ = lambda x: _inflate.zlib_raw(x, 9, zlib.Z_DEFAULT_STRATEGY)
        return S.stale_stream(enc_, len(enc_(d)), len(d)), enc_(d), len(d), lambda enc: enc.inflate_device, (d, len(enc_(d)))
    if name == "inflate_par, chunks of 4 KiB":
        _pair(1)
        d = _cache["mix"][:118000]
        enc_ = lambda x: _inflate.zlib_raw(x, 6, zlib.Z_DEFAULT_STRATEGY)
        p = enc_(d)
        assert 60 << 10 <= len(p) <= 68 << 10, len(p)
        return S.stale_stream(enc_, len(p), len(d)), p, len(d), lambda enc: enc.inflate_par_device, (d, len(p))
    if name == "bunzip2":
        d = text[20000:28000]
        enc_ = lambda x: bz2.compress(x, 9)
        return S.stale_stream(enc_, len(enc_(d)), len(d)), enc_(d), len(d), lambda enc: enc.bunzip2_device, (d, len(enc_(d)))
    if name == "unlzma":
        d = text[30000:35000]
        p = _unlzma.raw_payload(d)
        used = _unlzma.model_unlzma(p, len(d), True)[3]
        return S.stale_stream(_unlzma.raw_payload, len(p), len(d)), p, len(d), lambda enc: enc.unlzma_device, (d, used)
    if name == "unlegacy, PKZIP 1.10's Implode stream":
        row, p = next((r, s) for r, s in U.fixtures() if r["file"] == "many_formats_07_pk110.bin")
        m, f, n = row["format"], row["flags"], row["size"]
        stale = S.stale_stream(lambda x: U.implode(x, f), len(p), n)
        assert U.host_decode(m, f, stale, n)[0] == 0
        return stale, p, n, lambda enc: (lambda di, ni, do, cap: enc.unlegacy_device(di, ni, do, cap, m, f)), ((row["sha256"], int(row["crc32"], 16), n), len(p))
    raise KeyError(name)


DECODERS = ("inflate", "inflate_par, chunks of 4 KiB", "bunzip2", "unlzma", "unlegacy, PKZIP 1.10's Implode stream")


@pytest.mark.parametrize("a_in", ALIGN)
@pytest.mark.parametrize("name", DECODERS)
def test_decoders_on_pointers_behind_the_default_stream(encoder, name, a_in):
    if (name, "case") not in _cache:
        _cache[name, "case"] = _decoder_case(name)
    stale, fresh, cap, fn, (data, used) = _cache[name, "case"]
    assert len(stale) == len(fresh) and stale != fresh
    par = name.startswith("inflate_par")
    if par:
        encoder.set_knob("inflate_par_chunk_kib", 4)
    try:
        (ol, iu, reg), out, src = _behind_default(fn(encoder), stale, fresh, cap, a_in, name)
        last = encoder.inflate_par_last() if par else None
    finally:
        if par:
            encoder.set_knob("inflate_par_chunk_kib", 128)
    if isinstance(data, tuple):                               # the fixture's data are known by digest, CRC-32 and size
        assert (hashlib.sha256(out[:ol]).hexdigest(), reg ^ FF, ol, iu) == data + (used,), "%s: the bytes are not B's" % name
    else:
        assert (out[:ol], iu, reg) == (data, used, crc_reg(data)), "%s: the bytes are not B's" % name
    assert src == fresh, "the input was written"
    if par:
        assert last["fell_back"] == 0 and last["live_chunks"] >= 2, last


@pytest.mark.parametrize("a_in", ALIGN)
def test_crc32_on_a_pointer_behind_the_default_stream(encoder, a_in):
    """zada_crc32_device takes 16-byte aligned addresses only: its second alignment is five 16-byte words into the tensor."""
    a, b = _pair(100001, 4)
    raw, _, src = _behind_default(lambda di, n, do, cap: encoder.crc32_device(di, n), a, b, 16, 16 * a_in, "crc32_device")
    assert encoder.crc32_combine(FF, raw, len(b)) == crc_reg(b) and src == b


@pytest.mark.parametrize("a_in", ALIGN)
def test_compare_on_pointers_behind_the_default_stream(encoder, a_in):
    """the second buffer is pending: its stale content equals the first buffer, B differs from it in one byte"""
    import torch
    a, _ = _pair(50000, 5)
    at = 33333
    b = a[:at] + bytes([a[at] ^ 1]) + a[at + 1:]
    t_a = torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).cuda()
    first, _, src = _behind_default(lambda di, n, do, cap: encoder.compare_device(t_a.data_ptr(), di, n), a, b, 16, a_in, "compare_device")
    assert first == at and src == b


@pytest.mark.parametrize("a_in", ALIGN)
def test_find_on_a_pointer_behind_the_default_stream(encoder, a_in):
    import _findzip
    text = silesia_mix(40000, class_mask=1)
    needle = text[20000:20005]
    a, b = text[:18000] + text[22000:40000], text[4000:40000]
    wa, wb = _findzip.search_1_file(a, needle, True), _findzip.search_1_file(b, needle, True)
    assert len(a) == len(b) and wb[0] >= 1 and wa != wb
    got, _, src = _behind_default(lambda di, n, do, cap: encoder.find_device(di, n, needle), a, b, 16, a_in, "find_device")
    assert got == wb and src == b


@pytest.mark.parametrize("a_in", ALIGN)
def test_crypt_encode_on_a_pointer_behind_the_default_stream(encoder, a_in):
    """in place: the pending buffer is the output as well"""
    import _crypt
    a, b = _pair(30001, 6)
    k0 = _crypt.init_keys(PW)
    keys, _, src = _behind_default(lambda di, n, do, cap: encoder.crypt_encode_device(k0, di, n), a, b, 16, a_in, "crypt_encode_device")
    assert (src, keys) == _crypt.encode(k0, b)


@pytest.mark.parametrize("a_in", ALIGN)
def test_zip_device_on_pointers_behind_the_default_stream(encoder, a_in):
    """Encoder.zip_device on a table made by hand: the entries lie one behind the other in one pending tensor; the archive is the oracle's"""
    za = product()
    A, B = _lists()
    names = _names(B, "txt")
    if "zip want" not in _cache:
        _cache["zip want"] = oracle_zip(list(zip(names, B)), 8)
    want = _cache["zip want"]
    nms = [nm.encode() for nm in names]
    blob = np.frombuffer(b"".join(nms) + b"\0", dtype=np.uint8)

    def call(di, n, do, cap):
        tab = np.zeros(len(B), dtype=za.Encoder.zip_dtypes()[0])
        at = nat = 0
        for k, d in enumerate(B):
            tab[k] = (di + at if d else 0, len(d), blob.ctypes.data + nat, len(nms[k]), za.ZipCreate.DEFAULT_TIME, 1, 0)
            at += len(d)
            nat += len(nms[k])
        assert encoder.zip_bound(tab) <= cap
        return encoder.zip_device(tab, do, cap, 8)
    (alen, res), out, src = _behind_default(call, b"".join(A), b"".join(B), len(b"".join(B)) + len(want), a_in, "zip_device")
    assert out[:alen] == want and [int(r) for r in res["rc"]] == [0] * len(B) and src == b"".join(B)
    with zipfile.ZipFile(io.BytesIO(out[:alen])) as z:
        assert [z.read(i) for i in z.infolist()] == B


@pytest.mark.parametrize("a_in", ALIGN)
def test_unzip_device_on_pointers_behind_the_default_stream(encoder, a_in):
    """Encoder.unzip_device on a table made from tests/_orders.py's own reading of the archive"""
    from _orders import parse_zip
    za = product()
    stale, fresh, entries = _archives("deflate")
    rows, _ = parse_zip(fresh)
    slots = [(r["usize"] + 255) & ~255 for r in rows]
    offs = [sum(slots[:k]) for k in range(len(rows))]

    def call(di, n, do, cap):
        tab = np.zeros(len(rows), dtype=za.Encoder.unzip_dtypes()[0])
        for k, r in enumerate(rows):
            tab[k] = (r["data_offset"], r["csize"], offs[k], r["usize"], r["method"], 0, 0, 0)
        return encoder.unzip_device(di, n, do, cap, tab)
    (rc, res), out, src = _behind_default(call, stale, fresh, sum(slots), a_in, "unzip_device")
    assert rc == 0 and src == fresh
    for k, (r, (nm, d)) in enumerate(zip(rows, entries)):
        assert (int(res["rc"][k]), int(res["out_len"][k]), int(res["crc"][k]) ^ FF, out[offs[k]:offs[k] + len(d)]) == (0, len(d), zlib.crc32(d), d), nm
