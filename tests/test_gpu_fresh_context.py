"""Contexts with no history.

tests/conftest.py hands every test one session-wide Encoder whose workspaces only grow, so a call that books too little -- or that leans on what
an earlier call left behind -- is never seen by the rest of the suite.  Every call here runs on a context that was made for it (or, for the
orders, on one context made for that order), one context open at a time:

  * streams that go through one context span after span ("span_mib"), at the span sizes and guesses ("atoms_pct") where a span once asked
    for more atoms than the stream had booked (zada_sizing.h; tests/test_hostlogic.py checks the arithmetic exhaustively),
  * a fixed list of calls to every kind of entry point, alone and in four orders on one context: the bytes never depend on what ran before
    (the readers, the archive tools, the legacy coders and the trained handles each with one larger call: _later_families; every ordered pair
    of small calls is tests/test_gpu_call_orders.py's),
  * a stopped LZMA stream is exported right after its stop or not at all.

Expected bytes are the CPU oracles' and models' (oracle_deflate, tests/rich, _bzip2, _lzmah, _crypt, zlib; tests/_orders.py for the archives),
computed once per module."""
import zlib

import numpy as np
import pytest

import _crypt
import _rich
from _common import booked_atoms, oracle_deflate, oracle_tokens, product, silesia_mix

pytestmark = pytest.mark.gpu

MIB = 1 << 20
R = 11          # Method.Deflate_R: the model of tests/test_gpu_deflate_r.py


def crc_reg(d):
    return zlib.crc32(d) ^ 0xFFFFFFFF


def _zeros_heavy(n):
    """15/16 zeros (one atom per 258 bytes), 1/16 text per MiB: a span of 1 MiB has about 25 000 atoms, so a flush of 65 536 atoms fills
    every third span or so and the atoms carried over -- and the bytes they stand for, which stay resident -- reach across several spans."""
    text = silesia_mix(n // 16 + 65536, class_mask=1, version=2)
    out = bytearray(n)
    for k in range(n // MIB):
        out[k * MIB + 15 * 65536:(k + 1) * MIB] = text[k * 65536:(k + 1) * 65536]
    return bytes(out)


def _inputs():
    mix = silesia_mix(12 * MIB, version=2)
    rng = np.random.default_rng(99)
    return {
        "mix_8m_12345": mix[:8 * MIB + 12345],
        "mix_11m5": mix[:2 * 4 * MIB + 3 * MIB + MIB // 2],
        "mix_8m75": mix[:5 * MIB + 3 * MIB + 3 * MIB // 4],
        "mix_6m": mix[:6 * MIB],
        "mix_10m": mix[:8 * MIB + 2 * MIB],
        "zeros_heavy_8m": _zeros_heavy(8 * MIB),
        # a stretch of random bytes (one atom per byte) in the second span: that span has more atoms than the stream booked, so the arrays grow
        # while they hold the atoms carried over from the first.  (5 MiB of it, not 1: a stream in spans of 4 MiB and more books at least
        # 4 MiB of atoms, whatever "atoms_pct" says -- test_the_random_stretch_makes_the_arrays_grow asserts that this input is beyond it.)
        "mix_random_stretch": mix[:8 * MIB] + bytes(rng.integers(0, 256, 5 * MIB, dtype=np.uint8)) + mix[8 * MIB:9 * MIB],
    }


# (span_mib, atoms_pct, input)
SPAN_CASES = [
    (3, 50, "mix_8m_12345"),
    (4, 50, "mix_11m5"),
    (5, 50, "mix_8m75"),
    (2, 1, "mix_6m"),
    (8, 1, "mix_10m"),
    (1, 50, "zeros_heavy_8m"),
    (8, 1, "mix_random_stretch"),
]
SPAN_METHODS = (10, 7, R)


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


@pytest.fixture(scope="module")
def expected_streams(inputs):
    """(input, method) -> (rc, stream, CRC register), each computed once."""
    cache = {}

    def get(name, method):
        if (name, method) not in cache:
            d = inputs[name]
            if method == R:
                rc, s = _rich.deflate_r(d)
                cache[(name, method)] = (rc, s, crc_reg(d))
            else:
                cache[(name, method)] = oracle_deflate(d, method)
        return cache[(name, method)]
    return get


def _fresh(**knobs):
    enc = product().Encoder(0)
    for k, v in knobs.items():
        enc.set_knob(k, v)
    return enc


def _host(enc, d, method):
    out = bytearray(len(d) + 64)
    rc, ol, crc = enc.deflate_into(d, out, method)
    return rc, bytes(out[:ol]), crc


def _device(enc, d, method):
    import torch
    t_in = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    t_out = torch.zeros(len(d) + 4096, dtype=torch.uint8, device="cuda")
    rc, ol, crc = enc.deflate_device(t_in.data_ptr(), len(d), t_out.data_ptr(), len(d) + 4096, method)
    torch.cuda.synchronize()
    return rc, bytes(t_out[:ol].cpu().numpy()), crc


@pytest.mark.parametrize("span_mib,atoms_pct,name", SPAN_CASES)
def test_spans_on_a_context_with_no_history(inputs, expected_streams, span_mib, atoms_pct, name):
    """One stream, span after span, on a context that has booked nothing before: Deflate_3, Deflate_0 and Deflate_R through zada_deflate, and
    Deflate_3 through zada_deflate_device -- each on a context of its own -- give the oracle's (the model's) stream and CRC."""
    d = inputs[name]
    for method, run in [(m, _host) for m in SPAN_METHODS] + [(10, _device)]:
        want = expected_streams(name, method)
        enc = _fresh(span_mib=span_mib, atoms_pct=atoms_pct)
        try:
            got = run(enc, d, method)
        finally:
            enc.close()
        assert want[0] == 0 and got[0] == 0 and got[2] == want[2] == crc_reg(d), (method, run.__name__)
        assert got[1] == want[1], (method, run.__name__, len(got[1]), len(want[1]))


def test_the_random_stretch_makes_the_arrays_grow(inputs, expected_streams):
    """The precondition of the last span case, and its effect: the second span of `mix_random_stretch` has more atoms (counted from the oracle's
    tokens) than a fresh context books for spans of 8 MiB, so grow_atoms runs while the arrays hold the first span's carried atoms --
    #atoms_grown says so -- and the stream is still the oracle's."""
    d = inputs["mix_random_stretch"]
    span = 8 * MIB
    t = oracle_tokens(d, 10)
    lens = np.where(t & 0x80000000, (t >> 16) & 0x1FF, 1).astype(np.int64)
    start = np.concatenate(([0], np.cumsum(lens)[:-1]))
    per_span = np.bincount(start // span)
    booked = booked_atoms(span, 1)
    assert per_span[1] > booked and per_span[0] < booked and per_span[0] % 65536 != 0, (per_span, booked)
    enc = _fresh(span_mib=8, atoms_pct=1)
    try:
        got = _host(enc, d, 10)
        grown = dict(enc.last_timing()).get("#atoms_grown", 0)
    finally:
        enc.close()
    assert got == expected_streams("mix_random_stretch", 10)
    assert grown >= 1, grown


# ---- history independence across entry points ----

PASSWORD = b"fresh context"
HEADER11 = bytes(range(40, 51))


def _calls(inputs, expected_streams):
    """[(name, input bytes, run(enc) -> result, expected result)]: a fixed list of calls to every kind of entry point."""
    from _bzip2 import oracle_encode
    from _lzmah import oracle_lzma
    from test_gpu_lzma_variants import expected as lzma_expected
    rng = np.random.default_rng(2024)
    mix = silesia_mix(4 * MIB, version=2)
    text = silesia_mix(MIB, class_mask=1)
    calls = []

    def piece(lo, hi):
        n = int(rng.integers(lo, hi))
        o = int(rng.integers(0, len(mix) - n))
        return mix[o:o + n]

    def add(name, nbytes, run, want):
        calls.append((name, nbytes, run, want))

    def deflate_call(d, method):
        if method == R:
            rc, s = _rich.deflate_r(d)
            want = (rc, s if rc == 0 else None, crc_reg(d))
        else:
            rc, s, crc = oracle_deflate(d, method)
            want = (rc, s if rc == 0 else None, crc)

        def run(enc):
            rc2, out, crc2 = _host(enc, d, method)
            return rc2, out if rc2 == 0 else None, crc2
        add("deflate(%d bytes, method %d)" % (len(d), method), len(d), run, want)
    deflate_call(b"", 10)
    deflate_call(b"Z", 6)
    deflate_call(mix[5000:5000 + 70001], R)
    deflate_call(text[:70000], 6)
    deflate_call(mix[:3 * MIB], 10)

    datas = [piece(0, 20000) for _ in range(298)] + [b"", bytes(rng.integers(0, 256, 3000, dtype=np.uint8))]
    want = []
    for d in datas:
        rc, s, crc = oracle_deflate(d, 10)
        want.append((rc, s if rc == 0 else None, crc))
    add("deflate_batch(300 entries)", sum(map(len, datas)), lambda enc, datas=datas: enc.deflate_batch(datas, 10), want)

    d_span = inputs["mix_8m_12345"]

    def spanned(enc):
        enc.set_knob("span_mib", 3)
        try:
            return _host(enc, d_span, 10)
        finally:
            enc.set_knob("span_mib", 2048)
    add("deflate(8 MiB + 12345 in spans of 3 MiB)", len(d_span), spanned, expected_streams("mix_8m_12345", 10))

    d_bz = mix[MIB:3 * MIB]
    s, _ = oracle_encode(d_bz, 2)
    add("bzip2(2 MiB, method 14)", len(d_bz), lambda enc: enc.bzip2(d_bz, 14), (0, s, crc_reg(d_bz)))
    bz_datas = [piece(0, 120000) for _ in range(20)] + [b"", bytes(40000)]
    want = []
    for d in bz_datas:
        s, _ = oracle_encode(d, 2)
        want.append((1 if len(s) >= len(d) else 0, s, crc_reg(d)))
    add("bzip2_batch(22 entries)", sum(map(len, bz_datas)), lambda enc: enc.bzip2_batch(bz_datas, 14), want)

    d_lz = mix[300000:500000]
    add("lzma(200 KB, method 18)", len(d_lz), lambda enc: enc.lzma(d_lz, 18), oracle_lzma(d_lz, 18))
    lz_datas = [piece(0, 24000) for _ in range(30)] + [b""]
    add("lzma_batch(31 entries, method 16)", sum(map(len, lz_datas)), lambda enc: enc.lzma_batch(lz_datas, 16), [oracle_lzma(d, 16) for d in lz_datas])
    hbm_datas = [piece(1000, 12000) for _ in range(8)]          # method 19, LZMA_2_for_Zip_in_Zip: lc + lp = 12, the literal tables in HBM
    add("lzma_batch(8 entries, method 19)", sum(map(len, hbm_datas)), lambda enc: enc.lzma_batch(hbm_datas, 19), [lzma_expected(d, 19) for d in hbm_datas])

    d_pw = mix[2 * MIB:2 * MIB + 400000]
    add("compress_data(400 KB, password)", len(d_pw), lambda enc: enc.compress_data(d_pw, 10, password=PASSWORD, header=HEADER11),
        _crypt.compress_data_pw(d_pw, 10, PASSWORD, HEADER11)[:3])
    cr_datas = [piece(0, 50000) for _ in range(40)] + [b""]
    keys = [_crypt.init_keys(b"pw%d" % i) for i in range(len(cr_datas))]
    add("crypt_encode_batch(41 buffers)", sum(map(len, cr_datas)), lambda enc: enc.crypt_encode_batch(keys, cr_datas), [_crypt.encode(k, d) for k, d in zip(keys, cr_datas)])

    inf_datas = [piece(0, 30000) for _ in range(300)] + [b""]
    payloads = []
    for i, d in enumerate(inf_datas):
        c = zlib.compressobj(1 + i % 9, zlib.DEFLATED, -15)
        payloads.append(c.compress(d) + c.flush())
    add("inflate_batch(301 streams)", sum(map(len, inf_datas)), lambda enc: enc.inflate_batch(payloads, [len(d) for d in inf_datas], 8),
        [(0, d, len(d), len(p), crc_reg(d)) for d, p in zip(inf_datas, payloads)])
    d_inf = mix[3 * MIB:3 * MIB + 600000]
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    p_inf = c.compress(d_inf) + c.flush()
    add("inflate(600 KB)", len(d_inf), lambda enc: enc.inflate(p_inf, len(d_inf)), (d_inf, len(p_inf), crc_reg(d_inf)))
    _later_families(add, inputs, mix, text)
    return calls


def _later_families(add, inputs, mix, text):
    """One larger call per family that came after the list above, so that the four orders grow and shrink each family's own state objects (the readers',
    the archive writer's, ReZip's, Find_Zip's, the legacy coders', the trained handles').  Expected values as in tests/_orders.py: the CPU models', the
    oracle's, the standard library's."""
    import bz2
    import io
    import zipfile

    import _findzip
    import _legacy as L
    import _orders
    import _trained
    import _unlegacy as U
    import _unlzma
    from _inflate import zlib_raw
    from test_gpu_unlegacy import _mixed_entries
    za = product()

    ents = _mixed_entries()
    want = []
    for m, f, s, cap, d in ents:
        want.append((0, d, len(d), U.host_decode(m, f, s, cap)[3], crc_reg(d)))
    add("unlegacy_batch(%d entries)" % len(ents), sum(len(e[4]) for e in ents),
        lambda enc: enc.unlegacy_batch([e[2] for e in ents], [e[3] for e in ents], [e[0] for e in ents], [e[1] for e in ents]), want)

    d_bu = mix[:1200000]
    p_bu = bz2.compress(d_bu, 9)                               # level 9: blocks of 900 000 bytes, two of them
    add("bunzip2(1.2 MB, two level-9 blocks)", len(d_bu), lambda enc: enc.bunzip2(p_bu, len(d_bu)) + (len(enc.bunzip2_last_records(blocks=True)),),
        (d_bu, len(p_bu), crc_reg(d_bu), 2))
    d_ul = mix[MIB:2 * MIB]
    p_ul = _unlzma.raw_payload(d_ul, dict_size=MIB)
    add("unlzma(1 MiB)", len(d_ul), lambda enc: enc.unlzma(p_ul, len(d_ul)), (d_ul, len(p_ul), crc_reg(d_ul)))
    d_par = inputs["mix_10m"][:8 * MIB]
    p_par = zlib_raw(d_par, 6, zlib.Z_DEFAULT_STRATEGY)
    add("inflate_par(8 MiB)", len(d_par), lambda enc: enc.inflate_par(p_par, len(d_par)), (d_par, len(p_par), crc_reg(d_par)))

    half = MIB // 2
    z_entries = [("big/d%d.bin" % k, mix[k * half:(k + 1) * half]) for k in range(4)] + [("big/bz0.txt", text[:half]), ("big/bz1.bin", mix[2 * MIB:2 * MIB + half]),
                                                                                         ("big/stored.bin", mix[3 * MIB:3 * MIB + half]), ("big/lz.bin", mix[3 * MIB + half:3 * MIB + half + 200000])]
    z_methods = [zipfile.ZIP_DEFLATED] * 4 + [zipfile.ZIP_BZIP2] * 2 + [zipfile.ZIP_STORED, zipfile.ZIP_LZMA]
    bio = io.BytesIO()
    with zipfile.ZipFile(bio, "w") as zf:
        for (nm, d), m in zip(z_entries, z_methods):
            zf.writestr(zipfile.ZipInfo(nm, (2024, 5, 6, 7, 8, 10)), d, compress_type=m)
    z_arc = bio.getvalue()
    z_size = sum(len(d) for _, d in z_entries)

    def extract(enc):
        import torch
        t = torch.from_numpy(np.frombuffer(z_arc, dtype=np.uint8).copy()).cuda()
        got = za.UnZip(enc, bzip2=True, lzma=True).extract_device(za.ZipInfo.load_device(t))
        return {nm: v.cpu().numpy().tobytes() for nm, v in got.items()}
    add("extract_device(archive of 3.7 MiB)", z_size, extract, dict(z_entries))

    w_entries = [("w/e%d.bin" % k, mix[k * half + 777:(k + 1) * half + 777]) for k in range(8)]          # (the last one ends with the corpus: 777 bytes shorter)

    def write(enc):
        import torch
        tensors = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for _, d in w_entries]
        return za.ZipCreate(enc, 10).write_device_ex([nm for nm, _ in w_entries], tensors).cpu().numpy().tobytes()
    add("write_device_ex(4 MiB, Deflate_3)", sum(len(d) for _, d in w_entries), write, _orders.cpu_archive(w_entries, 10))

    # ReZip with {original, deflate_3, bzip2_3}: a single LZMA_3 stream of half a megabyte runs on one wave for seconds (test_gpu_rezip_device.py
    # leaves the LZMA approaches out of its large entry for the same reason)
    mask = (1 << 0) | (1 << 5) | (1 << 7)
    want = _orders.rezip_model(z_arc, {nm.encode(): d for nm, d in z_entries}, mask)

    def rezip(enc):
        import torch
        t = torch.from_numpy(np.frombuffer(z_arc, dtype=np.uint8).copy()).cuda()
        arc, rep = za.ReZip(enc).rezip_device(za.ZipInfo.load_device(t), approaches=mask, report=True)
        return arc.cpu().numpy().tobytes(), rep["entries"]
    add("rezip_device(archive of 3.7 MiB)", z_size + 1, rezip, want)

    needle = text[100000:100005]
    found = []
    for nm, d in sorted((nm.encode(), d) for nm, d in z_entries):
        occ, first = _findzip.closed_form(d, needle, True)
        if occ:
            found.append((nm, occ, first))
    assert found

    def findzip(enc):
        r = za.FindZip(enc).find(z_arc, needle)
        return [(e[4], e[1], e[2]) for e in r.entries if e[1] > 0], r.damaged
    add("findzip(archive of 3.7 MiB)", z_size + 2, findzip, (found, 0))

    lg_datas = L.batch_inputs(100)
    for method, name in ((1, "shrink_batch"), (5, "reduce_batch")):
        want = [(rc, s if rc == 0 else None, reg) for rc, s, reg in (L.model_result(d, method) for d in lg_datas)]
        add("%s(100 entries)" % name, sum(map(len, lg_datas)) + method,
            (lambda enc: enc.shrink_batch(lg_datas)) if method == 1 else (lambda enc: enc.reduce_batch(lg_datas, 5)), want)

    trainer = _trained.fixture("wsbase.csv")[:9000]
    src = _trained.fixture("wm1ns.csv")
    tr_datas = [src[37 * k:37 * k + (k * 7) % 300] for k in range(200)]
    stub = _trained.stub_of(trainer)
    skip = max(0, len(stub) - _trained.MARGIN)
    msgs = [_trained.message_of(trainer, d, skip) for d in tr_datas]

    def trained(enc):
        tc = td = None
        try:
            tc = za.TrainedCompression(enc, trainer)
            got = tc.encode(tr_datas)
            td = za.TrainedCompression.for_decoding(enc, tc.stub, tc.skip, tc.trainer_len)
            return tc.stub, got, td.decode(msgs, [len(d) for d in tr_datas])
        finally:
            for h in (tc, td):
                if h is not None:
                    h.close()
    add("trained(200 messages)", sum(map(len, tr_datas)), trained, (stub, msgs, tr_datas))


@pytest.fixture(scope="module")
def calls(inputs, expected_streams):
    return _calls(inputs, expected_streams)


def _differs(got, want):
    """None, or where the two results part (a batch: its first differing entry)."""
    if got == want:
        return None
    if isinstance(got, list) and isinstance(want, list) and len(got) == len(want):
        k = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        return "entry %d of %d" % (k, len(got))
    return "the result"


def test_every_call_alone_on_a_fresh_context(calls):
    for name, _, run, want in calls:
        enc = _fresh()
        try:
            got = run(enc)
        finally:
            enc.close()
        assert _differs(got, want) is None, (name, _differs(got, want))


def _orders(calls):
    idx = list(range(len(calls)))
    asc = sorted(idx, key=lambda i: calls[i][1])
    yield "ascending input size", asc
    yield "descending input size", asc[::-1]
    for seed in (1, 2):
        yield "shuffle %d" % seed, [int(i) for i in np.random.default_rng(seed).permutation(len(calls))]


@pytest.mark.parametrize("which", range(4))
def test_a_call_s_bytes_do_not_depend_on_the_calls_before(calls, which):
    """The whole list on ONE fresh context, in four orders: by input size upwards (every call books anew) and downwards (every call runs in
    workspaces larger than it needs, with the last call's bytes in them), and two seeded shuffles."""
    order_name, order = list(_orders(calls))[which]
    enc = _fresh()
    try:
        before = "nothing"
        for i in order:
            name, _, run, want = calls[i]
            got = run(enc)
            assert _differs(got, want) is None, "order %r: %s differs in %s, the call before was %s" % (order_name, name, _differs(got, want), before)
            before = name
    finally:
        enc.close()


# ---- the stopped LZMA stream ----

@pytest.mark.parametrize("between", ("deflate", "lzma_device"))
def test_a_stopped_lzma_stream_is_exported_at_once_or_not_at_all(between):
    """zada_lzma_export_state hands out the coder's state and the stream so far from buffers that any other call may fill or move.  After a
    stream stopped by its feedback, a zada_deflate -- or a zada_lzma_device of the same length, which leaves the same `n` in the saved state --
    on the same context, and the export is refused (ZADA_E_INVALID); right after the stop it is given, and the context goes on working."""
    import torch
    from _lzmah import oracle_lzma
    Z = product()
    d = silesia_mix(300000, version=2)
    other = silesia_mix(300000, seed=4321, version=2)
    enc = _fresh(lzma_chunk=20000)
    try:
        with pytest.raises(Z.UserAbort):
            enc.lzma(d, 18, feedback=lambda pct: pct >= 40)
        state, head, pos = enc.lzma_export_state(len(d) + 4096)           # at once: given (and asking twice changes nothing)
        assert 0 < pos < len(d) and enc.lzma_export_state(len(d) + 4096) == (state, head, pos)
        assert oracle_lzma(d, 18)[1].startswith(head)
        if between == "deflate":
            rc, s, crc = oracle_deflate(other, 10)
            assert _host(enc, other, 10) == (rc, s, crc)
        else:
            t_in = torch.frombuffer(bytearray(other), dtype=torch.uint8).cuda()
            t_out = torch.zeros(len(other) + 4096, dtype=torch.uint8, device="cuda")
            rc, ol, crc = enc.lzma_device(t_in.data_ptr(), len(other), t_out.data_ptr(), len(other) + 4096, 18)
            torch.cuda.synchronize()
            assert (rc, bytes(t_out[:ol].cpu().numpy()), crc) == oracle_lzma(other, 18)
        with pytest.raises(Z.ZadaError, match="zada_lzma_export_state"):
            enc.lzma_export_state(len(d) + 4096)
        # a stop BEFORE the first launch leaves no state of this stream either, whatever an earlier stream left in the buffer
        with pytest.raises(Z.UserAbort):
            enc.lzma(d, 18, feedback=lambda pct: True)
        with pytest.raises(Z.ZadaError, match="zada_lzma_export_state"):
            enc.lzma_export_state(len(d) + 4096)
        assert enc.lzma(d, 18) == oracle_lzma(d, 18)
    finally:
        enc.close()
