"""The node list of the call-order tests (test_gpu_call_orders.py, test_call_orders_plan.py): one small call per kind of entry point, each with the
result a CPU reference gives for it, and the sequence that visits every ordered pair of them.

A node is (name, run (enc) -> result, want).  `want` never comes from the product: it is the oracle's, a CPU model's or the standard library's
(oracle_deflate, tests/rich, _bzip2, _lzmah, _crypt, tests/legacy, _unlegacy.host_decode, _bunzip2, _unlzma, _inflate, _inflate_par, oracle_zip*,
_rezip / _rezip_legacy, _findzip, _trained, zlib, bz2, lzma, zipfile), so building the list needs no GPU.  A result holds the "last call" records
of its family where there are any -- they are context state, and can be stale.  Archives are parsed for the models by parse_zip below, not by the
product's ZipInfo.

COVERS names, per node, the entry points it reaches (Python methods as Class.method, C functions by name); EXEMPT the entry points without a
node, each with its reason.  tests/test_call_orders_plan.py holds that the two together are the whole public surface."""
import io
import struct
import zipfile
import zlib

import numpy as np

import _crypt
import _legacy as L
import _rezip
import _rezip_legacy as RL
import _rich
import _unlegacy as U
from _common import oracle_deflate, oracle_zip, oracle_zip_compressed, product, silesia_mix

FF = 0xFFFFFFFF
R = 11                                                     # Method.Deflate_R
PW, WRONG_PW = b"orders pw", b"not the password"
SEGMENT = 150                                              # calls per segment of the pair walk


def crc_reg(d):
    return zlib.crc32(d) ^ FF


def h11(k):
    """eleven fixed 'random' bytes"""
    return np.random.default_rng(700 + k).integers(0, 256, 11, dtype=np.uint8).tobytes()


# ---- the sequence -------------------------------------------------------------------------------------------------------------------------------
def sequence(k):
    """k * k + 1 node numbers in which every ordered pair (a, b), (a, a) included, is a pair of neighbours exactly once: for i ascending, i, then
    i, j for every j > i; node 0 closes the cycle."""
    seq = []
    for i in range(k):
        seq.append(i)
        for j in range(i + 1, k):
            seq += [i, j]
    return seq + [0]


def segments(seq, size=SEGMENT):
    """Consecutive pieces of about `size` calls; each begins with the last node of the piece before, so that no pair of neighbours is lost."""
    out, at = [], 0
    while at < len(seq) - 1:
        out.append(seq[at:at + size])
        at += size - 1
    return out


# ---- entry points: who reaches them, who needs no node ------------------------------------------------------------------------------------------
COVERS = {
    "deflate(70001, Deflate_Fixed)": ("Encoder.deflate", "zada_deflate"),
    "deflate(70001, Deflate_3)": ("Encoder.deflate_into", "zada_deflate", "Encoder.last_blocks", "zada_last_blocks"),
    "deflate(70001, Deflate_R)": ("Encoder.deflate_into", "zada_deflate"),
    "deflate(empty, Deflate_Fixed)": ("Encoder.deflate_into", "zada_deflate"),
    "deflate(empty, Deflate_3)": ("Encoder.deflate_into", "zada_deflate"),
    "deflate(empty, Deflate_R)": ("Encoder.deflate_into", "zada_deflate"),
    "deflate_batch(20)": ("Encoder.deflate_batch", "zada_deflate_batch"),
    "deflate_device(50000)": ("Encoder.deflate_device", "zada_deflate_device"),
    "bzip2(120000, BZip2_3)": ("Encoder.bzip2", "zada_bzip2", "Encoder.bz2_last_blocks", "zada_bz2_last_blocks"),
    "bzip2_batch(6)": ("Encoder.bzip2_batch", "zada_bzip2_batch"),
    "bzip2_device(30000)": ("Encoder.bzip2_device", "zada_bzip2_device"),
    "lzma(3000, LZMA_3)": ("Encoder.lzma", "zada_lzma"),
    "lzma_batch(8, LZMA_1)": ("Encoder.lzma_batch", "zada_lzma_batch"),
    "lzma_batch(2, LZMA_2_for_Zip_in_Zip)": ("Encoder.lzma_batch", "zada_lzma_batch"),
    "lzma_device(2000, LZMA_1)": ("Encoder.lzma_device", "zada_lzma_device"),
    "lzma stopped, exported, imported, resumed": ("Encoder.lzma", "Encoder.lzma_export_state", "Encoder.lzma_import_state", "zada_lzma", "zada_lzma_export_state",
                                                  "zada_lzma_import_state"),
    "shrink(5000)": ("Encoder.shrink", "zada_shrink"),
    "shrink_batch(8)": ("Encoder.shrink_batch", "zada_shrink_batch"),
    "reduce_batch(7, Reduce_4)": ("Encoder.reduce_batch", "zada_reduce_batch", "Encoder.reduce_last_record", "zada_reduce_last_record"),
    "reduce_batch(7, Reduce_1)": ("Encoder.reduce_batch", "zada_reduce_batch", "Encoder.reduce_last_record", "zada_reduce_last_record"),
    "reduce(1000), shrink_device, reduce_device": ("Encoder.reduce", "zada_reduce", "Encoder.shrink_device", "zada_shrink_device", "Encoder.reduce_device",
                                                   "zada_reduce_device"),
    "compress_data(40000, Deflate_3, password)": ("Encoder.compress_data", "zada_compress_data_pw"),
    "compress_data(8000, Preselection_2)": ("Encoder.compress_data", "zada_compress_data_hint", "zada_compress_data"),
    "crypt_encode_batch(10)": ("Encoder.crypt_encode_batch", "zada_crypt_encode_batch"),
    "crypt_encode, crypt_encode_device, crypt_decode_batch": ("Encoder.crypt_encode", "zada_crypt_encode", "Encoder.crypt_encode_device", "zada_crypt_encode_device",
                                                              "Encoder.crypt_decode_batch", "zada_crypt_decode_batch"),
    "crc32_device(100001)": ("Encoder.crc32_device", "zada_crc32_device"),
    "trained(8 messages)": ("TrainedCompression.encode", "TrainedCompression.encode_device", "TrainedCompression.encode_raw", "TrainedCompression.decode",
                            "TrainedCompression.decode_device", "TrainedCompression.decode_raw", "TrainedCompression.for_decoding", "zada_trained_stub",
                            "zada_trained_open_encoder", "zada_trained_open_decoder", "zada_trained_encode_device", "zada_trained_decode_device"),
    "inflate(60000)": ("Encoder.inflate", "zada_inflate"),
    "inflate_batch(30)": ("Encoder.inflate_batch", "zada_inflate_batch"),
    "inflate_device(60000)": ("Encoder.inflate_device", "zada_inflate_device"),
    "inflate_par(chunks of 4 KiB)": ("Encoder.inflate_par", "zada_inflate_par", "Encoder.inflate_par_last", "zada_inflate_par_last"),
    "inflate_par_device(chunks of 4 KiB)": ("Encoder.inflate_par_device", "zada_inflate_par_device", "Encoder.inflate_par_last", "zada_inflate_par_last"),
    "bunzip2(two blocks)": ("Encoder.bunzip2", "zada_bunzip2", "Encoder.bunzip2_last_records", "zada_bunzip2_last_records"),
    "bunzip2_batch(6)": ("Encoder.bunzip2_batch", "zada_bunzip2_batch", "Encoder.bunzip2_last_records", "zada_bunzip2_last_records"),
    "bunzip2_device(40000)": ("Encoder.bunzip2_device", "zada_bunzip2_device"),
    "unlzma(20000)": ("Encoder.unlzma", "zada_unlzma", "Encoder.unlzma_last_records", "zada_unlzma_last_records"),
    "unlzma_batch(8)": ("Encoder.unlzma_batch", "zada_unlzma_batch", "Encoder.unlzma_last_records", "zada_unlzma_last_records"),
    "unlzma_device(20000)": ("Encoder.unlzma_device", "zada_unlzma_device"),
    "unlegacy_batch(18)": ("Encoder.unlegacy_batch", "zada_unlegacy_batch", "Encoder.unlegacy_last_records", "zada_unlegacy_last_records"),
    "unlegacy, unlegacy_device": ("Encoder.unlegacy", "zada_unlegacy", "Encoder.unlegacy_device", "zada_unlegacy_device"),
    "extract_device(zipfile, 8 entries)": ("UnZip.extract_device", "Encoder.unzip_device", "zada_unzip_device"),
    "extract_device(encrypted)": ("UnZip.extract_device", "Encoder.unzip_device", "zada_unzip_device"),
    "extract_device(wrong password)": ("UnZip.extract_device", "Encoder.unzip_device", "zada_unzip_device"),
    "extract_device(legacy, methods 1 .. 6)": ("UnZip.extract_device", "Encoder.unzip_device", "zada_unzip_device"),
    "extract(encrypted, host bytes)": ("UnZip.extract", "Encoder.crypt_decode_batch", "zada_crypt_decode_batch", "Encoder.inflate_batch", "Encoder.bunzip2_batch",
                                       "Encoder.unlzma_batch"),
    "write_device(6, Deflate_3)": ("ZipCreate.write_device", "Encoder.zip_device", "zada_zip_device"),
    "write_device_ex(BZip2_3, password)": ("ZipCreate.write_device_ex", "Encoder.zip_device_ex", "zada_zip_device_ex"),
    "write_device_ex(LZMA_3)": ("ZipCreate.write_device_ex", "Encoder.zip_device_ex", "zada_zip_device_ex"),
    "write_device_ex(legacy, Shrink_1)": ("ZipCreate.write_device_ex", "Encoder.zip_device_ex", "zada_zip_device_ex"),
    "write_device_ex(legacy, Reduce_4)": ("ZipCreate.write_device_ex", "Encoder.zip_device_ex", "zada_zip_device_ex"),
    "add_stream, add_streams(password), finish": ("ZipCreate.add_stream", "ZipCreate.add_streams", "ZipCreate.add_compressed", "ZipCreate.finish", "Encoder.compress_data",
                                                  "Encoder.deflate_batch", "Encoder.crypt_encode_batch"),
    "rezip_device(6 entries)": ("ReZip.rezip_device", "Encoder.rezip_device", "zada_rezip_device"),
    "rezip(legacy, methods 1 .. 6)": ("ReZip.rezip", "ReZip.rezip_device", "Encoder.rezip_device", "zada_rezip_device"),
    "compare_device(two archives)": ("CompZip.compare_device", "Encoder.compzip_device", "zada_compzip_device"),
    "Encoder.compare_device(50000)": ("Encoder.compare_device", "zada_compare_device"),
    "find_device(5 bytes)": ("Encoder.find_device", "zada_find_device"),
    "find_device(17 bytes)": ("Encoder.find_device", "zada_find_device"),
    "FindZip.find(8 entries)": ("FindZip.find", "FindZip.find_device", "Encoder.findzip_device", "zada_findzip_device"),
    "refused: shrink_device, cap one short": ("Encoder.shrink_device", "zada_shrink_device"),
    "refused: unlegacy_device, cap one short": ("Encoder.unlegacy_device", "zada_unlegacy_device"),
    "stopped: lzma (UserAbort)": ("Encoder.lzma", "zada_lzma", "Encoder.lzma_export_state", "zada_lzma_export_state"),
    "refused: bzip2, cap too small": ("Encoder.bzip2", "zada_bzip2"),
    "refused: rezip_device, legacy source without the knob": ("Encoder.rezip_device", "zada_rezip_device"),
    "refused: write_device asked for Shrink_1": ("ZipCreate.write_device", "Encoder.zip_device", "zada_zip_device"),
    "refused: unlegacy_device, method 9": ("Encoder.unlegacy_device", "zada_unlegacy_device"),
}

_GETTER = "a getter: copies what the last call left on the host, launches nothing"
_HOST = "host arithmetic only, launches nothing"
_HOOK = "a test / stage hook, run on contexts of their own by the tests of its stage"
_RANGE = ("a three-range call does not fit the shape budget (ranges are cut at multiples of 64 KiB and hand 32 KiB + 1 MiB of context on); "
          "tests/test_ranges.py and tests/test_multigpu.py run them on contexts of their own")
_BZ_RANGE = ("a three-range call does not fit the shape budget (a range is at least one BZip2 block of 100 000 .. 900 000 bytes); test_gpu_bzip2.py runs "
             "them on contexts of their own")
EXEMPT = {
    "Encoder.close": "ends the context", "zada_destroy": "ends the context", "zada_create": "makes the context (every test's first call)",
    "Encoder.set_knob": "sets a number in the context, launches nothing", "zada_set_knob": "sets a number in the context, launches nothing",
    "zada_last_error": _GETTER, "zada_version": _HOST,
    "Encoder.last_trace": _GETTER, "zada_last_trace": _GETTER, "Encoder.last_timing": _GETTER, "zada_last_timing": _GETTER,
    "Encoder.unzip_dtypes": "a dtype", "Encoder.zip_dtypes": "a dtype", "Encoder.rezip_dtypes": "a dtype", "Encoder.compzip_dtype": "a dtype",
    "Encoder.findzip_dtype": "a dtype",
    "Encoder.zip_bound": "a bound: " + _HOST, "zada_zip_bound": "a bound: " + _HOST, "Encoder.zip_bound_ex": "a bound: " + _HOST, "zada_zip_bound_ex": "a bound: " + _HOST,
    "Encoder.rezip_bound": "a bound: " + _HOST, "zada_rezip_bound": "a bound: " + _HOST,
    "Encoder.crc32_combine": _HOST, "zada_crc32_combine": _HOST, "Encoder.bz2_select": _HOST, "zada_bz2_select": _HOST,
    "Encoder.crypt_init_keys": _HOST, "zada_crypt_init_keys": _HOST, "Encoder.crypt_header": _HOST, "zada_crypt_header": _HOST,
    "zada_guess_type_from_name": _HOST, "zada_preselect": _HOST, "zada_lzma_lit_table_bytes": _HOST,
    "zada_silesia_mix": "the corpus generator: " + _HOST,
    "TrainedCompression.close": "frees a handle", "zada_trained_close": "frees a handle", "TrainedCompression.info": _GETTER, "zada_trained_info": _GETTER,
    "Encoder.lz77_tokens": _HOOK, "zada_lz77_tokens": _HOOK, "Encoder.lzma_match_sets": _HOOK, "zada_lzma_match_sets": _HOOK,
    "zada_bz2_run": _HOOK, "zada_bz2_fetch": _HOOK, "zada_test_llhc": _HOOK, "zada_test_radix_sort": _HOOK, "zada_test_scan": _HOOK,
    "Encoder.range_open": _RANGE, "Encoder.range_lz": _RANGE, "Encoder.range_edges": _RANGE, "Encoder.range_place": _RANGE, "Encoder.range_analyze": _RANGE,
    "Encoder.range_choose": _RANGE, "Encoder.range_emit": _RANGE,
    "zada_range_open": _RANGE, "zada_range_lz": _RANGE, "zada_range_edges": _RANGE, "zada_range_place": _RANGE, "zada_range_analyze": _RANGE,
    "zada_range_choose": _RANGE, "zada_range_emit": _RANGE,
    "Encoder.bz2_range_open": _BZ_RANGE, "Encoder.bz2_range_encode": _BZ_RANGE, "Encoder.bz2_range_table": _BZ_RANGE, "Encoder.bz2_range_assemble": _BZ_RANGE,
    "zada_bz2_range_open": _BZ_RANGE, "zada_bz2_range_encode": _BZ_RANGE, "zada_bz2_range_table": _BZ_RANGE, "zada_bz2_range_assemble": _BZ_RANGE,
}
# exempt although they launch kernels: only these kinds (the plan test holds every other reason to "launches nothing")
EXEMPT_THOUGH_LAUNCHING = {k for k, v in EXEMPT.items() if v in (_HOOK, _RANGE, _BZ_RANGE)}


# ---- CPU references shared by several nodes -----------------------------------------------------------------------------------------------------
def cpu_stream(d, method):
    """(zip type, payload) of Compress_Data without a password, Store fallback applied: methods 0 .. 33 by the oracles, 1 .. 5 by tests/legacy."""
    d = bytes(d)
    if 1 <= method <= 5:
        rc, s, _ = L.model_result(d, method)
        return (method, s) if rc == 0 else (0, d)
    rc, s = _crypt.plain_payload(d, method)
    return (_crypt.zip_type(method), s) if rc == 0 else (0, d)


def with_password(plain, payloads):
    """The archive `plain` (no Zip_64 records) with every entry's payload replaced and Encryption_Flag_Bit set: flag, sizes, offsets and payloads
    change, nothing else does (as tests/test_gpu_crypt.py states it)."""
    zf = zipfile.ZipFile(io.BytesIO(plain))
    infos = zf.infolist()
    out, cd, offs = bytearray(), bytearray(), []
    for info, payload in zip(infos, payloads):
        o = info.header_offset
        nl, el = struct.unpack_from("<HH", plain, o + 26)
        assert el == 0
        hdr = bytearray(plain[o:o + 30 + nl])
        flag, = struct.unpack_from("<H", hdr, 6)
        struct.pack_into("<H", hdr, 6, flag | 1)
        struct.pack_into("<I", hdr, 18, len(payload))
        offs.append(len(out))
        out += hdr + payload
    p = zf.start_dir
    for info, payload, off in zip(infos, payloads, offs):
        nl, el, cl = struct.unpack_from("<HHH", plain, p + 28)
        rec = bytearray(plain[p:p + 46 + nl + el + cl])
        flag, = struct.unpack_from("<H", rec, 8)
        struct.pack_into("<H", rec, 8, flag | 1)
        struct.pack_into("<I", rec, 20, len(payload))
        struct.pack_into("<I", rec, 42, off)
        cd += rec
        p += len(rec)
    end = bytearray(plain[p:])
    assert end[:4] == b"PK\x05\x06"
    struct.pack_into("<I", end, 16, len(out))
    return bytes(out + cd + end)


def cpu_archive(entries, method, password=None, headers=None):
    """The archive Zip.Create writes for [(name, bytes)] under one method: the oracle's writer around the CPU references' payloads."""
    rows = []
    for nm, d in entries:
        zt, s = cpu_stream(d, method)
        rows.append((nm, s, zlib.crc32(d), len(d), zt))
    plain = oracle_zip_compressed(rows)
    if password is None:
        return plain
    return with_password(plain, [_crypt.compress_data_pw(d, method, password, h)[0] for (_, d), h in zip(entries, headers)])


def parse_zip(arc):
    """The central directory and the local headers of an archive without Zip64 records, in directory order, as dicts (what the models of ReZip need)."""
    arc = bytes(arc)
    end = arc.rfind(b"PK\x05\x06")
    n, cd_size, cd_off, clen = struct.unpack_from("<HIIH", arc, end + 10)
    out, p = [], cd_off
    for _ in range(n):
        (_, _, _, flags, method, dos_time, crc, csize, usize, nlen, xlen, clen2, _, _, _, off) = struct.unpack_from("<4sHHHHIIIIHHHHHII", arc, p)
        raw = arc[p + 46:p + 46 + nlen]
        lver, lflags, _, ltime = struct.unpack_from("<HHHI", arc, off + 4)
        lnl, lxl = struct.unpack_from("<HH", arc, off + 26)
        data_offset = off + 30 + lnl + lxl
        out.append(dict(raw_name=raw, key=raw.replace(b"\\", b"/"), method=method, flags=flags, crc=crc, csize=csize, usize=usize, version=lver, local_flags=lflags,
                        time=ltime, data_offset=data_offset, payload=arc[data_offset:data_offset + csize]))
        p += 46 + nlen + xlen + clen2
    return out, arc[end + 22:end + 22 + clen]


def rezip_model(arc, plain, approaches, formats=RL.ALL_FORMATS):
    """What ReZip writes for the source `arc` whose entries hold `plain` [key]: tests/_rezip_legacy.py's approach loop and header model around the CPU
    references' streams (entry names without an extension: the content hint of the Preselection methods is neutral).
    -> (archive bytes, [(name, {approach: size}, choice)])"""
    from test_preselect import expected_preselect
    ents, comment = parse_zip(arc)
    order = sorted(ents, key=lambda e: e["key"])
    consider0 = RL.consider_a_priori(approaches, formats)
    rows, report = [], []
    for e in order:
        if e["key"][-1:] == b"/":
            continue
        d = plain[e["key"]]
        consider = RL.consider_entry(consider0, e["usize"])
        size, stream = [0] * 12, [None] * 12
        size[0], stream[0] = e["csize"], (e["method"], e["payload"], e["method"] == 14 and bool(e["local_flags"] & 2))
        for a in range(1, 12):
            if consider[a]:
                m = RL.METHOD[a] if RL.METHOD[a] < 34 else expected_preselect(RL.METHOD[a], 0, 1, len(d))
                zt, s = cpu_stream(d, m)
                size[a], stream[a] = len(s), (zt, s, zt == 14)
        choice = RL.try_all_approaches(consider, size, RL.format_choice(formats, e["method"]))
        zt, s, eos = stream[choice]
        rows.append(dict(name=e["key"], version=e["version"], flags=e["local_flags"], time=e["time"], crc=e["crc"], usize=e["usize"], method=e["method"],
                         kept=choice == 0, csize=len(s), zip_type=zt, eos=eos, payload=s))
        report.append((e["key"], {RL.APPROACHES[a]: size[a] for a in range(12) if consider[a]}, RL.APPROACHES[choice]))
    body, tail, _, _ = RL.rezip_archive(rows, 0, comment)
    return body + tail, report


# ---- what the runs share ------------------------------------------------------------------------------------------------------------------------
def _dev(b):
    import torch
    b = bytes(b)
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() if b else torch.empty(0, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _device_call(fn, data, cap):
    """fn (d_in, n, d_out, cap) on fresh tensors -> (what fn returns, the cap output bytes)"""
    import torch
    t_in = _dev(data if len(data) else b"\0")
    t_out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = fn(t_in.data_ptr(), len(data), t_out.data_ptr(), cap)
    torch.cuda.synchronize()
    return r, _bytes(t_out)[:cap]


def _blocks(enc):
    return [tuple(int(x) for x in row) for row in enc.last_blocks()]


def _refusal(fn, *texts):
    """(the exception's class, the texts its message must hold -- a text it does not hold is replaced by the message itself)"""
    try:
        fn()
    except Exception as e:                                 # noqa: BLE001 (the class is the result)
        return (type(e).__name__,) + tuple(t if t in str(e) else str(e) for t in texts)
    return ("no exception",) + texts


def _decoded(rows):
    """the batch decoders' rows as the models give them: (rc, bytes or None, bytes written, input bytes used, CRC register -- of a refused entry the
    register as it was, as include/zada.h promises)"""
    return [(rc, out if rc == 0 else None, ol, used, reg if rc == 0 else FF) for rc, out, ol, used, reg in rows]


def damaged(stream, refused):
    """`stream` with one byte near its middle changed so that the CPU model refuses it (refused (bytes) -> bool): a flipped bit alone may leave a
    valid stream."""
    for at in range(len(stream) // 2, len(stream)):
        for x in (0xFF, 0x55, 0x01):
            s = stream[:at] + bytes([stream[at] ^ x]) + stream[at + 1:]
            if refused(s):
                return s
    raise AssertionError("no damage the model refuses")


def _extracted(res):
    return {nm: (_bytes(v) if hasattr(v, "cpu") else v if isinstance(v, (bytes, type(None))) else (type(v).__name__, str(v))) for nm, v in res.items()}


_nodes = []


def nodes():
    """[(name, run, want)], built once."""
    if not _nodes:
        _build(_nodes)
        assert [n[0] for n in _nodes] == list(COVERS), "COVERS names other nodes than the list holds, or in another order"
    return _nodes


def _build(out):
    from _bzip2 import oracle_encode
    from _lzmah import oracle_lzma
    from test_gpu_lzma_variants import expected as lzma_expected
    from test_preselect import expected_preselect
    import _bunzip2
    import _findzip
    import _inflate
    import _inflate_par
    import _trained
    import _unlzma
    import bz2

    rng = np.random.default_rng(4242)
    mix = silesia_mix(1 << 20, version=2)
    text = silesia_mix(300000, class_mask=1)
    names = iter(COVERS)

    def add(run, want):
        out.append((next(names), run, want))

    def piece(lo, hi):
        n = int(rng.integers(lo, hi))
        o = int(rng.integers(0, len(mix) - n))
        return mix[o:o + n]

    # ---- encoders ----
    def deflate_node(d, method, through):
        blocks = []
        if method == R:
            rc, s = _rich.deflate_r(d, blocks=blocks)
            crc = crc_reg(d)
        else:
            rc, s, crc = oracle_deflate(d, method, blocks)
        # (a stream that is not smaller than its input: the reference stops early, its block trace is a prefix of the device's -- left out;
        # and Deflate_Fixed has no block chooser: the reference traces nothing for it.)
        traced = rc == 0 and method != 6
        want = (rc, s if rc == 0 else None, crc, blocks if traced else None)

        def run(enc):
            if through == "deflate":
                s2, crc2 = enc.deflate(d, method)
                return 0, s2, crc2, _blocks(enc) if traced else None
            buf = bytearray(len(d) + 64)
            rc2, ol, crc2 = enc.deflate_into(d, buf, method)
            return rc2, bytes(buf[:ol]) if rc2 == 0 else None, crc2, _blocks(enc) if traced else None
        add(run, want)
    d70 = mix[5000:5000 + 70001]
    deflate_node(d70, 6, "deflate")
    deflate_node(d70, 10, "into")
    deflate_node(d70, R, "into")
    for m in (6, 10, R):
        deflate_node(b"", m, "into")

    datas = [piece(0, 20000) for _ in range(18)] + [b"", bytes(rng.integers(0, 256, 3000, dtype=np.uint8))]
    want = []
    for d in datas:
        rc, s, crc = oracle_deflate(d, 10)
        want.append((rc, s if rc == 0 else None, crc))
    add(lambda enc, datas=datas: enc.deflate_batch(datas, 10), want)

    d50 = mix[100000:150000]
    blocks = []
    rc, s, crc = oracle_deflate(d50, 10, blocks)
    assert rc == 0

    def run(enc):
        (rc2, ol, crc2), buf = _device_call(lambda di, n, do, cap: enc.deflate_device(di, n, do, cap, 10), d50, len(d50) + 64)
        return rc2, buf[:ol], crc2, _blocks(enc)
    add(run, (0, s, crc, blocks))

    d_bz = mix[200000:320000]
    s, ev = oracle_encode(d_bz, 2)
    add(lambda enc: enc.bzip2(d_bz, 14) + (enc.bz2_last_blocks(),), (0, s, crc_reg(d_bz), ev))
    bz_datas = [piece(1, 60000) for _ in range(4)] + [b"", bytes(40000)]
    want = []
    for d in bz_datas:
        s, _ = oracle_encode(d, 2)
        want.append((1 if len(s) >= len(d) else 0, s, crc_reg(d)))
    add(lambda enc: enc.bzip2_batch(bz_datas, 14), want)
    d_bzd = mix[330000:360000]
    s, _ = oracle_encode(d_bzd, 2)

    def run(enc):
        (rc2, ol, crc2), buf = _device_call(lambda di, n, do, cap: enc.bzip2_device(di, n, do, cap, 14), d_bzd, len(d_bzd) + 4096)
        return rc2, buf[:ol], crc2
    add(run, (0, s, crc_reg(d_bzd)))

    d_lz = mix[400000:403000]
    add(lambda enc: enc.lzma(d_lz, 18), oracle_lzma(d_lz, 18))
    lz_datas = [piece(0, 3000) for _ in range(7)] + [b""]
    add(lambda enc: enc.lzma_batch(lz_datas, 16), [oracle_lzma(d, 16) for d in lz_datas])
    hbm_datas = [piece(1000, 2500) for _ in range(2)]          # method 19, LZMA_2_for_Zip_in_Zip: lc + lp = 12, the literal tables in HBM
    add(lambda enc: enc.lzma_batch(hbm_datas, 19), [lzma_expected(d, 19) for d in hbm_datas])
    d_lzd = mix[410000:412000]
    w = oracle_lzma(d_lzd, 16)

    def run(enc):
        (rc2, ol, crc2), buf = _device_call(lambda di, n, do, cap: enc.lzma_device(di, n, do, cap, 16), d_lzd, len(d_lzd) + 4096)
        return rc2, buf[:ol], crc2
    add(run, w)

    w_lz = oracle_lzma(d_lz, 18)

    def run(enc):
        """stopped between two launches of 800 positions, exported, imported again, gone on with: the exported bytes, then the resumed call's from
        that length on, are the oracle's payload"""
        za = product()
        enc.set_knob("lzma_chunk", 800)
        try:
            try:
                enc.lzma(d_lz, 18, feedback=lambda pct: pct >= 40)
                return "not stopped"
            except za.UserAbort:
                pass
            state, head, pos = enc.lzma_export_state(len(d_lz) + 4096)
            enc.lzma_import_state(state)
            rc2, z, crc2 = enc.lzma(d_lz, 18)
            return 0 < pos < len(d_lz), w_lz[1].startswith(head), (rc2, head + z[len(head):], crc2), enc.lzma(d_lz, 18)
        finally:
            enc.set_knob("lzma_chunk", 0)
    add(run, (True, True, w_lz, w_lz))

    d_sh = L.contract_input(1)
    rc, s, reg = L.model_result(d_sh, 1)
    assert rc == 0 and len(d_sh) <= 5000
    add(lambda enc: enc.shrink(d_sh), (0, s, len(s), reg))
    sh_datas = L.batch_contract_inputs(1) + [L.edge_input(1200, seed=4)]
    assert len(sh_datas) == 8 and max(map(len, sh_datas)) <= 5000
    want = [L.model_result(d, 1) for d in sh_datas]
    add(lambda enc: enc.shrink_batch(sh_datas), [(rc, s if rc == 0 else None, reg) for rc, s, reg in want])

    def reduce_node(method):
        rd = [d[:1000] for d in L.batch_contract_inputs(5)]
        want_rows, want_recs = [], []
        for d in rd:
            s, raw, slen, foll, _ = L.reduce(d, method - 1)
            want_rows.append((1 if len(s) >= len(d) else 0, s if len(s) < len(d) else None, crc_reg(d)))
            want_recs.append((raw, bytes(slen), L.followers_in_use(slen, foll)))

        def run(enc):
            rows = enc.reduce_batch(rd, method)
            recs = []
            for i in range(len(rd)):                       # (one launch group: the records are those of the whole list)
                raw, slen, foll = enc.reduce_last_record(i)
                recs.append((raw, bytes(slen), L.followers_in_use(slen, foll)))
            return rows, recs
        add(run, (want_rows, want_recs))
    reduce_node(5)
    reduce_node(2)

    d_rd = L.contract_input(5)
    assert len(d_rd) <= 1000
    w_rd, w_sh = L.model_result(d_rd, 5), L.model_result(d_rd, 1)
    assert w_rd[0] == 0 and w_sh[0] == 0

    def run(enc):
        (rc1, ol1, c1), b1 = _device_call(lambda di, n, do, cap: enc.shrink_device(di, n, do, cap), d_rd, len(d_rd))
        (rc2, ol2, c2), b2 = _device_call(lambda di, n, do, cap: enc.reduce_device(di, n, do, cap, 5), d_rd, len(d_rd))
        return enc.reduce(d_rd, 5), (rc1, b1[:ol1], c1), (rc2, b2[:ol2], c2)
    add(run, ((0, w_rd[1], len(w_rd[1]), w_rd[2]), w_sh, w_rd))

    d_pw = mix[500000:540000]
    add(lambda enc: enc.compress_data(d_pw, 10, password=PW, header=h11(0)), _crypt.compress_data_pw(d_pw, 10, PW, h11(0))[:3])
    d_ps = text[20000:28000]                                   # Preselection_2, neutral, below 9 000 bytes: Deflate_3; the same entry as source code: LZMA_2_for_Source
    want = []
    for hint in (0, 1):
        m = expected_preselect(35, hint, 1, len(d_ps))
        zt, s = cpu_stream(d_ps, m)
        want.append((s, zlib.crc32(d_ps), zt))
    assert [w[2] for w in want] == [8, 14]
    add(lambda enc: [enc.compress_data(d_ps, 35, content_hint=hint) for hint in (0, 1)], want)

    cr_datas = [piece(0, 20000) for _ in range(9)] + [b""]
    keys = [_crypt.init_keys(b"pw%d" % i) for i in range(len(cr_datas))]
    add(lambda enc: enc.crypt_encode_batch(keys, cr_datas), [_crypt.encode(k, d) for k, d in zip(keys, cr_datas)])
    d_cr = mix[560000:590001]
    k0 = _crypt.init_keys(PW)
    w_cr = _crypt.encode(k0, d_cr)

    def run(enc):
        t = _dev(d_cr)
        kd = enc.crypt_encode_device(k0, t.data_ptr(), len(d_cr))
        back = enc.crypt_decode_batch([k0, keys[1]], [w_cr[0], _crypt.encode(keys[1], d_cr[:777])[0]])
        return enc.crypt_encode(k0, d_cr), (_bytes(t), kd), [b for b, _ in back]
    add(run, (w_cr, w_cr, [d_cr, d_cr[:777]]))

    d_crc = mix[600000:700001]

    def run(enc):
        t = _dev(d_crc)
        assert t.data_ptr() % 16 == 0
        return enc.crc32_combine(FF, enc.crc32_device(t.data_ptr(), len(d_crc)), len(d_crc))
    add(run, crc_reg(d_crc))

    trainer = _trained.fixture("wsbase.csv")[:9000]
    src = _trained.fixture("wm1ns.csv")
    tr_datas = [src[300 * k:300 * k + n] for k, n in enumerate((600, 1, 0, 450, 300, 599, 77, 512))]
    stub = _trained.stub_of(trainer)
    skip = max(0, len(stub) - _trained.MARGIN)
    msgs = [_trained.message_of(trainer, d, skip) for d in tr_datas]
    sent = list(msgs)
    sent[3] = damaged(sent[3], lambda s: _trained.model_decode(stub[:skip] + s, len(trainer) + len(tr_datas[3]))[0][0] != 0)
    back = []
    for d, m in zip(tr_datas, sent):
        rec, _ = _trained.model_decode(stub[:skip] + m, len(trainer) + len(d))
        back.append(rec[1][len(trainer):] if rec[0] == 0 else "DataError")
    assert back[3] != tr_datas[3] and [b for k, b in enumerate(back) if k != 3] == [d for k, d in enumerate(tr_datas) if k != 3]

    def run(enc):
        za = product()
        tc = td = None
        try:
            tc = za.TrainedCompression(enc, trainer)
            got = tc.encode(tr_datas)
            forks = (tc.info()["forked"], tc.info()["unforked"])
            td = za.TrainedCompression.for_decoding(enc, tc.stub, tc.skip, tc.trainer_len)
            dec = td.decode(sent, [len(d) for d in tr_datas], errors="return")
            return tc.stub, tc.skip, got, forks, [type(x).__name__ if isinstance(x, Exception) else x for x in dec]
        finally:
            for h in (tc, td):
                if h is not None:
                    h.close()
    add(run, (stub, skip, msgs, (len(tr_datas), 0), back))     # (a trainer of twice the matcher's look-ahead and more: every entry starts from the fork)

    # ---- decoders ----
    d_inf = mix[700000:760000]
    p_inf = _inflate.zlib_raw(d_inf, 9, zlib.Z_DEFAULT_STRATEGY)
    add(lambda enc: enc.inflate(p_inf, len(d_inf)), (d_inf, len(p_inf), crc_reg(d_inf)))
    inf_datas = [piece(0, 12000) for _ in range(29)] + [b""]
    payloads = [_inflate.zlib_raw(d, 1 + i % 9, zlib.Z_DEFAULT_STRATEGY) for i, d in enumerate(inf_datas)]
    payloads[7] = damaged(payloads[7], lambda s: _inflate.model_inflate(s, len(inf_datas[7]))[0] != 0)
    want = _decoded([_inflate.model_inflate(p, len(d))[:5] for p, d in zip(payloads, inf_datas)])
    assert [w[0] for w in want].count(0) == 29 and want[7][0] == _inflate.E_DATA
    add(lambda enc: _decoded(enc.inflate_batch(payloads, [len(d) for d in inf_datas], 8)), want)

    def run(enc):
        r, buf = _device_call(lambda di, n, do, cap: enc.inflate_device(di, n, do, cap), p_inf, len(d_inf))
        return r, buf
    add(run, ((len(d_inf), len(p_inf), crc_reg(d_inf)), d_inf))

    d_par = mix[:620000]
    p_par = _inflate.zlib_raw(d_par, 6, zlib.Z_DEFAULT_STRATEGY)
    assert 150000 <= len(p_par) <= 300000, len(p_par)
    m_par = _inflate_par.model_inflate_par(p_par, len(d_par), 4)
    assert m_par[:5] == (0, d_par, len(d_par), len(p_par), crc_reg(d_par)) and m_par[6]["fell_back"] == 0 and m_par[6]["live_chunks"] >= 2

    def run(enc):
        enc.set_knob("inflate_par_chunk_kib", 4)
        try:
            return enc.inflate_par(p_par, len(d_par)) + (enc.inflate_par_last(),)
        finally:
            enc.set_knob("inflate_par_chunk_kib", 128)
    add(run, (d_par, len(p_par), crc_reg(d_par), m_par[6]))

    def run(enc):
        enc.set_knob("inflate_par_chunk_kib", 4)
        try:
            r, buf = _device_call(lambda di, n, do, cap: enc.inflate_par_device(di, n, do, cap), p_par, len(d_par))
            return r, buf, enc.inflate_par_last()
        finally:
            enc.set_knob("inflate_par_chunk_kib", 128)
    add(run, ((len(d_par), len(p_par), crc_reg(d_par)), d_par, m_par[6]))

    BM = _bunzip2.model()
    d_bu = mix[100000:250000]
    p_bu = bz2.compress(d_bu, 1)                               # level 1: blocks of 100 000 bytes, two of them
    m_bu = _bunzip2.model_bunzip2(p_bu, len(d_bu), records=8)
    assert m_bu[:2] == (0, d_bu) and len(m_bu[6]) == 2

    def run(enc):
        r = enc.bunzip2(p_bu, len(d_bu))
        return r, [BM.bm_rule_name(int(x)).decode() for x in enc.bunzip2_last_records()[:, 0]], [tuple(int(x) for x in b[1:]) for b in enc.bunzip2_last_records(blocks=True)]
    add(run, ((d_bu, len(p_bu), crc_reg(d_bu)), [m_bu[5]], [tuple(int(x) for x in w) for w in m_bu[6]]))

    bu = [(bz2.compress(d_bu, 1), len(d_bu)), (oracle_encode(mix[5000:35000], 2)[0], 30000), (bz2.compress(b"q", 9), 1), (bz2.compress(b"", 9), 0),
          (bz2.compress(text[:50000], 9), 50000), (bz2.compress(text[50000:90000], 5), 40000)]
    bu[4] = (damaged(bu[4][0], lambda s: _bunzip2.model_bunzip2(s, 50000)[0] != 0), 50000)
    m_rows = [_bunzip2.model_bunzip2(p, cap) for p, cap in bu]
    assert [m[0] for m in m_rows] == [0, 0, 0, 0, _bunzip2.E_DATA, 0], [m[0] for m in m_rows]

    def run(enc):
        rows = enc.bunzip2_batch([p for p, _ in bu], [cap for _, cap in bu])
        return _decoded(rows), [BM.bm_rule_name(int(x)).decode() for x in enc.bunzip2_last_records()[:, 0]]
    add(run, (_decoded([m[:5] for m in m_rows]), [m[5] for m in m_rows]))
    p_bd = bz2.compress(text[100000:140000], 9)

    def run(enc):
        return _device_call(lambda di, n, do, cap: enc.bunzip2_device(di, n, do, cap), p_bd, 40000)
    add(run, ((40000, len(p_bd), crc_reg(text[100000:140000])), text[100000:140000]))

    d_ul = mix[800000:820000]
    p_ul = _unlzma.raw_payload(d_ul)
    m_ul = _unlzma.model_unlzma(p_ul, len(d_ul), True)
    assert m_ul[:2] == (0, d_ul)
    add(lambda enc: (enc.unlzma(p_ul, len(d_ul)), [tuple(int(x) for x in r) for r in enc.unlzma_last_records()]), ((d_ul, m_ul[3], crc_reg(d_ul)), [m_ul[6]]))
    ul = [(_unlzma.raw_payload(piece(1, 9000), lc, lp, pb), True) for lc, lp, pb in _unlzma.RAW_PARAMS[:4]]
    ul.append((_unlzma.oracle_payload(mix[830000:832000], 19), True))          # lc + lp = 12: the literal tables in HBM
    ul.append((_unlzma.oracle_payload(mix[840000:843000], 18, end_marker=False), False))
    ul.append((_unlzma.raw_payload(b""), True))
    ul.append((damaged(_unlzma.raw_payload(text[150000:158000]), lambda s: _unlzma.model_unlzma(s, 8000, True)[0] != 0), True))
    ul_caps = [9000, 9000, 9000, 9000, 2000, 3000, 0, 8000]
    m_rows = [_unlzma.model_unlzma(p, cap, eos) for (p, eos), cap in zip(ul, ul_caps)]
    assert [m[0] for m in m_rows][:7] == [0] * 7 and m_rows[7][0] == _unlzma.E_DATA, [m[0] for m in m_rows]

    def run(enc):
        rows = enc.unlzma_batch([p for p, _ in ul], ul_caps, [e for _, e in ul])
        return _decoded(rows), [tuple(int(x) for x in r) for r in enc.unlzma_last_records()]
    add(run, (_decoded([m[:5] for m in m_rows]), [m[6] for m in m_rows]))

    def run(enc):
        return _device_call(lambda di, n, do, cap: enc.unlzma_device(di, n, do, cap), p_ul, len(d_ul))
    add(run, ((len(d_ul), m_ul[3], crc_reg(d_ul)), d_ul))

    ug = [(m, f, s, len(d)) for m, f, s, d in U.valid_streams() if (m <= 5 and len(d) in (300, 1500)) or (m == 6 and (len(d) == 1500 or (len(d) == 530 and f in (0, 6))))]
    ug += [U.crafted()[nm][:4] for nm in ("shrink_special_3", "implode_tree_over")]
    assert len(ug) == 18 and {c[0] for c in ug} == {1, 2, 3, 4, 5, 6} and {c[1] for c in ug if c[0] == 6} >= set(U.IMPLODE_FLAGS)
    m_rows = [U.host_decode(m, f, s, cap) for m, f, s, cap in ug]
    assert [r[5][0] for r in m_rows[-2:]] == [5, 8] and all(r[0] == 0 for r in m_rows[:16])

    def run(enc):
        rows = enc.unlegacy_batch([c[2] for c in ug], [c[3] for c in ug], [c[0] for c in ug], [c[1] for c in ug])
        return _decoded(rows), [tuple(int(x) for x in r) for r in enc.unlegacy_last_records()]
    add(run, (_decoded([r[:5] for r in m_rows]), [r[5] for r in m_rows]))
    d_ug = L.edge_input(1000, seed=91) + L.rnd(92, 24, bytes(range(256))) * 3 + b"z" * 50      # (its last token is a string: cap one short is not a valid stream)
    s_ug, s_im = U.encode(d_ug, 1), U.implode(d_ug, 6)
    m_ug, m_im = U.host_decode(1, 0, s_ug, len(d_ug)), U.host_decode(6, 6, s_im, len(d_ug))
    assert m_ug[:2] == (0, d_ug) and m_im[:2] == (0, d_ug) and U.host_decode(1, 0, s_ug, len(d_ug) - 1)[5][0] == 2

    def run(enc):
        return enc.unlegacy(s_im, len(d_ug), 6, 6), _device_call(lambda di, n, do, cap: enc.unlegacy_device(di, n, do, cap, 1), s_ug, len(d_ug))
    add(run, ((d_ug, m_im[3], crc_reg(d_ug)), ((len(d_ug), m_ug[3], crc_reg(d_ug)), d_ug)))

    # ---- archives ----
    z_entries = [("a/text.txt", text[:30000]), ("b/mix.bin", mix[900000:925000]), ("c/stored.bin", piece(1, 9000)), ("d/empty", b""), ("e/bz.txt", text[30000:52000]),
                 ("f/lz.bin", mix[930000:945000]), ("g/one", b"z"), ("h/zeros", bytes(20000))]
    z_methods = [zipfile.ZIP_DEFLATED, zipfile.ZIP_LZMA, zipfile.ZIP_STORED, zipfile.ZIP_STORED, zipfile.ZIP_BZIP2, zipfile.ZIP_LZMA, zipfile.ZIP_DEFLATED, zipfile.ZIP_BZIP2]
    bio = io.BytesIO()
    with zipfile.ZipFile(bio, "w") as zf:
        for (nm, d), m in zip(z_entries, z_methods):
            zf.writestr(zipfile.ZipInfo(nm, (2024, 5, 6, 7, 8, 10)), d, compress_type=m)
    z_arc = bio.getvalue()
    assert {i.compress_type for i in zipfile.ZipFile(io.BytesIO(z_arc)).infolist()} == {0, 8, 12, 14}

    def run(enc):
        za = product()
        return _extracted(za.UnZip(enc, bzip2=True, lzma=True).extract_device(za.ZipInfo.load_device(_dev(z_arc))))
    add(run, dict(z_entries))

    e_entries = [("p/text.txt", text[60000:85000], 10), ("p/mix.bin", mix[950000:970000], 14), ("p/stored.bin", piece(1, 5000), 0), ("p/rand.bin", bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), 10),
                 ("p/lz.bin", text[90000:92500], 16)]
    rows = []
    for k, (nm, d, m) in enumerate(e_entries):
        payload, crc, zt, _ = _crypt.compress_data_pw(d, m, PW, h11(10 + k))
        rows.append((nm, payload, crc, len(d), zt, True))
    e_arc = _crypt.archive(rows)
    assert [r[4] for r in rows] == [8, 12, 0, 0, 14]

    def run(enc):
        za = product()
        return _extracted(za.UnZip(enc, bzip2=True, lzma=True).extract_device(za.ZipInfo.load_device(_dev(e_arc)), password=PW))
    add(run, {nm: d for nm, d, _ in e_entries})

    def run(enc):
        za = product()
        return _extracted(za.UnZip(enc, bzip2=True, lzma=True).extract_device(za.ZipInfo.load_device(_dev(e_arc)), password=WRONG_PW, errors="collect"))
    add(run, {nm: ("WrongPassword", "entry %r: wrong password" % nm) for nm, _, _ in e_entries})

    lg = []
    for k, m in enumerate((1, 2, 3, 4, 5)):
        d = L.edge_input(900 - 70 * k, seed=300 + k)
        lg.append(("legacy/m%d.txt" % m, U.encode(d, m), m, 0, zlib.crc32(d), len(d), d))
    d = L.edge_input(950, seed=310)
    lg.append(("legacy/m6.txt", U.implode(d, 6), 6, 6, zlib.crc32(d), len(d), d))
    assert all(len(e[1]) < e[5] for e in lg)
    lg_arc = U.zip_of([e[:6] for e in lg])

    def run(enc):
        za = product()
        return _extracted(za.UnZip(enc, legacy=True).extract_device(za.ZipInfo.load_device(_dev(lg_arc))))
    add(run, {e[0]: e[6] for e in lg})

    def run(enc):
        za = product()
        return _extracted(za.UnZip(enc, bzip2=True, lzma=True).extract(za.ZipInfo.load(e_arc), password=PW))
    add(run, {nm: d for nm, d, _ in e_entries})

    def writer_node(entries, method, password=None, legacy=False, ex=True):
        heads = [h11(40 + k) for k in range(len(entries))] if password else None
        want = cpu_archive(entries, method, password, heads)
        if not ex:
            assert want == oracle_zip(entries, method)

        def run(enc):
            zc = product().ZipCreate(enc, method)
            tensors = [_dev(d) for _, d in entries]
            if not ex:
                return _bytes(zc.write_device([nm for nm, _ in entries], tensors))
            return _bytes(zc.write_device_ex([nm for nm, _ in entries], tensors, password=password, _headers=heads, legacy=legacy))
        add(run, want)
    w_entries = [("w/text.txt", text[:20000]), ("w/mix.bin", mix[960000:985000]), ("w/empty", b""), ("w/rand.bin", bytes(rng.integers(0, 256, 2000, dtype=np.uint8))),
                 ("w/one", b"x"), ("w/zeros.bin", bytes(30000))]
    writer_node(w_entries, 10, ex=False)                       # (the archive is oracle_zip's)
    writer_node(w_entries[:5] + [("w/text2.txt", text[200000:260000])], 14, password=PW)
    writer_node([("l/a.txt", text[:2500]), ("l/b.bin", mix[1000:3000]), ("l/empty", b""), ("l/rand", bytes(rng.integers(0, 256, 600, dtype=np.uint8)))], 18)
    writer_node([("s/a.txt", L.edge_input(3000)), ("s/b", L.rnd(21, 700, bytes(range(256)))), ("s/empty", b""), ("s/q", b"q"), ("s/c.txt", L.edge_input(4800, seed=5))], 1, legacy=True)
    writer_node([("r/a.txt", L.edge_input(1000)), ("r/b", L.rnd(22, 500, bytes(range(256)))), ("r/empty", b""), ("r/q", b"q"), ("r/c.txt", L.edge_input(800, seed=6))], 5, legacy=True)

    h_entries = [("h/text.txt", text[100000:130000]), ("h\\rand.bin", bytes(rng.integers(0, 256, 3000, dtype=np.uint8))), ("h/empty", b""), ("h/mix.bin", mix[10000:40000])]
    h_heads = [h11(60 + k) for k in range(len(h_entries))]
    want = with_password(oracle_zip(h_entries, 10), [_crypt.compress_data_pw(d, 10, PW, h)[0] for (_, d), h in zip(h_entries, h_heads)])

    def run(enc):
        zc = product().ZipCreate(enc, 10)
        zc.add_stream(h_entries[0][0], h_entries[0][1], password=PW, _header=h_heads[0])
        zc.add_streams([nm for nm, _ in h_entries[1:]], [d for _, d in h_entries[1:]], password=PW, _headers=h_heads[1:])
        return zc.finish()
    add(run, want)

    rz_plain = [("zeta", text[:3000]), ("alpha", mix[20000:22500]), ("mid", text[5000:7000]), ("lz", text[8000:8700] * 3), ("tiny", text[:17]), ("empty", b"")]
    rows = []
    for (nm, d), m in zip(rz_plain, (0, 8, 14, 18, 10, 0)):    # the source's methods: Store, Deflate_1, BZip2_3, LZMA_3, Deflate_3, Store
        zt, s = cpu_stream(d, m)
        rows.append((nm, s, zlib.crc32(d), len(d), zt))
    rz_src = oracle_zip_compressed(rows)
    want = rezip_model(rz_src, {nm.encode(): d for nm, d in rz_plain}, RL.DEFAULT)
    assert len({c for _, _, c in want[1]}) >= 3, [c for _, _, c in want[1]]

    def run(enc):
        za = product()
        arc, rep = za.ReZip(enc).rezip_device(za.ZipInfo.load_device(_dev(rz_src)), report=True)
        return _bytes(arc), rep["entries"]
    add(run, want)

    want = rezip_model(lg_arc, {e[0].encode(): e[6] for e in lg}, RL.TWELVE)

    def run(enc):
        arc, rep = product().ReZip(enc, legacy=True).rezip(lg_arc, report=True)
        return arc, rep["entries"]
    add(run, want)

    c1 = [("same.txt", text[:9000]), ("other.bin", mix[50000:58000]), ("dir/", b""), ("short.txt", text[9000:12000]), ("only1", b"abc")]
    c2 = [("same.txt", text[:9000]), ("other.bin", mix[50000:54000] + b"\x00" + mix[54001:58000]), ("short.txt", text[9000:12000]), ("only2", b"def")]
    a1, a2 = cpu_archive(c1, 10), cpu_archive(c2, 14)
    counters, verdicts = _rezip.comp_zip([(nm.encode(), d) for nm, d in c1], [(nm.encode(), d) for nm, d in c2])
    assert counters["compare_failures"] == 1 and counters["total_differences"] == 4

    def run(enc):
        za = product()
        r = za.CompZip(enc).compare_device(za.ZipInfo.load_device(_dev(a1)), za.ZipInfo.load_device(_dev(a2)))
        return {k: getattr(r, k) for k in counters}, [(e[5], e[1], e[2]) for e in r.entries], r.damaged
    add(run, (counters, verdicts, 0))

    d_cmp = mix[60000:110000]

    def run(enc):
        a, b = _dev(d_cmp), _dev(d_cmp[:33333] + bytes([d_cmp[33333] ^ 1]) + d_cmp[33334:])
        return enc.compare_device(a.data_ptr(), b.data_ptr(), len(d_cmp)), enc.compare_device(a.data_ptr(), a.data_ptr(), len(d_cmp))
    add(run, (33333, len(d_cmp)))

    d_find = text[:40000]
    for s in (d_find[20000:20005], d_find[30000:30017]):
        w = _findzip.search_1_file(d_find, s, True)
        assert w[0] >= 1

        def run(enc, s=s):
            t = _dev(d_find)
            return enc.find_device(t.data_ptr(), len(d_find), s)
        add(run, w)
    needle = text[31000:31005]
    w = _findzip.find_zip([(nm.encode(), d) for nm, d in z_entries], needle, True)
    assert len(w[0]) >= 1

    def run(enc):
        r = product().FindZip(enc).find(z_arc, needle)
        return [(e[4], e[1], e[2]) for e in r.entries if e[1] > 0], r.in_names, r.lines(), r.damaged
    add(run, (w[0], w[1], w[2], 0))

    # ---- refusals and stops ----
    s_sh = L.model_result(d_sh, 1)[1]
    add(lambda enc: _refusal(lambda: _device_call(lambda di, n, do, cap: enc.shrink_device(di, n, do, cap), d_sh, len(s_sh) - 1), "zada_shrink_device failed: rc=-1", "too small"),
        ("ZadaError", "zada_shrink_device failed: rc=-1", "too small"))
    add(lambda enc: _refusal(lambda: _device_call(lambda di, n, do, cap: enc.unlegacy_device(di, n, do, cap, 1), s_ug, len(d_ug) - 1),
                             "zada_unlegacy_device: ", "unlegacy: entry 0: output beyond cap at input byte "),
        ("DataError", "zada_unlegacy_device: ", "unlegacy: entry 0: output beyond cap at input byte "))

    def run(enc):
        """stopped before its first launch: no state of this stream is exported"""
        return _refusal(lambda: enc.lzma(d_lz, 18, feedback=lambda pct: True)) + _refusal(lambda: enc.lzma_export_state(len(d_lz) + 4096), "zada_lzma_export_state")
    add(run, ("UserAbort", "ZadaError", "zada_lzma_export_state"))
    add(lambda enc: _refusal(lambda: enc.bzip2(text[:20000], 14, cap=100), "zada_bzip2 failed: rc=-1", "too small"), ("ZadaError", "zada_bzip2 failed: rc=-1", "too small"))

    lg_rows = sorted(parse_zip(lg_arc)[0], key=lambda e: e["key"])

    def run(enc):
        import torch
        za = product()
        t = _dev(lg_arc)
        blob = np.frombuffer(b"".join(e["key"] for e in lg_rows) + b"\0", dtype=np.uint8)
        tab = np.zeros(len(lg_rows), dtype=za.Encoder.rezip_dtypes()[0])
        at = 0
        for k, e in enumerate(lg_rows):
            tab[k] = (e["data_offset"], e["csize"], e["usize"], e["crc"], e["time"], e["method"], e["local_flags"], e["version"], 0, len(e["key"]), 0, blob.ctypes.data + at)
            at += len(e["key"])
        cap = enc.rezip_bound(tab, 0)
        out_t = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return _refusal(lambda: enc.rezip_device(t.data_ptr(), len(lg_arc), tab, out_t.data_ptr(), cap), "zada_rezip_device failed: rc=-1",
                        "zada_rezip_device: entry 0: unknown source method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)")
    add(run, ("ZadaError", "zada_rezip_device failed: rc=-1", "zada_rezip_device: entry 0: unknown source method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)"))

    def run(enc):
        zc = product().ZipCreate(enc, 1)
        return _refusal(lambda: zc.write_device(["x"], [_dev(d_rd)]), "zada_zip_device: method 1 (Shrink_1) is not one it takes: Store (0), Deflate_Fixed .. Deflate_R (6 .. 11)")
    add(run, ("ZadaError", "zada_zip_device: method 1 (Shrink_1) is not one it takes: Store (0), Deflate_Fixed .. Deflate_R (6 .. 11)"))
    add(lambda enc: _refusal(lambda: _device_call(lambda di, n, do, cap: enc.unlegacy_device(di, n, do, cap, 9), s_ug, len(d_ug)), "zada_unlegacy_device failed: rc=-1",
                             "method outside 1 .. 6"),
        ("ZadaError", "zada_unlegacy_device failed: rc=-1", "method outside 1 .. 6"))


def differs(got, want):
    """None, or where the two results part: the path of the first differing item (a batch: its first differing entry)."""
    if isinstance(got, np.ndarray) or isinstance(want, np.ndarray):
        return None if np.array_equal(got, want) else "an array"
    if type(got) in (list, tuple) and type(want) in (list, tuple):
        if len(got) != len(want):
            return "%d items, %d expected" % (len(got), len(want))
        for i, (a, b) in enumerate(zip(got, want)):
            w = differs(a, b)
            if w is not None:
                return "item %d of %d: %s" % (i, len(got), w)
        return None
    if isinstance(got, dict) and isinstance(want, dict):
        if sorted(got) != sorted(want):
            return "keys %r, %r expected" % (sorted(got), sorted(want))
        for k in want:
            w = differs(got[k], want[k])
            if w is not None:
                return "%r: %s" % (k, w)
        return None
    if got == want:
        return None
    if isinstance(got, (bytes, bytearray)) and isinstance(want, (bytes, bytearray)):
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        return "%d bytes, %d expected, first difference at byte %d" % (len(got), len(want), at)
    return "%.200r, %.200r expected" % (got, want)
