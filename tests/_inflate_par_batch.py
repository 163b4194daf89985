"""Helpers of the tests of the batched parallel Inflate (the knob "inflate_par_batch"): loader of the CPU model
(tests/inflate_par/inflate_par_batch_host.cpp = zip-ada_amd/csrc/zada_inflate_par_batch_plan.h around zada_inflate_par_logic.h, every kernel a
loop), the twenty streams the CPU and the GPU test share ("the rows"), and the raw "archive" of hand-made zada_unzip_entry rows the GPU tests send
through Encoder.unzip_device: streams back to back, outputs at every alignment with guard bytes between them."""
import ctypes
import os
import subprocess
import zlib

import numpy as np

import _inflate
import _inflate_par as P
from _common import ROOT

_cache = {}
_DIR = os.path.join(ROOT, "tests", "inflate_par")
_SRC = os.path.join(_DIR, "inflate_par_batch_host.cpp")
_MAIN = os.path.join(_DIR, "par_batch_check_main.cpp")
_HDRS = [os.path.join(ROOT, "zip-ada_amd", "csrc", h) for h in ("zada_inflate_logic.h", "zada_inflate_par_logic.h", "zada_inflate_par_batch_plan.h")]
BATCH_MIB = 8192          # the default of "inflate_par_batch_mib"
GUARD = 0xA5
START = 0xFFFFFFFF


def build_model():
    p = os.path.join(_DIR, "libinflate_par_batch_host.so")
    if P._stale(p, [_SRC] + _HDRS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", p, _SRC], check=True)
    return p


def build_check_program():
    """The stand-alone program of the sanitizer test: the model and its own main, under ASan + UBSan."""
    p = os.path.join(_DIR, "par_batch_check_asan")
    if P._stale(p, [_SRC, _MAIN] + _HDRS):
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17", "-o", p,
                        _MAIN, _SRC], check=True)
    return p


def model():
    if "m" not in _cache:
        M = ctypes.CDLL(build_model())
        M.ipb_inflate.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 6 + [ctypes.c_uint32] * 5 + [ctypes.c_void_p] * 5
        M.ipb_rule_name.restype = ctypes.c_char_p
        M.ipb_rule_name.argtypes = [ctypes.c_uint]
        _cache["m"] = M
    return _cache["m"]


def model_batch(table, chunk_kib, min_kib=4, deflate64=0, batch_mib=BATCH_MIB, repair_pct=P.REPAIR_PCT, crcs=None):
    """table: list of (format, stream, cap).  -> (per stream (rc, bytes, out_len, in_used, crc register, "taken" | the reason it was handed over |
    "not selected"), the summed record as Encoder.inflate_par_last gives it, the pass cut: indices behind every pass among the selected streams).
    Exact-size heap copies, as _inflate.model_inflate."""
    M = model()
    n = len(table)
    srcs = [np.frombuffer(bytes(s), dtype=np.uint8).copy() if len(s) else np.zeros(1, np.uint8) for _, s, _ in table]
    outs = [np.empty(max(cap, 1), dtype=np.uint8) for _, _, cap in table]
    u64 = lambda xs: np.array(list(xs), dtype=np.uint64)
    fmt = np.array([f for f, _, _ in table], dtype=np.uint32)
    inp, n_in = u64(a.ctypes.data for a in srcs), u64(len(s) for _, s, _ in table)
    outp, cap = u64(a.ctypes.data for a in outs), u64(c for _, _, c in table)
    crc = np.full(n, START, dtype=np.uint32) if crcs is None else np.array(crcs, dtype=np.uint32)
    rc, res, info = np.zeros(n, np.int32), np.zeros((n, 6), np.uint64), np.zeros(8, np.uint64)
    ends, npass = np.zeros(max(n, 1), np.uint32), np.zeros(1, np.uint32)
    r = M.ipb_inflate(n, fmt.ctypes.data, inp.ctypes.data, n_in.ctypes.data, outp.ctypes.data, cap.ctypes.data, crc.ctypes.data, chunk_kib, repair_pct, deflate64, min_kib,
                      batch_mib, rc.ctypes.data, res.ctypes.data, info.ctypes.data, ends.ctypes.data, npass.ctypes.data)
    assert r == 0, r
    rows = []
    for k, (f, s, _) in enumerate(table):
        selected = min_kib > 0 and len(s) >= min_kib << 10 and (f == 8 or deflate64)
        way = "taken" if res[k][4] else P.REASONS[int(res[k][5])] if selected else "not selected"
        rows.append((int(rc[k]), outs[k][:int(res[k][0])].tobytes(), int(res[k][0]), int(res[k][1]), int(res[k][3]), way))
    d = {key: int(info[i]) for i, key in enumerate(P.INFO)}
    d["reason"] = P.REASONS[d["reason"]]
    return rows, d, [int(x) for x in ends[:int(npass[0])]]


def the_rows():
    """(label, data, raw Deflate stream): the six marker streams, the planted false positive, the 2 MiB corpus through zlib 0 / 1 / 6 / 9 and the three
    golden samples through zlib 0 / 6 / 9 -- twenty streams, in this order."""
    if "rows" not in _cache:
        out = [(name, d, s) for name, (d, s, _) in P.marker_streams().items()]
        inner, outer = P.planted_false_positive()
        out.append(("planted", inner, outer))
        c = P.corpus_2m()
        out += [("corpus_2m/zlib%d" % lv, c, _inflate.zlib_raw(c, lv, zlib.Z_DEFAULT_STRATEGY)) for lv in (0, 1, 6, 9)]
        for name in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin"):
            d = _inflate.golden(name)
            out += [("%s/zlib%d" % (name, lv), d, _inflate.zlib_raw(d, lv, zlib.Z_DEFAULT_STRATEGY)) for lv in (0, 6, 9)]
        assert len(out) == 20
        _cache["rows"] = out
    return _cache["rows"]


def single_records(chunk_kib=4):
    """_inflate_par.model_inflate_par of every one of the rows alone (computed once): list of its seven results."""
    if ("single", chunk_kib) not in _cache:
        _cache[("single", chunk_kib)] = [P.model_inflate_par(s, len(d), chunk_kib) for _, d, s in the_rows()]
    return _cache[("single", chunk_kib)]


def rows_model(batch_mib=BATCH_MIB):
    """model_batch of the rows at 4 KiB chunks (computed once per bound)."""
    if ("rows_model", batch_mib) not in _cache:
        _cache[("rows_model", batch_mib)] = model_batch([(8, s, len(d)) for _, d, s in the_rows()], 4, batch_mib=batch_mib)
    return _cache[("rows_model", batch_mib)]


def sum_records(recs):
    """The sum zada_unzip_device leaves of the records of its large entries, one after the other."""
    d = {k: sum(r[k] for r in recs) for k in P.INFO if k != "reason"}
    fell = [r["reason"] for r in recs if r["fell_back"]]
    d["reason"] = fell[-1] if fell else "none"
    return d


def flip(stream, usize, refused=False):
    """One bit of the stream flipped, near its middle: the first place where zlib then refuses the stream or decodes as many bytes as before -- the
    rule of test_gpu_inflate_par._flip, on a raw stream.  refused: the first such place where zlib refuses (a raw stream has no CRC-32 of its own
    to tell the other kind of damage by)."""
    if refused:
        # (the decoder's state in front of the middle once; a trial reads the 32 KiB behind its flip, where zlib meets nearly every broken code)
        mid = len(stream) // 2
        head = zlib.decompressobj(-15)
        head.decompress(stream[:mid])
        for pos in range(mid, len(stream)):
            b = bytearray(stream[mid:pos + 32768])
            b[pos - mid] ^= 0x10
            try:
                head.copy().decompress(bytes(b))
            except zlib.error:
                b = bytearray(stream)
                b[pos] ^= 0x10
                return bytes(b)
        raise AssertionError("no such place")
    for pos in range(len(stream) // 2, len(stream)):
        b = bytearray(stream)
        b[pos] ^= 0x10
        try:
            ok = len(zlib.decompressobj(-15).decompress(bytes(b), usize + 1)) == usize
        except zlib.error:
            ok = True
        if ok:
            return bytes(b)
    raise AssertionError("no such place")


def layout(caps, lead=32):
    """Output offsets for rows of `caps` bytes: every run of sixteen rows takes all sixteen alignments of its first byte, each row at the alignment
    (not yet used in its run) nearest behind the row before -- so rows are adjacent byte for byte wherever that alignment is free.  -> (offsets, size
    of the buffer: `lead` guard bytes in front and at least that many behind)"""
    offs, cur, free = [], lead, []
    for cap in caps:
        if not free:
            free = list(range(16))
        a = min(free, key=lambda x: (x - cur) % 16)
        free.remove(a)
        cur += (a - cur) % 16
        offs.append(cur)
        cur += cap
    return offs, cur + lead


def run_table(enc, table, crcs=None, out_offs=None):
    """table: list of (method, stream, cap) through ONE Encoder.unzip_device call as a raw archive: the streams back to back in a device buffer that
    ends at the last one's last byte, the outputs by layout () in a buffer of GUARD.  -> (the call's rc, the structured results, the host copy of the
    output buffer, the offsets).  Asserts that no byte outside the ranges [out_off, out_off + out_len) changed -- for a row that failed, outside
    [out_off, out_off + cap): the one-wave decoder, which judges every such row, writes what it decoded before it met the damage."""
    import torch
    n = len(table)
    arc = b"".join(bytes(s) for _, s, _ in table)
    offs, total = layout([cap for _, _, cap in table]) if out_offs is None else out_offs
    tab = np.zeros(n, dtype=enc.unzip_dtypes()[0])
    tab["n_in"] = [len(s) for _, s, _ in table]
    tab["in_off"] = np.cumsum(tab["n_in"]) - tab["n_in"]
    tab["out_off"], tab["cap"], tab["method"] = offs, [cap for _, _, cap in table], [m for m, _, _ in table]
    t_arc = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).cuda()
    t_out = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, res = enc.unzip_device(t_arc.data_ptr(), len(arc), t_out.data_ptr(), total, tab, None, START if crcs is None else np.array(crcs, dtype=np.uint32))
    torch.cuda.synchronize()
    host = t_out.cpu().numpy()
    keep = np.ones(total, dtype=bool)
    for k in range(n):
        keep[offs[k]:offs[k] + (int(res["out_len"][k]) if res["rc"][k] == 0 else table[k][2])] = False
    bad = np.flatnonzero(keep & (host != GUARD))
    assert len(bad) == 0, "bytes outside the delivered ranges were written: offsets %r" % [int(x) for x in bad[:8]]
    return rc, res, host, offs


def row_bytes(host, offs, res, k):
    return host[offs[k]:offs[k] + int(res["out_len"][k])].tobytes()
