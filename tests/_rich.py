"""Loader of the Deflate_R CPU model (tests/rich/rich_model.c), compiled on first use into a git-ignored library the way
_common.hostcheck() builds its own, and the Deflate_R stream the model's tokens give."""
import ctypes
import os
import subprocess

import numpy as np

from _common import ROOT, oracle

TOKEN_MATCH = 0x80000000
SECTOR = 8192
_cache = {}


def model():
    if "r" not in _cache:
        d = os.path.join(ROOT, "tests", "rich")
        src = os.path.join(d, "rich_model.c")
        p = os.path.join(d, "librich_model.so")
        if not os.path.exists(p) or os.path.getmtime(p) < os.path.getmtime(src):
            subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", p, src], check=True)
        M = ctypes.CDLL(p)
        for f in (M.rich_restate, M.rich_closed):
            f.restype = ctypes.c_uint64
            f.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        _cache["r"] = M
    return _cache["r"]


def _run(fn, data, fill):
    data = bytes(data)
    t = np.zeros(len(data) + 8, dtype=np.uint32)
    capped = ctypes.c_uint64(0)
    k = fn(data, len(data), fill, t.ctypes.data, len(t), ctypes.byref(capped))
    assert k <= len(t), k
    return t[:k], capped.value


def restate(data, fill=0):
    """LZ77_by_Rich restated literally: (tokens, searches cut at 4 096 candidates)."""
    return _run(model().rich_restate, data, fill)


def closed(data, fill=0):
    """The per-sector closed form the GPU implements: (tokens, searches cut at 4 096 candidates)."""
    return _run(model().rich_closed, data, fill)


def tokens(data, fill=0):
    return closed(data, fill)[0]


def deflate_r(data, toks=None, blocks=None):
    """The Deflate_R stream of `data`: (rc, bytes); rc 1 = Compression_inefficient.
    Deflate_R differs from Deflate_3 in its LZ77 front end only (zip-compress-deflate.adb:1573-1579).  Behind it, both have
    max_choice = 3 (:1310-1311: the splitter tests every step level), and the same Put_or_delay_* path (:1437-1456), block
    chooser and emitter.  So the oracle's entropy stage with method 10 (Deflate_3), fed the model's tokens, writes the stream
    the reference writes for Deflate_R.  blocks: collects the block trace (first atom, atoms, format, bits)."""
    data = bytes(data)
    if toks is None:
        toks = tokens(data)
    toks = np.ascontiguousarray(toks, dtype=np.uint32)
    n = len(data)
    out = ctypes.create_string_buffer(n + 64)
    ol = ctypes.c_uint64(0)
    cb = None
    if blocks is not None:
        from _common import TRACE

        def tr(_u, kind, a, b, c, d):
            if kind == 2:
                blocks.append((a, b, c, d))
        cb = TRACE(tr)
    rc = oracle().zo_deflate_from_tokens(data, n, toks.ctypes.data if len(toks) else None, len(toks), 10, out, n + 64, ctypes.byref(ol),
                                         ctypes.cast(cb, ctypes.c_void_p) if cb else None, None)
    assert rc in (0, 1), rc
    return rc, out.raw[:ol.value]


def token_spans(toks):
    """(start position, length, distance or 0) of every token."""
    toks = np.asarray(toks, dtype=np.uint32)
    is_m = (toks & TOKEN_MATCH) != 0
    lens = np.where(is_m, (toks >> 16) & 0x1FF, 1).astype(np.int64)
    dist = np.where(is_m, toks & 0xFFFF, 0).astype(np.int64)
    pos = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64) if len(toks) else np.zeros(0, dtype=np.int64)
    return pos, lens, dist, is_m
