"""Loader of the ZipCrypto CPU model (tests/crypt/crypt_model.c: Zip.CRC_Crypto restated byte-serially), compiled on first use into a
git-ignored library the way _rich.py builds its own, the encrypted branch of Compress_data_single_method on top of the existing oracles,
and a minimal archive writer for the model's bytes."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np

from _common import ROOT, oracle_deflate

_cache = {}


def model():
    if "m" not in _cache:
        d = os.path.join(ROOT, "tests", "crypt")
        src = os.path.join(d, "crypt_model.c")
        p = os.path.join(d, "libcrypt_model.so")
        if not os.path.exists(p) or os.path.getmtime(p) < os.path.getmtime(src):
            subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", p, src], check=True)
        M = ctypes.CDLL(p)
        M.cm_init_keys.restype = None
        M.cm_init_keys.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
        M.cm_encode.restype = None
        M.cm_encode.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p, ctypes.c_uint64]
        _cache["m"] = M
    return _cache["m"]


def pw_bytes(password):
    """Character'Pos of every character of the password: Latin-1."""
    return password.encode("latin-1") if isinstance(password, str) else bytes(password)


def init_keys(password):
    """Init_Keys (zip-crc_crypto.adb:110-116) -> (key0, key1, key2)."""
    k = (ctypes.c_uint32 * 3)()
    pw = pw_bytes(password)
    model().cm_init_keys(pw, len(pw), k)
    return tuple(k)


def encode(keys, data):
    """Encode (:118-128) -> (cipher text, keys behind it)."""
    k = (ctypes.c_uint32 * 3)(*keys)
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    model().cm_encode(k, buf.ctypes.data if len(buf) else None, len(buf))
    return buf.tobytes(), tuple(k)


def header(keys, random11, crc_final):
    """The 12-byte encryption header (zip-compress.adb:153-161) -> (encoded header, keys behind it = mem_encrypt_pack)."""
    assert len(random11) == 11
    return encode(keys, bytes(random11) + bytes([(crc_final >> 24) & 0xFF]))


def plain_payload(data, method):
    """(rc, stream) of a single method from the existing oracles; rc 1 = compression_ok False."""
    data = bytes(data)
    if method == 0:
        return 1, b""
    if 6 <= method <= 10:
        rc, s, _ = oracle_deflate(data, method)
        return rc, s
    if method == 11:
        from _rich import deflate_r
        return deflate_r(data)
    if 12 <= method <= 14:
        from _bzip2 import oracle_encode
        s, _ = oracle_encode(data, method - 12)
        return (1 if len(s) >= len(data) else 0), s
    if 15 <= method <= 33:
        from test_gpu_lzma_variants import expected              # (oracle_lzma, and the data-type methods' parameters around oracle_lzma_encode)
        rc, s, _ = expected(data, method)
        return rc, s
    raise ValueError(method)


def zip_type(method):
    return 0 if method == 0 else 12 if 12 <= method <= 14 else 14 if 15 <= method <= 33 else 8


def compress_data_pw(data, method, password, random11, content_hint=None):
    """The encrypted branch of Compress_data_single_method (zip-compress.adb:142-241) -> (header + payload, CRC-32, zip_type, attempt)
    where attempt = header + the encoded stream of the compressed attempt, also when Store replaced it."""
    data = bytes(data)
    if content_hint is not None:
        from test_preselect import expected_preselect
        method = expected_preselect(method, content_hint, 1, len(data))
    crc = zlib.crc32(data) & 0xFFFFFFFF                                # the first scan (:152) and Final (:157)
    hdr, kept = header(init_keys(password), random11, crc)             # mem_encrypt_pack := encrypt_pack (:166)
    rc, stream = plain_payload(data, method)
    attempt = hdr + encode(kept, stream)[0]
    if rc == 0:
        return attempt, crc, zip_type(method), attempt
    return hdr + encode(kept, data)[0], crc, 0, attempt               # Store from the kept keys (:224-237)


def archive(entries):
    """A minimal archive of (name, payload, crc, usize, zip_type, encrypted) entries, for a decoder to read the model's bytes from."""
    buf, cd = bytearray(), bytearray()
    for name, payload, crc, usize, zt, enc in entries:
        nm = name.encode("utf-8")
        flag = 0x0800 | (1 if enc else 0) | (2 if zt == 14 else 0)
        off = len(buf)
        buf += struct.pack("<4sHHHIIIIHH", b"PK\x03\x04", 20, flag, zt, 16789 * 65536, crc, len(payload), usize, len(nm), 0) + nm + payload
        cd += struct.pack("<4sHHHHIIIIHHHHHII", b"PK\x01\x02", 20, 20, flag, zt, 16789 * 65536, crc, len(payload), usize, len(nm), 0, 0, 0, 0, 0, off) + nm
    n = len(entries)
    return bytes(buf + cd + struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, n, n, len(cd), len(buf), 0))
