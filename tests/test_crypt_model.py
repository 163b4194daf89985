"""ZipCrypto without a GPU.  The CPU model (tests/crypt/crypt_model.c, Zip.CRC_Crypto restated byte-serially) is pinned by a decoder it
shares no code with: archives assembled from the model's bytes are read back by zipfile with pwd= (and by unzip -P where it is installed).
The product library's pure host entry points, zada_crypt_init_keys and zada_crypt_header, are then compared with the model; the library is
loaded in a child process, as test_preselect.py does."""
import json
import os
import shutil
import subprocess
import sys
import zipfile
import zlib
import io

import numpy as np
import pytest

import _crypt
from _common import ROOT, oracle_deflate, silesia_mix

PASSWORDS = [b"a", b"secret", "p\xe4ssw\xf6rd \xff\x80".encode("latin-1"), bytes(range(1, 64))]
SIZES = (0, 1, 11, 12, 13, 100000)


def _h11(seed):
    return bytes(np.random.RandomState(seed).randint(0, 256, 11).astype(np.uint8))


def _stored(data, pw, h11):
    crc = zlib.crc32(data) & 0xFFFFFFFF
    hdr, kept = _crypt.header(_crypt.init_keys(pw), h11, crc)
    return hdr + _crypt.encode(kept, data)[0], crc, len(data), 0


def _deflated(data, pw, h11):
    payload, crc, zt, _ = _crypt.compress_data_pw(data, 10, pw, h11)
    return payload, crc, len(data), zt


def test_model_known_keys():
    # Init_Keys of the empty password leaves the three constants (zip-crc_crypto.adb:112)
    assert _crypt.init_keys(b"") == (0x12345678, 0x23456789, 0x34567890)
    assert _crypt.encode((1, 2, 3), b"") == (b"", (1, 2, 3))


@pytest.mark.parametrize("pw", PASSWORDS, ids=lambda p: "pw%d" % len(p))
def test_model_archives_open_in_zipfile(pw):
    entries, want = [], {}
    for i, n in enumerate(SIZES):
        data = silesia_mix(n, class_mask=1, offset=i * 65536)
        for kind, make in (("stored", _stored), ("deflated", _deflated)):
            name = "%s_%d.txt" % (kind, n)
            payload, crc, usize, zt = make(data, pw, _h11(100 + i))
            assert zt in (0, 8) and (zt == 8 or len(payload) == 12 + len(data))
            entries.append((name, payload, crc, usize, zt, True))
            want[name] = data
    assert any(e[4] == 8 for e in entries) and any(e[4] == 0 for e in entries)
    z = zipfile.ZipFile(io.BytesIO(_crypt.archive(entries)))
    for name, data in want.items():
        assert z.read(name, pwd=pw) == data, name


def test_model_encode_in_pieces_is_encode_of_the_whole():
    data = silesia_mix(50000)
    keys = _crypt.init_keys(b"pieces")
    whole, kw = _crypt.encode(keys, data)
    for piece in (1, 12, 4097):
        k, out = keys, b""
        for o in range(0, len(data), piece):
            ct, k = _crypt.encode(k, data[o:o + piece])
            out += ct
        assert out == whole and k == kw, piece


def test_wrong_password_is_refused():
    data = silesia_mix(5000, class_mask=1)
    pw, h11 = b"right", _h11(5)
    payload, crc, usize, zt = _stored(data, pw, h11)
    # a wrong password passes zipfile's check with probability 1 / 256: pick one whose decrypted check byte DIFFERS from crc >> 24, so that the
    # refusal is certain (the model decrypts the header: decoding is Encode's mirror image, keys updated with the plain byte)
    wrong = None
    for k in range(256):
        cand = b"wrong%d" % k
        keys = list(_crypt.init_keys(cand))
        plain = bytearray()
        for c in payload[:12]:
            # Decode (:130-136): plain byte = cipher byte xor Crypto_code, then Update_keys with the plain byte -- via Encode of the plain byte
            code = _crypt.encode(tuple(keys), b"\0")[0][0]
            b = c ^ code
            keys = list(_crypt.encode(tuple(keys), bytes([b]))[1])
            plain.append(b)
        if plain[11] != (crc >> 24):
            wrong = cand
            break
    assert wrong is not None
    z = zipfile.ZipFile(io.BytesIO(_crypt.archive([("f.txt", payload, crc, usize, zt, True)])))
    with pytest.raises(RuntimeError):
        z.read("f.txt", pwd=wrong)
    assert z.read("f.txt", pwd=pw) == data


@pytest.mark.skipif(shutil.which("unzip") is None, reason="unzip is not installed")
def test_model_archive_opens_in_unzip(tmp_path):
    pw = b"unzip-pw"
    data = silesia_mix(600000)
    entries = [("big.bin",) + _deflated(data, pw, _h11(1)) + (True,), ("stored.bin",) + _stored(data[:70000], pw, _h11(2)) + (True,),
               ("empty",) + _stored(b"", pw, _h11(3)) + (True,)]
    p = tmp_path / "model.zip"
    p.write_bytes(_crypt.archive(entries))
    r = subprocess.run(["unzip", "-P", pw.decode(), "-t", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(["unzip", "-P", "not-it", "-t", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0


def test_compress_data_pw_model_store_fallback_keeps_the_header():
    rnd = bytes(np.random.RandomState(3).randint(0, 256, 4096).astype(np.uint8))
    rc, _, _ = oracle_deflate(rnd, 10)
    assert rc == 1
    payload, crc, zt, attempt = _crypt.compress_data_pw(rnd, 10, b"pw", _h11(9))
    assert zt == 0 and len(payload) == len(rnd) + 12 and payload[:12] == attempt[:12] and payload != attempt


CHILD = r'''
import ctypes, json, os, sys
ROOT = %(root)r
L = ctypes.CDLL(os.path.join(ROOT, "zip-ada_amd", "libzada_hip.so"))
u32p = ctypes.POINTER(ctypes.c_uint32)
L.zada_crypt_init_keys.restype = None
L.zada_crypt_init_keys.argtypes = [ctypes.c_char_p, ctypes.c_uint64, u32p]
L.zada_crypt_header.restype = None
L.zada_crypt_header.argtypes = [u32p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
req = json.loads(sys.stdin.read())
out = {"keys": [], "headers": []}
for pw in req["passwords"]:
    pw = bytes(pw)
    k = (ctypes.c_uint32 * 3)()
    L.zada_crypt_init_keys(pw, len(pw), k)
    out["keys"].append(list(k))
for keys, h11, crc in req["headers"]:
    k = (ctypes.c_uint32 * 3)(*keys)
    o = ctypes.create_string_buffer(12)
    L.zada_crypt_header(k, bytes(h11), crc, o)
    out["headers"].append([list(o.raw), list(k)])
print(json.dumps(out))
'''


def test_product_init_keys_and_header_match_the_model():
    rs = np.random.RandomState(17)
    pws = [b"", b"a", b"secret"] + PASSWORDS + [bytes(rs.randint(0, 256, k).astype(np.uint8)) for k in (1, 5, 40, 300)]
    hdrs = [([int(x) for x in rs.randint(0, 1 << 32, 3, dtype=np.uint64)], [int(x) for x in rs.randint(0, 256, 11)], int(rs.randint(0, 1 << 32, dtype=np.uint64)))
            for _ in range(40)]
    hdrs += [([0, 0, 0], [0] * 11, 0), ([0xFFFFFFFF] * 3, [255] * 11, 0xFFFFFFFF)]
    req = {"passwords": [list(p) for p in pws], "headers": hdrs}
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], input=json.dumps(req), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for pw, k in zip(pws, got["keys"]):
        assert tuple(k) == _crypt.init_keys(pw), pw
    for (keys, h11, crc), (o, k) in zip(hdrs, got["headers"]):
        want, kw = _crypt.header(tuple(keys), bytes(h11), crc)
        assert bytes(o) == want and tuple(k) == kw


def test_crypt_host_side_is_clean_under_asan_and_ubsan():
    """zada_crypt_init_keys / zada_crypt_header of the instrumented library (`make asan`, as test_host_asan.py loads it) against the model, and
    the new entry points' argument checks: no context, null buffers, an empty password -> ZADA_E_INVALID, never a crash."""
    import glob
    csrc = os.path.join(ROOT, "zip-ada_amd", "csrc")
    lib = os.path.join(ROOT, "zip-ada_amd", "variants", "libzada_hip_asan.so")
    srcs = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(ROOT, "include", "zada.h")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rt = glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so")
    assert rt, "clang's ASan runtime (hipcc's) is not installed"
    rs = np.random.RandomState(23)
    pws = [b"", b"x", bytes(rs.randint(0, 256, 1000).astype(np.uint8))]
    hdrs = [([int(x) for x in rs.randint(0, 1 << 32, 3, dtype=np.uint64)], [int(x) for x in rs.randint(0, 256, 11)], int(rs.randint(0, 1 << 32, dtype=np.uint64))) for _ in range(8)]
    child = CHILD.replace('"libzada_hip.so"', '"variants", "libzada_hip_asan.so"').replace("print(json.dumps(out))", r'''
vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
k = (ctypes.c_uint32 * 3)()
L.zada_crypt_init_keys(None, 0, k)                   # (an empty password is no bytes at all)
out["empty"] = list(k)
buf = ctypes.create_string_buffer(64)
L.zada_crypt_encode.argtypes = [vp, u32p, vp, u64]
L.zada_crypt_encode_device.argtypes = [vp, u32p, vp, u64]
L.zada_crypt_encode_batch.argtypes = [vp, i32, vp, vp, vp]
L.zada_compress_data_pw.argtypes = [vp, i32, i32, ctypes.c_char_p, u64, ctypes.c_char_p, vp, u64, vp, u64, vp, vp, vp, vp]
out["rc"] = [L.zada_crypt_encode(None, k, buf, 64), L.zada_crypt_encode(None, None, None, 0), L.zada_crypt_encode_device(None, k, buf, 64),
             L.zada_crypt_encode_batch(None, 1, None, None, None), L.zada_crypt_encode_batch(None, -1, None, None, None),
             L.zada_compress_data_pw(None, 10, 0, b"pw", 2, bytes(11), buf, 64, buf, 64, buf, buf, buf, None),
             L.zada_compress_data_pw(None, 10, 0, None, 0, None, None, 0, None, 0, None, None, None, None)]
print(json.dumps(out))''')
    req = {"passwords": [list(p) for p in pws], "headers": hdrs}
    env = dict(os.environ, LD_PRELOAD=rt[0], ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:protect_shadow_gap=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-c", child % {"root": ROOT}], input=json.dumps(req), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert [tuple(k) for k in got["keys"]] == [_crypt.init_keys(p) for p in pws] and tuple(got["empty"]) == _crypt.init_keys(b"")
    for (keys, h11, crc), (o, k) in zip(hdrs, got["headers"]):
        assert (bytes(o), tuple(k)) == _crypt.header(tuple(keys), bytes(h11), crc)
    assert got["rc"] == [-1] * 7, got["rc"]
