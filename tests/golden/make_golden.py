"""Generates the committed fixtures under tests/golden/ (run in the BUILD container, where
/root/reference exists; the fixtures -- data only -- travel to the GPU box, the reference does not).

  llhc_vectors.json   the three frequency vectors the reference's own LLHC test program feeds to
                      Length_Limited_Coding (test/test_llhc.adb:15, 46, 69-128; that program prints
                      the lengths and asserts nothing) + the oracle's code lengths ("self-pinned")
  sample.xls, sample.jpg, sample_pgm_100k.bin   data files of the reference's test corpus
                      (test/test_data/), the edge cases test/test_za.hac zips (sample.jpg is the
                      file behind lz77.adb:740-744)
  deflate_digests.json  SHA-256 + size of the oracle's stream for every (input, method) of the
                      parity matrix ("self-pinned": detects any later drift of the oracle and gives
                      the GPU tests a second, oracle-free comparison)
  lzma_digests.json   the same for the LZMA half (methods 15 .. 18), with the counters of the DL-code variants taken
  bzip2_digests.json  the same for the BZip2 half (methods 12 .. 14), with the block / tactic trace; every stream was
                      decompressed with libbz2 when the file was made
  atsize_digests.json  SHA-256 + size + CRC of the oracle's stream for the streams the at-size GPU tests make (1 GiB to 4.2 GiB;
                      `make_golden.py atsize`, needs neither the reference nor a GPU: the corpus generator and the oracle alone).
                      BZip2_3 at size is left out (the oracle would take 80 minutes per stream): see ATSIZE below
  zlib_tokens_*.npz   position-indexed LZ77 tokens made by libz 1.2.11 deflateTune for the
                      fixture files (the independent pin of the LZ77 stage)
"""
import ctypes
import hashlib
import json
import os
import re
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _common import METHODS, LEVEL, TUNE, oracle, zlibpin, oracle_deflate, edge_inputs  # noqa: E402

REF = "/root/reference"


def llhc_vectors():
    src = open(os.path.join(REF, "test", "test_llhc.adb")).read()
    v1 = [int(x) for x in re.search(r"freq := \(([\d, ]+)\);\s*\n\s*for m in 4 \.\. 5", src).group(1).split(",")]
    v2 = [int(x) for x in re.search(r"\n\s*freq := \(([\d, ]+)\);\s*--  OK after fixing LLHC", src).group(1).split(",")]
    body = src[src.index("procedure Test_3"):]
    pairs = re.findall(r"(\d+)\s*=>\s*(\d+)", body[:body.index("New_Line")])
    v3 = [0] * 288
    for k, v in pairs:
        v3[int(k)] = int(v)
    out = []
    for name, freq, mbs in (("test_1", v1, (4, 5)), ("test_2", v2, (7,)), ("test_3", v3, (15,))):
        for mb in mbs:
            f = np.array(freq, dtype=np.uint64)
            bl = np.zeros(len(freq), dtype=np.int32)
            assert oracle().zo_llhc(f.ctypes.data, len(freq), mb, bl.ctypes.data) == 0
            out.append(dict(name=name, max_bits=mb, freq=freq, lengths=bl.tolist(), source="test/test_llhc.adb", pinned="self (oracle)"))
    json.dump(out, open(os.path.join(HERE, "llhc_vectors.json"), "w"))
    return out


def data_files():
    td = os.path.join(REF, "test", "test_data")
    shutil.copyfile(os.path.join(td, "sample.xls"), os.path.join(HERE, "sample.xls"))
    shutil.copyfile(os.path.join(td, "sample.jpg"), os.path.join(HERE, "sample.jpg"))
    open(os.path.join(HERE, "sample_pgm_100k.bin"), "wb").write(open(os.path.join(td, "sample.pgm"), "rb").read()[:100000])
    for f in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin"):
        os.chmod(os.path.join(HERE, f), 0o644)


def zlib_tokens():
    for f in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin"):
        d = open(os.path.join(HERE, f), "rb").read()
        for lvl in (6, 8, 10):
            z = np.zeros(len(d), dtype=np.uint32)
            rc = zlibpin().zp_zlib_position_tokens(d, len(d), *TUNE[lvl], z.ctypes.data)
            assert rc == 0, rc
            np.savez_compressed(os.path.join(HERE, "zlib_tokens_%s_L%d.npz" % (f.replace(".", "_"), lvl)), tokens=z)


def digests():
    cases = dict(edge_inputs())
    for f in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin"):
        cases[f] = open(os.path.join(HERE, f), "rb").read()
    out = {}
    for name, d in sorted(cases.items()):
        for m in METHODS:
            rc, z, crc = oracle_deflate(d, m)
            out["%s|%d" % (name, m)] = dict(rc=rc, size=len(z), sha256=hashlib.sha256(z).hexdigest() if rc == 0 else None,
                                           in_sha256=hashlib.sha256(d).hexdigest(), crc=crc ^ 0xFFFFFFFF)
    json.dump(out, open(os.path.join(HERE, "deflate_digests.json"), "w"), indent=0, sort_keys=True)


def bzip2_digests():
    """bzip2_digests.json: SHA-256 + size of the oracle's BZip2 stream per (input, method 12..14), the block trace (raw start,
    raw length, tactic, sub-blocks) and whether libbz2 gives the input back ("self-pinned" + round trip)."""
    import bz2
    from _bzip2 import oracle_encode, bz_inputs
    cases = bz_inputs()
    for f in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin"):
        cases[f] = open(os.path.join(HERE, f), "rb").read()
    out = {}
    for name, d in sorted(cases.items()):
        for m in (12, 13, 14):
            if m != 14 and len(d) > 400000:
                continue
            z, ev = oracle_encode(d, m - 12)
            if len(d):
                assert bz2.decompress(z) == d, (name, m)
            out["%s|%d" % (name, m)] = dict(size=len(z), sha256=hashlib.sha256(z).hexdigest(), in_sha256=hashlib.sha256(d).hexdigest(), blocks=ev)
    json.dump(out, open(os.path.join(HERE, "bzip2_digests.json"), "w"), indent=0, sort_keys=True)


def lzma_digests():
    """lzma_digests.json: SHA-256 + size of the oracle's Zip LZMA payload per (input, method 15..18) and the counters of the
    choices taken ("self-pinned"); liblzma gives the input back for every one of them."""
    from _lzmah import oracle_lzma, oracle_lzma_encode, lz_inputs, lzma_decode
    cases = lz_inputs()
    for f in ("sample.xls", "sample.jpg", "sample_pgm_100k.bin"):
        cases[f] = open(os.path.join(HERE, f), "rb").read()
    out = {}
    for name, d in sorted(cases.items()):
        for m in (15, 16, 17, 18):
            rc, z, crc = oracle_lzma(d, m)
            assert lzma_decode(z, 4) == d, (name, m)
            st = oracle_lzma_encode(d, m - 15)[1]
            out["%s|%d" % (name, m)] = dict(rc=rc, size=len(z), sha256=hashlib.sha256(z).hexdigest(), in_sha256=hashlib.sha256(d).hexdigest(), choices=st)
    json.dump(out, open(os.path.join(HERE, "lzma_digests.json"), "w"), indent=0, sort_keys=True)


# The streams the at-size GPU tests make (tests/test_gpu_parity.py::test_full_size_properties, tests/test_gpu_atsize.py).  name ->
# (corpus version, seed, n, method, through zo_compress_data).  The oracle runs one core at about 3 MB/s (Deflate_3) and 9 MB/s
# (Deflate_1): the longest of the four takes about a quarter of an hour, `atsize` runs them as four processes side by side (each
# needs about twice its input in RAM).  BZip2_3 at size (the 1.2 GiB and 1.125 GiB streams of test_gpu_atsize.py) is not here:
# zo_bzip2 takes 64.5 s for 16 MiB of the corpus on one core, which projects to 82 and 77 minutes for the two streams -- beyond the
# 45 minutes of one core set as the limit for a fixture that has to be made again whenever the corpus generator changes.
ATSIZE = {
    "c2_1gib_v2": (2, 0x5A1E51A, 1 << 30, 10, False),
    "two_and_a_half_gib": (1, 0x5A1E51A, (5 << 29) + 12345, 10, False),
    "c3_rank_shape": (1, 0x5A1E51A, (64 << 20) + (2 << 30) + (64 << 20), 10, False),
    "zip64_big_bin": (1, 0x5A1E51A, (4 << 30) + (200 << 20) + 77, 8, True),
}


def atsize_one(name):
    """One entry of atsize_digests.json, printed as a JSON line (no copy of the input or the stream is made on the way)."""
    import time
    from _common import mixlib
    version, seed, n, method, through_compress_data = ATSIZE[name]
    O = ctypes.CDLL(oracle()._name)                 # (a handle of its own: the input goes in as a pointer, not as bytes)
    M = mixlib()
    d = np.zeros(n, dtype=np.uint8)
    (M.zada_silesia_mix_v2 if version >= 2 else M.zada_silesia_mix)(seed, 0x1F, 0, n, d.ctypes.data)
    out = np.zeros(n + 64, dtype=np.uint8)
    ol = ctypes.c_uint64(0)
    crc = ctypes.c_uint32(0xFFFFFFFF)
    pin, pout = ctypes.c_void_p(d.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    t0 = time.time()
    if through_compress_data:
        zt = ctypes.c_uint16(0)
        rc = O.zo_compress_data(pin, ctypes.c_uint64(n), method, pout, ctypes.c_uint64(n + 64), ctypes.byref(ol), ctypes.byref(crc), ctypes.byref(zt))
        assert zt.value == 8, zt.value
        crc_final = crc.value
    else:
        rc = O.zo_deflate(pin, ctypes.c_uint64(n), method, pout, ctypes.c_uint64(n + 64), ctypes.byref(ol), ctypes.byref(crc), None, None, None, None)
        crc_final = crc.value ^ 0xFFFFFFFF
    assert rc == 0, rc
    z = memoryview(out)[:ol.value]
    e = dict(version=version, seed=seed, n=n, in_sha256=hashlib.sha256(memoryview(d)).hexdigest(), method=method,
             through="zo_compress_data" if through_compress_data else "zo_deflate", rc=rc, size=ol.value,
             sha256=hashlib.sha256(z).hexdigest(), crc=crc_final, oracle_seconds=round(time.time() - t0))
    print(json.dumps({name: e}), flush=True)


def atsize_digests():
    import subprocess
    procs = [(k, subprocess.Popen([sys.executable, os.path.abspath(__file__), "atsize", k], stdout=subprocess.PIPE)) for k in ATSIZE]
    out = {}
    for k, p in procs:
        text = p.communicate()[0]
        assert p.returncode == 0, k
        out.update(json.loads(text.decode().strip().splitlines()[-1]))
    json.dump(out, open(os.path.join(HERE, "atsize_digests.json"), "w"), indent=0, sort_keys=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "atsize":
        atsize_one(sys.argv[2]) if len(sys.argv) > 2 else atsize_digests()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "bzip2":
        bzip2_digests()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "lzma":
        lzma_digests()
        sys.exit(0)
    llhc_vectors()
    data_files()
    zlib_tokens()
    digests()
    bzip2_digests()
    lzma_digests()
    print("golden fixtures written to", HERE)
