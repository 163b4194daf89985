"""GPU script: what extracting an archive that lies in device memory gives.  One process; warm-up, then the median of 9 runs; wall
clock around UnZip.extract_device with the archive tensor resident (the call synchronises), device times per kernel from HIP events on the
context's stream (last_timing).
  small/deflate, small/bzip2, small/lzma: an archive of 10 000 entries of 16 KiB of the benchmark corpus (silesia_mix_v2), written by the product
     with Deflate_3, BZip2_3, LZMA_3; small/deflate_pw: the Deflate archive with a password.
  stored_1g: one stored entry of 1 GiB.
Per case: extract_device; UnZip.extract on the same archive as bytes in the same run (the host-pointer path: the yardstick); sixteen host threads of
zlib, libbz2 or liblzma over the entries' payloads, each thread a contiguous sixteenth.  For the stored gigabyte also the one-wave k_inf_crc on a
64 MiB slice of the same buffer (a stored-block Deflate stream through zada_inflate_device; the whole gigabyte would only take sixteen times as long).
Arguments: the JSON file to write (default: standard output only); a second argument names the cases, comma-separated."""
import bz2
import json
import os
import statistics
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import product
from _lzmah import lzma_decode

Z = product()
enc = Z.Encoder(0)
uz = Z.UnZip(enc, bzip2=True, lzma=True)
E, SZ, THREADS, RUNS = 10000, 16384, 16, 9
PW = "perf-password"
cases = sys.argv[2].split(",") if len(sys.argv) > 2 else ["small/deflate", "small/bzip2", "small/lzma", "small/deflate_pw", "stored_1g"]
res = {"corpus": "silesia_mix_v2", "tree": os.environ.get("ZADA_TREE"), "runs": RUNS, "cases": {}}


def dump():
    if len(sys.argv) > 1 and sys.argv[1] != "-":
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


def med(xs):
    return {"median": statistics.median(xs), "runs": xs}


def walls(fn, runs=RUNS, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def threads16(info, arc, one):
    """Sixteen threads, each decoding a contiguous sixteenth of the entries' payloads; -> milliseconds per run."""
    pay = [arc[e.data_offset:e.data_offset + e.csize] for e in info.entries]
    cuts = [len(pay) * k // THREADS for k in range(THREADS + 1)]

    def loop(k):
        return sum(len(one(p)) for p in pay[cuts[k]:cuts[k + 1]])
    want = sum(e.usize for e in info.entries)
    with ThreadPoolExecutor(THREADS) as pool:
        def run():
            assert sum(pool.map(loop, range(THREADS))) == want
        return walls(run, runs=7, warm=2)


def measure(name, arc, password, host_one, extract_runs=RUNS):
    info_h = Z.ZipInfo.load(arc)
    t_arc = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8)).cuda()
    info_d = Z.ZipInfo.load_device(t_arc)
    raw = sum(e.usize for e in info_h.entries)
    got = uz.extract_device(info_d, password=password)
    want = uz.extract(info_h, password=password)
    assert all(bytes(got[nm][:64].cpu().numpy()) == want[nm][:64] and got[nm].numel() == len(want[nm]) for nm in list(want)[::997]), "extract_device differs from extract"
    del got, want
    timing = []

    def dev():
        uz.extract_device(info_d, password=password)
        timing.append(dict(enc.last_timing()))
    w_dev = walls(dev)
    timing = timing[-RUNS:]
    kernels = {k: statistics.median(t[k] for t in timing) for k in timing[0] if not k.startswith("#")}
    w_host = walls(lambda: uz.extract(info_h, password=password), runs=extract_runs, warm=1)
    c = {"entries": len(info_h.entries), "bytes": raw, "archive_bytes": len(arc), "extract_device_ms": med(w_dev), "extract_ms": med(w_host), "kernel_ms": kernels,
         "device_ms": sum(kernels.values()), "extract_device_GBps": raw / statistics.median(w_dev) / 1e6, "extract_GBps": raw / statistics.median(w_host) / 1e6}
    c["faster_than_extract"] = statistics.median(w_dev) < statistics.median(w_host)
    if host_one is not None and password is None:
        w_thr = threads16(info_h, arc, host_one)
        c["threads16_ms"] = med(w_thr)
        c["threads16_GBps"] = raw / statistics.median(w_thr) / 1e6
        c["faster_than_16_threads_within_10pct"] = statistics.median(w_dev) <= statistics.median(w_thr) * 1.10
    res["cases"][name] = c
    dump()
    print("%s: extract_device %.2f ms (%.2f GB/s; kernels %.2f ms), extract %.1f ms (%.2f GB/s)%s" % (
        name, statistics.median(w_dev), c["extract_device_GBps"], c["device_ms"], statistics.median(w_host), c["extract_GBps"],
        ", 16 threads %.1f ms (%.2f GB/s)" % (c["threads16_ms"]["median"], c["threads16_GBps"]) if "threads16_ms" in c else ""), flush=True)
    print("   " + ", ".join("%s %.3f" % kv for kv in kernels.items()), flush=True)
    return t_arc, info_d


if any(c.startswith("small/") for c in cases):
    small = Z.silesia_mix(E * SZ, version=2).tobytes()
    datas = [small[i * SZ:(i + 1) * SZ] for i in range(E)]
    names = ["e%05d.bin" % i for i in range(E)]
    for name, method, pw, one in (("small/deflate", Z.Method.Deflate_3, None, lambda p: zlib.decompress(p, -15)), ("small/deflate_pw", Z.Method.Deflate_3, PW, None),
                                  ("small/bzip2", 14, None, bz2.decompress), ("small/lzma", 18, None, lambda p: lzma_decode(p, 4))):
        if name not in cases:
            continue
        zc = Z.ZipCreate(enc, method)
        zc.add_streams(names, datas, password=pw)
        measure(name, zc.finish(), pw, one)

if "stored_1g" in cases:
    n = 1 << 30
    blob = Z.silesia_mix(64 << 20, version=2).tobytes() * 16
    crc = zlib.crc32(blob)
    nm = b"stored.bin"
    arc = (struct.pack("<4sHHHIIIIHH", b"PK\x03\x04", 20, 0, 0, 0, crc, n, n, len(nm), 0) + nm + blob +
           struct.pack("<4sHHHHIIIIHHHHHII", b"PK\x01\x02", 20, 20, 0, 0, 0, crc, n, n, len(nm), 0, 0, 0, 0, 0, 0) + nm)
    arc += struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, 1, 1, 46 + len(nm), 30 + len(nm) + n, 0)
    del blob
    t_arc, info_d = measure("stored_1g", arc, None, None, extract_runs=3)
    c = res["cases"]["stored_1g"]
    c["store_kernels_GBps"] = n / (c["kernel_ms"]["unzip:k_uz_store"] + c["kernel_ms"].get("unzip:k_uz_fold", 0.0)) / 1e6
    # the one-wave k_inf_crc on a 64 MiB slice of the same bytes: a stored-block stream through zada_inflate_device
    m = 64 << 20
    off = info_d.entries[0].data_offset
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    stream = co.compress(arc[off:off + m]) + co.flush()
    del arc
    t_in = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8)).cuda()
    t_out = torch.empty(m, dtype=torch.uint8, device="cuda")
    one = []
    for _ in range(4):
        ol, used, reg = enc.inflate_device(t_in.data_ptr(), len(stream), t_out.data_ptr(), m)
        one.append(dict(enc.last_timing())["inflate:k_inf_crc"])
    assert ol == m and torch.equal(t_out, t_arc[off:off + m])
    c["k_inf_crc_one_wave_64MiB_ms"] = med(one[1:])
    c["k_inf_crc_one_wave_GBps"] = m / statistics.median(one[1:]) / 1e6
    print("   stored: k_uz_store + k_uz_fold %.2f GB/s; one-wave k_inf_crc on a 64 MiB slice: %.1f ms = %.2f GB/s" % (
        c["store_kernels_GBps"], statistics.median(one[1:]), c["k_inf_crc_one_wave_GBps"]), flush=True)

print(json.dumps(res), flush=True)
dump()
enc.close()
