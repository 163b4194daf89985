"""GPU script: what the batched Inflate gives.  One process; warm-up, then the median of repeated runs; device times from HIP events on
the context's stream (last_timing: k_inflate + k_inf_crc), host-buffer times by the wall clock.
  A. 10 000 entries of 16 KiB of the benchmark corpus (silesia_mix_v2), Deflate_3 streams made by the product: zada_inflate_batch, device time
     and through host buffers, MB/s of uncompressed bytes; against zlib.decompress (.., -15) of the same streams on the same box with one thread
     and with a pool of 16 threads (what a command may use there), each thread looping over a contiguous sixteenth of the entries.
  B. one 64 MiB stream through zada_inflate_device (one wave), against one zlib thread.
Arguments: the JSON file to write (default: standard output only); "A" as a second argument: part A alone (for a profiler run)."""
import json
import os
import statistics
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import ROOT, product

Z = product()
enc = Z.Encoder(0)
only_a = len(sys.argv) > 2 and sys.argv[2] == "A"
res = {"corpus": "silesia_mix_v2"}
try:
    res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
except OSError:
    res["commit"] = None
# (a tree without its history, or one not committed yet: the caller names it -- e. g. "43e6c8e + working tree")
res["commit"] = os.environ.get("ZADA_TREE") or res["commit"]


def med(xs):
    return {"median": statistics.median(xs), "runs": xs}


# ---- A ----
E, SZ, THREADS = 10000, 16384, 16
small = Z.silesia_mix(E * SZ, version=2).tobytes()
datas = [small[i * SZ:(i + 1) * SZ] for i in range(E)]
packed = enc.deflate_batch(datas, Z.Method.Deflate_3)
idx = [i for i, p in enumerate(packed) if p[0] == 0]
streams = [packed[i][1] for i in idx]
sizes = [SZ] * len(idx)
raw_bytes = SZ * len(idx)
res["A"] = {"entries": len(idx), "entry_bytes": SZ, "stream_bytes": sum(len(s) for s in streams)}
for _ in range(2):
    got = enc.inflate_batch(streams, sizes)
assert all(g[0] == 0 and g[1] == datas[i] and g[4] == packed[i][2] for g, i in zip(got, idx)), "inflated bytes differ from the inputs"
dev, wall, k_inf, k_crc = [], [], [], []
for _ in range(9):
    t = time.perf_counter()
    enc.inflate_batch(streams, sizes)
    wall.append((time.perf_counter() - t) * 1e3)
    tm = dict(enc.last_timing())
    k_inf.append(tm["inflate:k_inflate"]); k_crc.append(tm["inflate:k_inf_crc"]); dev.append(tm["inflate:k_inflate"] + tm["inflate:k_inf_crc"])
res["A"]["device_ms"] = med(dev)
res["A"]["k_inflate_ms"] = med(k_inf)
res["A"]["k_inf_crc_ms"] = med(k_crc)
res["A"]["host_buffers_ms"] = med(wall)
res["A"]["device_MBps"] = raw_bytes / statistics.median(dev) / 1e3
res["A"]["host_buffers_MBps"] = raw_bytes / statistics.median(wall) / 1e3
print("A. %d entries of %d bytes: device %.2f ms (k_inflate %.2f + k_inf_crc %.2f) = %.0f MB/s; through host buffers (Python wrapper included) %.1f ms = %.0f MB/s" % (
    len(idx), SZ, statistics.median(dev), statistics.median(k_inf), statistics.median(k_crc), res["A"]["device_MBps"], statistics.median(wall), res["A"]["host_buffers_MBps"]), flush=True)


def zloop(lo, hi):
    n = 0
    for s in streams[lo:hi]:
        n += len(zlib.decompress(s, -15))
    return n


if not only_a:
    one, many = [], []
    for _ in range(5):
        t = time.perf_counter()
        assert zloop(0, len(streams)) == raw_bytes
        one.append((time.perf_counter() - t) * 1e3)
    cuts = [len(streams) * k // THREADS for k in range(THREADS + 1)]
    with ThreadPoolExecutor(THREADS) as pool:
        for _ in range(7):
            t = time.perf_counter()
            assert sum(pool.map(lambda k: zloop(cuts[k], cuts[k + 1]), range(THREADS))) == raw_bytes
            many.append((time.perf_counter() - t) * 1e3)
    many = many[2:]
    res["A"]["zlib_1_thread_ms"] = med(one)
    res["A"]["zlib_16_threads_ms"] = med(many)
    res["A"]["zlib_1_thread_MBps"] = raw_bytes / statistics.median(one) / 1e3
    res["A"]["zlib_16_threads_MBps"] = raw_bytes / statistics.median(many) / 1e3
    res["A"]["device_over_zlib_16_threads"] = res["A"]["device_MBps"] / res["A"]["zlib_16_threads_MBps"]
    res["A"]["condition_met"] = res["A"]["device_MBps"] >= res["A"]["zlib_16_threads_MBps"]
    print("   zlib: one thread %.1f ms = %.0f MB/s; %d threads %.1f ms = %.0f MB/s; device / %d threads = %.1f" % (
        statistics.median(one), res["A"]["zlib_1_thread_MBps"], THREADS, statistics.median(many), res["A"]["zlib_16_threads_MBps"], THREADS,
        res["A"]["device_over_zlib_16_threads"]), flush=True)

    # ---- B ----
    n = 64 << 20
    big = Z.silesia_mix(n, version=2)
    stream, reg = enc.deflate(big.tobytes(), Z.Method.Deflate_3)
    t_in = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    t_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    dev = []
    for k in range(3):                                   # (the first run is the warm-up)
        ol, used, r2 = enc.inflate_device(t_in.data_ptr(), len(stream), t_out.data_ptr(), n)
        tm = dict(enc.last_timing())
        dev.append(tm["inflate:k_inflate"] + tm["inflate:k_inf_crc"])
    assert (ol, used, r2) == (n, len(stream), reg) and bytes(t_out.cpu().numpy()) == big.tobytes(), "the long stream differs"
    dev = dev[1:]
    zt = []
    for _ in range(3):
        t = time.perf_counter()
        assert len(zlib.decompress(stream, -15)) == n
        zt.append((time.perf_counter() - t) * 1e3)
    res["B"] = {"bytes": n, "stream_bytes": len(stream), "device_ms": med(dev), "device_MBps": n / statistics.median(dev) / 1e3,
                "zlib_1_thread_ms": med(zt), "zlib_1_thread_MBps": n / statistics.median(zt) / 1e3}
    print("B. one stream of %d MiB, one wave: %.0f ms = %.1f MB/s; zlib, one thread: %.0f ms = %.0f MB/s" % (
        n >> 20, statistics.median(dev), res["B"]["device_MBps"], statistics.median(zt), res["B"]["zlib_1_thread_MBps"]), flush=True)

print(json.dumps(res), flush=True)
if len(sys.argv) > 1 and sys.argv[1] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
enc.close()
