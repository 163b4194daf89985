"""GPU script: what writing an archive from device memory into device memory gives.  One process; warm-up, then the median of 9 runs;
wall clock around ZipCreate.write_device with the input tensors resident (the call synchronises), device times per kernel from HIP events on the
context's stream (last_timing: the launches of all groups of the call, equal names added up).
  small16k: 10 000 entries of 16 KiB of the benchmark corpus (silesia_mix_v2), Deflate_3;  mid256k: 2 000 entries of 256 KiB, Deflate_3;
  stored_1g: one stored entry of 1 GiB.
Per case: write_device; ZipCreate.add_streams + finish from host bytes on the same build (the host-pointer path: the yardstick); zada_deflate_batch
alone (Store: zlib.crc32 of the bytes, what add_streams does for Store); sixteen host threads of zlib level 6 over the entries, each thread a contiguous
sixteenth.  For k_zw_pack, k_zw_place (and k_uz_store + k_uz_fold for the stored gigabyte) the GB/s of the bytes they read, which they also write.
Arguments: the JSON file to write (default: standard output only); a second argument names the cases, comma-separated."""
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import product

Z = product()
enc = Z.Encoder(0)
THREADS, RUNS = 16, 9
cases = sys.argv[2].split(",") if len(sys.argv) > 2 else ["small16k", "mid256k", "stored_1g"]
res = {"corpus": "silesia_mix_v2", "runs": RUNS, "cases": {}}


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


def measure(name, method, datas, host_runs=RUNS):
    names = ["e%05d.bin" % i for i in range(len(datas))]
    raw = sum(len(d) for d in datas)
    arena = torch.from_numpy(np.frombuffer(b"".join(datas), dtype=np.uint8)).cuda()
    tensors = list(arena.split([len(d) for d in datas]))
    zc = Z.ZipCreate(enc, method)
    zc.add_streams(names, datas)
    cd_off = len(zc.buf)                                  # where the central directory begins
    want = zc.finish()
    got = Z.ZipCreate(enc, method).write_device(names, tensors)
    assert got.numel() == len(want) and bytes(got[:4096].cpu().numpy()) == want[:4096] and bytes(got[-4096:].cpu().numpy()) == want[-4096:], "write_device differs from add_streams + finish"
    del got
    timing = []

    def dev():
        Z.ZipCreate(enc, method).write_device(names, tensors)
        timing.append(dict(enc.last_timing()))
    w_dev = walls(dev)
    timing = timing[-RUNS:]
    kernels = {k: statistics.median(t[k] for t in timing) for k in timing[0] if not k.startswith("#")}

    def host():
        z = Z.ZipCreate(enc, method)
        z.add_streams(names, datas)
        z.finish()
    w_host = walls(host, runs=host_runs, warm=1)
    w_batch = walls((lambda: [zlib.crc32(d) for d in datas]) if method == Z.Method.Store else (lambda: enc.deflate_batch(datas, method)), runs=host_runs, warm=1)
    pieces = datas if len(datas) >= THREADS else [datas[0][len(datas[0]) * k // THREADS:len(datas[0]) * (k + 1) // THREADS] for k in range(THREADS)]
    cuts = [len(pieces) * k // THREADS for k in range(THREADS + 1)]
    with ThreadPoolExecutor(THREADS) as pool:
        w_thr = walls(lambda: list(pool.map(lambda k: [zlib.compress(p, 6) for p in pieces[cuts[k]:cuts[k + 1]]], range(THREADS))), runs=5, warm=1)
    c = {"entries": len(datas), "bytes": raw, "archive_bytes": len(want), "write_device_ms": med(w_dev), "add_streams_finish_ms": med(w_host), "batch_alone_ms": med(w_batch),
         "threads16_zlib6_ms": med(w_thr), "kernel_ms": kernels, "device_ms": sum(kernels.values()),
         "faster_than_host_path": statistics.median(w_dev) < statistics.median(w_host)}
    # (k_zw_place moves the local headers, their Zip64 extensions too, and the payloads: all that lies in front of the directory)
    moved = {"zip:k_zw_pack": raw, "zip:k_zw_place": cd_off if method != Z.Method.Store else None,
             "unzip:k_uz_store": raw if method == Z.Method.Store else None}
    c["kernel_GBps"] = {k: v / kernels[k] / 1e6 for k, v in moved.items() if v and k in kernels and kernels[k] > 0}
    if method == Z.Method.Store and "unzip:k_uz_store" in kernels:
        c["kernel_GBps"]["k_uz_store+k_uz_fold"] = raw / (kernels["unzip:k_uz_store"] + kernels.get("unzip:k_uz_fold", 0.0)) / 1e6
    res["cases"][name] = c
    dump()
    print("%s: write_device %.2f ms (kernels %.2f ms), add_streams + finish %.1f ms, batch alone %.1f ms, 16 zlib threads %.1f ms" % (
        name, statistics.median(w_dev), c["device_ms"], statistics.median(w_host), statistics.median(w_batch), statistics.median(w_thr)), flush=True)
    print("   " + ", ".join("%s %.3f" % kv for kv in kernels.items()), flush=True)
    print("   GB/s: " + ", ".join("%s %.1f" % kv for kv in c["kernel_GBps"].items()), flush=True)


if "small16k" in cases:
    blob = Z.silesia_mix(10000 * 16384, version=2).tobytes()
    measure("small16k", Z.Method.Deflate_3, [blob[i * 16384:(i + 1) * 16384] for i in range(10000)])
if "mid256k" in cases:
    blob = Z.silesia_mix(2000 * 262144, version=2).tobytes()
    measure("mid256k", Z.Method.Deflate_3, [blob[i * 262144:(i + 1) * 262144] for i in range(2000)], host_runs=5)
if "stored_1g" in cases:
    blob = Z.silesia_mix(64 << 20, version=2).tobytes() * 16
    measure("stored_1g", Z.Method.Store, [blob], host_runs=3)
print(json.dumps(res), flush=True)
dump()
enc.close()
