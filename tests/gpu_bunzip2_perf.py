"""GPU script: what the BZip2 reader gives.  One process; warm-up, then the median of repeated runs; device times from HIP events on
the context's stream (last_timing: every mark of the call from "bunzip2:begin" on, the host's chain resolve between the launches included),
host-buffer times by the wall clock.
  A. 10 000 entries of 16 KiB of the benchmark corpus (silesia_mix_v2), BZip2_3 streams made by the product: zada_bunzip2_batch, device time and
     through host buffers, MB/s of uncompressed bytes; against bz2.decompress of the same streams on the same box with one thread and with a pool
     of 16 threads (what a command may use there), each thread looping over a contiguous sixteenth of the entries.
  B. one BZip2_3 stream of 256 MiB (argument 3: MiB) through zada_bunzip2_device and through host buffers, against one bz2 thread -- and against 16
     threads that each decode the same stream at once (libbz2 cannot cut one stream: that is the box's rate at this block size).
Arguments: the JSON file to write (default: standard output only); "A" or "B" as a second argument: that part alone, without libbz2 (for a profiler run)."""
import bz2
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import product

Z = product()
enc = Z.Encoder(0)
part = sys.argv[2] if len(sys.argv) > 2 else ""
mib_b = int(sys.argv[3]) if len(sys.argv) > 3 else 256
res = {"corpus": "silesia_mix_v2", "commit": os.environ.get("ZADA_TREE")}
THREADS = 16


def med(xs):
    return {"median": statistics.median(xs), "runs": xs}


def device_ms():
    split = {}
    for name, ms in enc.last_timing():
        if name.startswith("bunzip2:"):
            split[name] = split.get(name, 0.0) + ms
    return sum(split.values()), split


if part in ("", "A"):
    E, SZ = 10000, 16384
    small = Z.silesia_mix(E * SZ, version=2).tobytes()
    datas = [small[i * SZ:(i + 1) * SZ] for i in range(E)]
    packed = enc.bzip2_batch(datas, Z.Method.BZip2_3)
    assert all(p[0] in (0, 1) and p[1] is not None for p in packed)
    streams = [p[1] for p in packed]
    sizes = [SZ] * E
    raw_bytes = SZ * E
    res["A"] = {"entries": E, "entry_bytes": SZ, "stream_bytes": sum(len(s) for s in streams)}
    for _ in range(2):
        got = enc.bunzip2_batch(streams, sizes)
    assert all(g[0] == 0 and g[1] == d and g[4] == p[2] for g, d, p in zip(got, datas, packed)), "decoded bytes differ from the inputs"
    dev, wall, split = [], [], {}
    for _ in range(7):
        t = time.perf_counter()
        enc.bunzip2_batch(streams, sizes)
        wall.append((time.perf_counter() - t) * 1e3)
        d, split = device_ms()
        dev.append(d)
    res["A"].update(device_ms=med(dev), host_buffers_ms=med(wall), last_split_ms=split, device_MBps=raw_bytes / statistics.median(dev) / 1e3,
                    host_buffers_MBps=raw_bytes / statistics.median(wall) / 1e3)
    print("A. %d entries of %d bytes: device %.2f ms = %.0f MB/s; through host buffers (Python wrapper included) %.1f ms = %.0f MB/s" % (
        E, SZ, statistics.median(dev), res["A"]["device_MBps"], statistics.median(wall), res["A"]["host_buffers_MBps"]), flush=True)
    if part == "":
        def loop(lo, hi):
            return sum(len(bz2.decompress(s)) for s in streams[lo:hi])
        one, many = [], []
        for _ in range(3):
            t = time.perf_counter()
            assert loop(0, E) == raw_bytes
            one.append((time.perf_counter() - t) * 1e3)
        cuts = [E * k // THREADS for k in range(THREADS + 1)]
        with ThreadPoolExecutor(THREADS) as pool:
            for _ in range(5):
                t = time.perf_counter()
                assert sum(pool.map(lambda k: loop(cuts[k], cuts[k + 1]), range(THREADS))) == raw_bytes
                many.append((time.perf_counter() - t) * 1e3)
        many = many[1:]
        res["A"].update(bz2_1_thread_ms=med(one), bz2_16_threads_ms=med(many), bz2_1_thread_MBps=raw_bytes / statistics.median(one) / 1e3,
                        bz2_16_threads_MBps=raw_bytes / statistics.median(many) / 1e3)
        res["A"]["condition_met"] = res["A"]["device_MBps"] >= res["A"]["bz2_16_threads_MBps"]
        print("   libbz2: one thread %.0f ms = %.0f MB/s; %d threads %.0f ms = %.0f MB/s" % (
            statistics.median(one), res["A"]["bz2_1_thread_MBps"], THREADS, statistics.median(many), res["A"]["bz2_16_threads_MBps"]), flush=True)

if part in ("", "B"):
    n = mib_b << 20
    big = Z.silesia_mix(n, version=2).tobytes()
    rc, stream, reg = enc.bzip2(big, Z.Method.BZip2_3)
    assert rc == 0
    t_in = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    t_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    dev, split = [], {}
    for k in range(4):                                   # (the first run is the warm-up)
        ol, used, r2 = enc.bunzip2_device(t_in.data_ptr(), len(stream), t_out.data_ptr(), n)
        d, split = device_ms()
        dev.append(d)
    assert (ol, used, r2) == (n, len(stream), reg) and bytes(t_out.cpu().numpy()) == big, "the long stream differs"
    dev = dev[1:]
    wall = []
    for _ in range(2):
        t = time.perf_counter()
        out, used, r2 = enc.bunzip2(stream, n)
        wall.append((time.perf_counter() - t) * 1e3)
    assert out == big
    res["B"] = {"bytes": n, "stream_bytes": len(stream), "blocks": len(enc.bunzip2_last_records(blocks=True)), "device_ms": med(dev), "last_split_ms": split,
                "device_MBps": n / statistics.median(dev) / 1e3, "host_buffers_ms": med(wall), "host_buffers_MBps": n / statistics.median(wall) / 1e3}
    print("B. one stream of %d MiB, %d blocks: device %.0f ms = %.0f MB/s; through host buffers %.0f ms = %.0f MB/s" % (
        mib_b, res["B"]["blocks"], statistics.median(dev), res["B"]["device_MBps"], statistics.median(wall), res["B"]["host_buffers_MBps"]), flush=True)
    if part == "":
        t = time.perf_counter()
        assert len(bz2.decompress(stream)) == n
        one = (time.perf_counter() - t) * 1e3
        with ThreadPoolExecutor(THREADS) as pool:
            t = time.perf_counter()
            assert sum(pool.map(lambda k: len(bz2.decompress(stream)), range(THREADS))) == n * THREADS
            many = (time.perf_counter() - t) * 1e3
        res["B"].update(bz2_1_thread_ms=one, bz2_1_thread_MBps=n / one / 1e3, bz2_16_threads_same_stream_ms=many, bz2_16_threads_MBps=n * THREADS / many / 1e3)
        res["B"]["condition_met"] = res["B"]["device_MBps"] >= res["B"]["bz2_16_threads_MBps"]
        print("   libbz2: one thread %.0f ms = %.0f MB/s; %d threads, the same stream each, %.0f ms = %.0f MB/s" % (
            one, res["B"]["bz2_1_thread_MBps"], THREADS, many, res["B"]["bz2_16_threads_MBps"]), flush=True)

print(json.dumps(res), flush=True)
if len(sys.argv) > 1 and sys.argv[1] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
enc.close()
