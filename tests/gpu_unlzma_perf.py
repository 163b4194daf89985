"""GPU script: what the LZMA reader gives.  One process; warm-up, then the median of repeated runs; device times from HIP events on
the context's stream (last_timing: the marks "unlzma:*" of the call), host-buffer times by the wall clock.
  A. 10 000 entries of 16 KiB of the benchmark corpus (silesia_mix_v2), LZMA_3 payloads made by the product: zada_unlzma_batch, device time and
     through host buffers, MB/s of uncompressed bytes; against liblzma on the same payloads on the same box with one thread and with a pool of 16
     threads (what a command may use there), each thread looping over a contiguous sixteenth of the entries.  Beside it one entry of the batch
     alone: entries x its time / the batch's time is how many entries the device had in flight on average.
  B. one stream of 8 MiB (argument 3: MiB; written by liblzma, preset 6) through zada_unlzma_device and through host buffers, against one liblzma
     thread: one stream runs at one wave's pace.
Arguments: the JSON file to write (default: standard output only); "A" or "B" as a second argument: that part alone, without liblzma."""
import json
import lzma
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
mib_b = int(sys.argv[3]) if len(sys.argv) > 3 else 8
res = {"corpus": "silesia_mix_v2", "compute_units": torch.cuda.get_device_properties(0).multi_processor_count}
THREADS = 16


def med(xs):
    return {"median": statistics.median(xs), "runs": xs}


def device_ms():
    split = {}
    for name, ms in enc.last_timing():
        if name.startswith("unlzma:"):
            split[name] = split.get(name, 0.0) + ms
    return sum(split.values()), split


def liblzma_decode(p):
    d, ds = p[4], int.from_bytes(p[5:9], "little")
    dec = lzma.LZMADecompressor(lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA1, "dict_size": ds, "lc": d % 9, "lp": (d // 9) % 5, "pb": d // 45}])
    return dec.decompress(p[9:])


if part in ("", "A"):
    E, SZ = 10000, 16384
    small = Z.silesia_mix(E * SZ, version=2).tobytes()
    datas = [small[i * SZ:(i + 1) * SZ] for i in range(E)]
    packed = enc.lzma_batch(datas, Z.Method.LZMA_3)
    payloads = [p[1] for p in packed]
    sizes = [SZ] * E
    raw_bytes = SZ * E
    res["A"] = {"entries": E, "entry_bytes": SZ, "stream_bytes": sum(len(s) for s in payloads)}
    for _ in range(2):
        got = enc.unlzma_batch(payloads, sizes, True)
    assert all(g[0] == 0 and g[1] == d and g[4] == p[2] for g, d, p in zip(got, datas, packed)), "decoded bytes differ from the inputs"
    dev, wall, split = [], [], {}
    for _ in range(7):
        t = time.perf_counter()
        enc.unlzma_batch(payloads, sizes, True)
        wall.append((time.perf_counter() - t) * 1e3)
        d, split = device_ms()
        dev.append(d)
    one_entry = []
    for k in range(7):
        enc.unlzma_batch(payloads[k * 1000:k * 1000 + 1], [SZ], True)
        one_entry.append(device_ms()[1].get("unlzma:k_unlzma", 0.0))
    kern = split.get("unlzma:k_unlzma", statistics.median(dev))
    res["A"].update(device_ms=med(dev), host_buffers_ms=med(wall), last_split_ms=split, device_MBps=raw_bytes / statistics.median(dev) / 1e3,
                    host_buffers_MBps=raw_bytes / statistics.median(wall) / 1e3, one_entry_kernel_ms=med(one_entry),
                    entries_in_flight=E * statistics.median(one_entry) / kern, entries_in_flight_per_cu=E * statistics.median(one_entry) / kern / res["compute_units"])
    print("A. %d entries of %d bytes: device %.2f ms = %.0f MB/s; through host buffers (Python wrapper included) %.1f ms = %.0f MB/s" % (
        E, SZ, statistics.median(dev), res["A"]["device_MBps"], statistics.median(wall), res["A"]["host_buffers_MBps"]), flush=True)
    print("   one entry alone: kernel %.3f ms; entries in flight on average: %.0f = %.1f per CU" % (
        statistics.median(one_entry), res["A"]["entries_in_flight"], res["A"]["entries_in_flight_per_cu"]), flush=True)
    if part == "":
        def loop(lo, hi):
            return sum(len(liblzma_decode(s)) for s in payloads[lo:hi])
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
        res["A"].update(liblzma_1_thread_ms=med(one), liblzma_16_threads_ms=med(many), liblzma_1_thread_MBps=raw_bytes / statistics.median(one) / 1e3,
                        liblzma_16_threads_MBps=raw_bytes / statistics.median(many) / 1e3)
        print("   liblzma: one thread %.0f ms = %.0f MB/s; %d threads %.0f ms = %.0f MB/s" % (
            statistics.median(one), res["A"]["liblzma_1_thread_MBps"], THREADS, statistics.median(many), res["A"]["liblzma_16_threads_MBps"]), flush=True)

if part in ("", "B"):
    n = mib_b << 20
    big = Z.silesia_mix(n, version=2).tobytes()
    c = lzma.LZMACompressor(lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA1, "preset": 6, "dict_size": 1 << 23}])
    payload = bytes([9, 4, 5, 0, 0x5D]) + (1 << 23).to_bytes(4, "little") + c.compress(big) + c.flush()
    t_in = torch.frombuffer(bytearray(payload), dtype=torch.uint8).cuda()
    t_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    dev, split = [], {}
    for k in range(3):                                   # (the first run is the warm-up)
        ol, used, r2 = enc.unlzma_device(t_in.data_ptr(), len(payload), t_out.data_ptr(), n, True)
        d, split = device_ms()
        dev.append(d)
    assert (ol, used) == (n, len(payload)) and bytes(t_out.cpu().numpy()) == big, "the long stream differs"
    dev = dev[1:]
    wall = []
    for _ in range(2):
        t = time.perf_counter()
        out, used, r2 = enc.unlzma(payload, n, True)
        wall.append((time.perf_counter() - t) * 1e3)
    assert out == big
    res["B"] = {"bytes": n, "stream_bytes": len(payload), "device_ms": med(dev), "last_split_ms": split, "device_MBps": n / statistics.median(dev) / 1e3,
                "host_buffers_ms": med(wall), "host_buffers_MBps": n / statistics.median(wall) / 1e3}
    print("B. one stream of %d MiB: device %.0f ms = %.1f MB/s; through host buffers %.0f ms = %.1f MB/s" % (
        mib_b, statistics.median(dev), res["B"]["device_MBps"], statistics.median(wall), res["B"]["host_buffers_MBps"]), flush=True)
    if part == "":
        t = time.perf_counter()
        assert len(liblzma_decode(payload)) == n
        one = (time.perf_counter() - t) * 1e3
        res["B"].update(liblzma_1_thread_ms=one, liblzma_1_thread_MBps=n / one / 1e3)
        print("   liblzma: one thread %.0f ms = %.0f MB/s" % (one, res["B"]["liblzma_1_thread_MBps"]), flush=True)

print(json.dumps(res), flush=True)
if len(sys.argv) > 1 and sys.argv[1] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
enc.close()
