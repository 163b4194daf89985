"""GPU script: what the Shrink / Reduce / Implode readers give.  One process; warm-up, then the median of 9 runs; device times from
HIP events on the context's stream (last_timing: the marks "unlegacy:*" of the call), host-buffer times by the wall clock.
  A. 10 000 entries each of 6 000 bytes Shrink, 9 000 bytes Reduce_4 (both written by the product's encoders) and 16 KiB Implode (three trees, 8 KiB
     dictionary; written by the tests' imploder -- 500 distinct entries, each twenty times), of the benchmark corpus (silesia_mix_v2):
     zada_unlegacy_batch, device time and through host buffers, MB/s of uncompressed bytes.  Beside it one entry of the batch alone: entries x its
     time / the batch's kernel time is how many entries the device had in flight on average.  Against the logic header on one CPU core (the
     tests' host build, 500 entries) and, where it reads the format, Info-ZIP's unzip on one core (an archive of 500 entries, unzip -tq).
  B. one entry of 1 MiB of each: one stream runs at one wave's pace.
Argument: the JSON file to write (default: standard output only)."""
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _unlegacy as U
from _common import product

Z = product()
enc = Z.Encoder(0)
CUS = torch.cuda.get_device_properties(0).multi_processor_count
res = {"corpus": "silesia_mix_v2", "compute_units": CUS}
KERNEL = {1: "unlegacy:k_unshrink", 5: "unlegacy:k_unreduce", 6: "unlegacy:k_explode"}
RUNS, SAMPLE = 9, 500


def med(xs):
    return {"median": statistics.median(xs), "runs": xs}


def device_ms():
    split = {}
    for name, ms in enc.last_timing():
        if name.startswith("unlegacy:"):
            split[name] = split.get(name, 0.0) + ms
    return sum(split.values()), split


def streams_of(datas, method, flags):
    if method == 1:
        packed = enc.shrink_batch(datas)
    elif method == 5:
        packed = enc.reduce_batch(datas, Z.Method.Reduce_4)
    else:
        some = [U.implode(d, flags) for d in datas[:SAMPLE]]
        return [(datas[k % SAMPLE], some[k % SAMPLE]) for k in range(len(datas))]
    return [(d, s) for d, (rc, s, _) in zip(datas, packed) if rc == 0]


def cpu_figures(pairs, method, flags, row):
    t = time.perf_counter()
    for d, s in pairs[:SAMPLE]:
        assert U.host_decode(method, flags, s, len(d))[0] == 0
    ms = (time.perf_counter() - t) * 1e3
    raw = sum(len(d) for d, _ in pairs[:SAMPLE])
    row.update(logic_header_1_core_MBps=raw / ms / 1e3)
    if method in (1, 6) and shutil.which("unzip"):
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "a.zip")
            with open(p, "wb") as f:
                f.write(U.zip_of([("e%d" % k, s, method, flags, zlib.crc32(d), len(d)) for k, (d, s) in enumerate(pairs[:SAMPLE])]))
            t = time.perf_counter()
            r = subprocess.run(["unzip", "-tq", p], capture_output=True, text=True)
            ms = (time.perf_counter() - t) * 1e3
            assert r.returncode == 0, r.stdout[-300:]
        row.update(unzip_1_core_MBps=raw / ms / 1e3)


for label, method, flags, SZ in (("shrink_6000", 1, 0, 6000), ("reduce4_9000", 5, 0, 9000), ("implode_16k", 6, 6, 16384)):
    E = 10000
    text = Z.silesia_mix(E * SZ, version=2).tobytes()
    pairs = streams_of([text[i * SZ:(i + 1) * SZ] for i in range(E)], method, flags)
    E = len(pairs)                                        # (an entry its encoder does not shrink is stored, and not read here)
    payloads, sizes, raw = [s for _, s in pairs], [len(d) for d, _ in pairs], sum(len(d) for d, _ in pairs)
    for _ in range(2):
        got = enc.unlegacy_batch(payloads, sizes, method, flags)
    assert all(g[0] == 0 and g[1] == d for g, (d, _) in zip(got, pairs)), "decoded bytes differ from the inputs"
    dev, wall, split = [], [], {}
    for _ in range(RUNS):
        t = time.perf_counter()
        enc.unlegacy_batch(payloads, sizes, method, flags)
        wall.append((time.perf_counter() - t) * 1e3)
        d, split = device_ms()
        dev.append(d)
    one = []
    for k in range(RUNS):
        enc.unlegacy_batch(payloads[k * 1000:k * 1000 + 1], sizes[k * 1000:k * 1000 + 1], method, flags)
        one.append(device_ms()[1].get(KERNEL[method], 0.0))
    kern = split.get(KERNEL[method], statistics.median(dev))
    row = {"entries": E, "entry_bytes": SZ, "stream_bytes": sum(len(s) for s in payloads), "device_ms": med(dev), "host_buffers_ms": med(wall), "last_split_ms": split,
           "device_MBps": raw / statistics.median(dev) / 1e3, "host_buffers_MBps": raw / statistics.median(wall) / 1e3, "one_entry_kernel_ms": med(one),
           "entries_in_flight_per_cu": E * statistics.median(one) / kern / CUS}
    cpu_figures(pairs, method, flags, row)
    res[label] = row
    print("A. %s: %d entries: device %.2f ms = %.0f MB/s; through host buffers %.1f ms = %.0f MB/s; one entry alone %.3f ms, %.1f in flight per CU; CPU: %s" % (
        label, E, statistics.median(dev), row["device_MBps"], statistics.median(wall), row["host_buffers_MBps"], statistics.median(one), row["entries_in_flight_per_cu"],
        {k: round(v) for k, v in row.items() if k.endswith("core_MBps")}), flush=True)

n = 1 << 20
big = Z.silesia_mix(n, version=2).tobytes()
for label, method, flags in (("shrink_1mib", 1, 0), ("reduce4_1mib", 5, 0), ("implode_1mib", 6, 6)):
    s = U.encode(big, method) if method != 6 else U.implode(big, flags)
    t_in = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    t_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    dev = []
    for k in range(RUNS + 1):                            # (the first run is the warm-up)
        ol, used, _ = enc.unlegacy_device(t_in.data_ptr(), len(s), t_out.data_ptr(), n, method, flags)
        dev.append(device_ms()[0])
    assert (ol, used) == (n, len(s)) and bytes(t_out.cpu().numpy()) == big, "the long stream differs"
    dev = dev[1:]
    wall = []
    for _ in range(RUNS):
        t = time.perf_counter()
        out = enc.unlegacy(s, n, method, flags)[0]
        wall.append((time.perf_counter() - t) * 1e3)
    assert out == big
    row = {"bytes": n, "stream_bytes": len(s), "device_ms": med(dev), "device_MBps": n / statistics.median(dev) / 1e3, "host_buffers_ms": med(wall),
           "host_buffers_MBps": n / statistics.median(wall) / 1e3}
    cpu_figures([(big, s)], method, flags, row)
    res[label] = row
    print("B. %s: device %.1f ms = %.1f MB/s; through host buffers %.1f ms = %.1f MB/s; CPU: %s" % (
        label, statistics.median(dev), row["device_MBps"], statistics.median(wall), row["host_buffers_MBps"],
        {k: round(v) for k, v in row.items() if k.endswith("core_MBps")}), flush=True)

print(json.dumps(res), flush=True)
if len(sys.argv) > 1 and sys.argv[1] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
enc.close()
