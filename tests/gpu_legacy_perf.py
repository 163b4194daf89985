"""GPU script: what Shrink_1 and Reduce_4 give on the device.  One process; one warm-up, then nine runs, medians; device time per
kernel from HIP events on the context's stream (last_timing), the calls through host buffers by the wall clock (Python wrapper included).  The
yardstick is the CPU models' closed forms (tests/legacy/) on one core of the same box: there is no other encoder of these methods here.
  A. 10 000 entries of 6 000 bytes, Shrink_1 (zada_shrink_batch): the sizes `rezip` sends to these methods.
  B. 10 000 entries of 9 000 bytes, Reduce_4 (zada_reduce_batch); the share of k_reduce_lz in the device time.
  C. one entry of 1 MiB through each: one stream runs at one wave's pace.
  D. entries in flight per CU: the kernel time of 256 x k equal entries for k = 1 .. 6 -- it steps up where a CU has to take a second round.
The model runs over a sample of B's entries (argument 2, default 500) and is scaled to the batch; over everything else in full.
Arguments: the JSON file to write (default: standard output only)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _legacy as L
from _common import product

Z = product()
enc = Z.Encoder(0)
SAMPLE = int(sys.argv[2]) if len(sys.argv) > 2 else 500
RUNS = 9
res = {"corpus": "silesia_mix_v2", "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "runs": RUNS}


def med(xs):
    return {"median": statistics.median(xs), "runs": xs}


def kernels():
    split = {}
    for name, ms in enc.last_timing():
        if not name.startswith("#"):
            split[name] = split.get(name, 0.0) + ms
    return split


def timed(fn):
    """one warm-up, RUNS runs -> (wall ms per run, device ms per run, per-kernel medians)"""
    fn()
    wall, dev, per = [], [], {}
    for _ in range(RUNS):
        t = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t) * 1e3)
        k = kernels()
        dev.append(sum(k.values()))
        for name, ms in k.items():
            per.setdefault(name, []).append(ms)
    return wall, dev, {k: statistics.median(v) for k, v in per.items()}


def report(tag, what, nbytes, wall, dev, per, model_ms, extra=None):
    r = {"what": what, "bytes": nbytes, "host_buffers_ms": med(wall), "device_ms": med(dev), "kernel_ms": per, "model_one_core_ms": model_ms,
         "device_MBps": nbytes / statistics.median(dev) / 1e3, "host_buffers_MBps": nbytes / statistics.median(wall) / 1e3, "model_MBps": nbytes / model_ms / 1e3}
    r.update(extra or {})
    res[tag] = r
    print("%s. %s: device %.1f ms = %.1f MB/s; through host buffers %.1f ms = %.1f MB/s; model on one core %.0f ms = %.1f MB/s" % (
        tag, what, statistics.median(dev), r["device_MBps"], statistics.median(wall), r["host_buffers_MBps"], model_ms, r["model_MBps"]), flush=True)
    print("   kernels: " + ", ".join("%s %.2f" % kv for kv in sorted(per.items())), flush=True)


def model_ms(fn, datas):
    t = time.perf_counter()
    for d in datas:
        fn(d)
    return (time.perf_counter() - t) * 1e3


E = 10000
corpus = Z.silesia_mix(E * 9000, version=2).tobytes()

# A
datas = [corpus[i * 6000:(i + 1) * 6000] for i in range(E)]
got = enc.shrink_batch(datas)
assert all(g == ((r, s if r == 0 else None, c)) for g, (r, s, c) in zip(got[:200], (L.model_result(d, 1) for d in datas[:200]))), "Shrink batch differs from the model"
wall, dev, per = timed(lambda: enc.shrink_batch(datas))
report("A", "%d entries of 6 000 bytes, Shrink_1" % E, E * 6000, wall, dev, per, model_ms(lambda d: L.shrink(d), datas),
       {"stream_bytes": sum(len(g[1]) for g in got if g[0] == 0), "stored": sum(1 for g in got if g[0])})

# B
datas = [corpus[i * 9000:(i + 1) * 9000] for i in range(E)]
got = enc.reduce_batch(datas, 5)
assert all(g == ((r, s if r == 0 else None, c)) for g, (r, s, c) in zip(got[:200], (L.model_result(d, 5) for d in datas[:200]))), "Reduce batch differs from the model"
wall, dev, per = timed(lambda: enc.reduce_batch(datas, 5))
sample = datas[::max(1, E // SAMPLE)]
report("B", "%d entries of 9 000 bytes, Reduce_4" % E, E * 9000, wall, dev, per, model_ms(lambda d: L.reduce(d, 4), sample) * E / len(sample),
       {"stream_bytes": sum(len(g[1]) for g in got if g[0] == 0), "stored": sum(1 for g in got if g[0]), "model_sample": len(sample),
        "k_reduce_lz_share": per.get("k_reduce_lz", 0.0) / max(sum(per.values()), 1e-9)})
print("   share of k_reduce_lz in the device time: %.1f %%" % (100 * res["B"]["k_reduce_lz_share"]), flush=True)

# C
big = corpus[:1 << 20]
for tag, name, fn, mfn in (("C1", "Shrink_1", lambda: enc.shrink(big), lambda d: L.shrink(d)), ("C2", "Reduce_4", lambda: enc.reduce(big, 5), lambda d: L.reduce(d, 4))):
    wall, dev, per = timed(fn)
    report(tag, "one entry of 1 MiB, %s" % name, len(big), wall, dev, per, model_ms(mfn, [big]))

# D
one = corpus[:6000]
steps = {}
for name, fn, kern in (("Shrink_1", lambda ds: enc.shrink_batch(ds), "k_shrink"), ("Reduce_4", lambda ds: enc.reduce_batch(ds, 5), "k_reduce_lz")):
    row = []
    for k in range(1, 7):
        ds = [one] * (res["compute_units"] * k)
        fn(ds)
        t = []
        for _ in range(3):
            fn(ds)
            t.append(kernels().get(kern, 0.0))
        row.append(statistics.median(t))
    steps[name] = row
    per_cu = max(k + 1 for k in range(6) if row[k] < 1.5 * row[0])
    print("D. %s: %s ms for 1 .. 6 entries per CU: %s -> %d in flight per CU" % (name, kern, ", ".join("%.2f" % x for x in row), per_cu), flush=True)
    steps[name + "_in_flight_per_cu"] = per_cu
res["D"] = steps

print(json.dumps(res), flush=True)
if len(sys.argv) > 1 and sys.argv[1] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
enc.close()
