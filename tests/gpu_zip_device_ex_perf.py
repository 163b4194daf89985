"""GPU script: what zada_zip_device_ex gives for the methods and the passwords zada_zip_device does not take.  One process; warm-up,
then the median of 9 runs; wall clock around ZipCreate.write_device_ex with the input tensors resident (the call synchronises), device times per
kernel from HIP events on the context's stream (last_timing: the launches of all groups of the call, equal names added up).
  10 000 entries of 16 KiB of the benchmark corpus (silesia_mix_v2) for BZip2_3, LZMA_2, LZMA_3, Preselection_2 (names cycling .txt, .c, .bin, .png)
  and Deflate_3 with a password.
Per case: write_device_ex against ZipCreate.add_streams + finish from host bytes on the same build (the host-pointer path: the yardstick), whose
archive it must equal.  There is no threshold: the figures go into profiles/zip_device/NOTES.md.
Arguments: the JSON file to write (default: standard output only); a second argument names the cases, comma-separated; a third the number of entries
(default 10 000) and a fourth the number of measured runs (default 9)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import product

Z = product()
enc = Z.Encoder(0)
CASES = {"bzip2_3": (Z.Method.BZip2_3, None), "lzma_2": (Z.Method.LZMA_2, None), "lzma_3": (Z.Method.LZMA_3, None), "presel_2": (Z.Method.Preselection_2, None),
         "deflate_3_pw": (Z.Method.Deflate_3, "measure")}
cases = sys.argv[2].split(",") if len(sys.argv) > 2 and sys.argv[2] else list(CASES)
COUNT = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
RUNS = int(sys.argv[4]) if len(sys.argv) > 4 else 9
res = {"corpus": "silesia_mix_v2", "runs": RUNS, "entries": COUNT, "entry_bytes": 16384, "cases": {}}


def dump():
    if len(sys.argv) > 1 and sys.argv[1] != "-":
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


def med(xs):
    return {"median": statistics.median(xs), "runs": xs}


def walls(fn, runs, warm):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


blob = Z.silesia_mix(COUNT * 16384, version=2).tobytes()
datas = [blob[i * 16384:(i + 1) * 16384] for i in range(COUNT)]
arena = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8)).cuda()
tensors = list(arena.split([len(d) for d in datas]))
headers = [bytes((i + j) % 256 for j in range(11)) for i in range(COUNT)]
for name in cases:
    method, pw = CASES[name]
    ext = ("txt", "c", "bin", "png") if name == "presel_2" else ("bin",)
    names = ["e%05d.%s" % (i, ext[i % len(ext)]) for i in range(COUNT)]
    kw = dict(password=pw, _headers=headers) if pw else {}
    zc = Z.ZipCreate(enc, method)
    zc.add_streams(names, datas, **kw)
    want = zc.finish()
    got = bytes(Z.ZipCreate(enc, method).write_device_ex(names, tensors, **kw).cpu().numpy())
    assert got == want, "%s: write_device_ex differs from add_streams + finish" % name
    timing = []

    def dev():
        Z.ZipCreate(enc, method).write_device_ex(names, tensors, **kw)
        timing.append(dict(enc.last_timing()))

    def host():
        z = Z.ZipCreate(enc, method)
        z.add_streams(names, datas, **kw)
        z.finish()
    w_dev = walls(dev, RUNS, 1)
    timing = timing[-RUNS:]
    kernels = {k: statistics.median(t.get(k, 0.0) for t in timing) for k in timing[0] if not k.startswith("#")}
    w_host = walls(host, RUNS, 1)
    c = {"archive_bytes": len(want), "write_device_ex_ms": med(w_dev), "add_streams_finish_ms": med(w_host), "kernel_ms": kernels, "device_ms": sum(kernels.values()),
         "faster_than_host_path": statistics.median(w_dev) < statistics.median(w_host)}
    res["cases"][name] = c
    dump()
    print("%s: write_device_ex %.2f ms (launch phases %.2f ms), add_streams + finish %.1f ms" % (name, statistics.median(w_dev), c["device_ms"], statistics.median(w_host)), flush=True)
    print("   " + ", ".join("%s %.3f" % kv for kv in sorted(kernels.items(), key=lambda kv: -kv[1])[:12]), flush=True)
print(json.dumps(res), flush=True)
dump()
enc.close()
