"""GPU script: what the knob "zip_legacy" gives.  One process; one warm-up, then the median of 9 runs; wall clock around the Python
calls with the input tensors resident (the calls synchronise), device times per kernel from HIP events on the context's stream (last_timing: the
launches of all groups of the call, equal names added up).  The batches are those of profiles/legacy/NOTES.md (silesia_mix_v2):
  shrink_1    10 000 entries of 6 000 bytes, ZipCreate (Shrink_1).write_device_ex (legacy=True) against add_streams + finish from host bytes
  reduce_4    10 000 entries of 9 000 bytes, the same under Reduce_4
  rezip       ReZip (legacy=True).rezip_device of 10 000 stored entries of 4 KiB with all twelve approaches against the default ten
write_device_ex must equal add_streams + finish.  There is no threshold: the figures go into profiles/zip_legacy/NOTES.md, also where the device
path is no faster.
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
CASES = {"shrink_1": (Z.Method.Shrink_1, 6000), "reduce_4": (Z.Method.Reduce_4, 9000), "rezip": (None, 4096)}
cases = sys.argv[2].split(",") if len(sys.argv) > 2 and sys.argv[2] else list(CASES)
COUNT = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
RUNS = int(sys.argv[4]) if len(sys.argv) > 4 else 9
res = {"corpus": "silesia_mix_v2", "runs": RUNS, "entries": COUNT, "cases": {}}


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


def kernels_of(timing):
    return {k: statistics.median(t.get(k, 0.0) for t in timing) for k in timing[0] if not k.startswith("#")}


for name in cases:
    method, nbytes = CASES[name]
    blob = Z.silesia_mix(COUNT * nbytes, version=2).tobytes()
    datas = [blob[i * nbytes:(i + 1) * nbytes] for i in range(COUNT)]
    names = ["e%05d.bin" % i for i in range(COUNT)]
    timing = []
    if method is not None:
        arena = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8)).cuda()
        tensors = list(arena.split([len(d) for d in datas]))
        zc = Z.ZipCreate(enc, method)
        zc.add_streams(names, datas)
        want = zc.finish()
        got = bytes(Z.ZipCreate(enc, method).write_device_ex(names, tensors, legacy=True).cpu().numpy())
        assert got == want, "%s: write_device_ex differs from add_streams + finish" % name

        def dev():
            Z.ZipCreate(enc, method).write_device_ex(names, tensors, legacy=True)
            timing.append(dict(enc.last_timing()))

        def host():
            z = Z.ZipCreate(enc, method)
            z.add_streams(names, datas)
            z.finish()
        w_dev = walls(dev, RUNS, 1)
        kernels = kernels_of(timing[-RUNS:])
        w_host = walls(host, RUNS, 1)
        stored = sum(1 for e in zc.entries if e["zip_type"] == 0)
        c = {"entry_bytes": nbytes, "archive_bytes": len(want), "stored": stored, "write_device_ex_ms": med(w_dev), "add_streams_finish_ms": med(w_host), "kernel_ms": kernels,
             "device_ms": sum(kernels.values()), "faster_than_host_path": statistics.median(w_dev) < statistics.median(w_host)}
        print("%s: write_device_ex %.2f ms (launch phases %.2f ms), add_streams + finish %.2f ms; %d of %d entries stored" %
              (name, statistics.median(w_dev), c["device_ms"], statistics.median(w_host), stored, COUNT), flush=True)
    else:
        zc = Z.ZipCreate(enc, Z.Method.Store)
        zc.add_streams(names, datas)
        src = torch.from_numpy(np.frombuffer(zc.finish(), dtype=np.uint8).copy()).cuda()
        info = Z.ZipInfo.load_device(src)
        c = {"entry_bytes": nbytes, "source_bytes": src.numel()}
        for label, rz in (("twelve", Z.ReZip(enc, legacy=True)), ("ten", Z.ReZip(enc))):
            out, rep = rz.rezip_device(info, report=True)
            timing.clear()

            def run():
                rz.rezip_device(info)
                timing.append(dict(enc.last_timing()))
            w = walls(run, RUNS, 1)
            kernels = kernels_of(timing[-RUNS:])
            c[label] = {"rezip_device_ms": med(w), "kernel_ms": kernels, "device_ms": sum(kernels.values()), "archive_bytes": out.numel(),
                        "wins": {a: v["count"] for a, v in rep["totals"].items() if v["count"]}}
            print("rezip, %s approaches: %.1f ms (launch phases %.1f ms), archive %d bytes, wins %r" % (label, statistics.median(w), c[label]["device_ms"], out.numel(), c[label]["wins"]),
                  flush=True)
    res["cases"][name] = c
    dump()
    print("   " + ", ".join("%s %.3f" % kv for kv in sorted(kernels.items(), key=lambda kv: -kv[1])[:12]), flush=True)
print(json.dumps(res), flush=True)
dump()
enc.close()
