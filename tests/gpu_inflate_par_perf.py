"""GPU script: what the parallel Inflate gives for one large stream, after gpu_inflate_perf.py.  One process; a warm-up run, then the
median of repeated runs.  The figure of a run is the wall clock of the device-resident call, which ends synchronised (every host step of the
method -- the chain, the repairs -- is inside it); the per-kernel split is from HIP events on the context's stream (last_timing).
  B. the 64 MiB Deflate_3 stream of profiles/inflate/NOTES.md B at "inflate_par_chunk_kib" 16 .. 1 024, against one zlib thread in the same run
     and, once, against the parent's path (zada_inflate_device, one wave: about 8 s).
  G. the 1 GiB benchmark stream (silesia_mix_v2 through zada_deflate_device, Deflate_3) at the same chunk sizes, against one zlib thread.
  A. NOTES.md's batch of 10 000 entries of 16 KiB through zada_unzip_device (UnZip.extract_device, test_only) with "inflate_par_min_kib" off and
     at 64: no entry is that large, the batch has to be untouched.
Arguments: the JSON file to write ("-": standard output only), then the parts to run (default: B A G)."""
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import ROOT, product

Z = product()
enc = Z.Encoder(0)
parts = sys.argv[2:] or ["B", "A", "G"]
CHUNKS = (16, 32, 64, 128, 256, 512, 1024)
res = {"corpus": "silesia_mix_v2"}
try:
    res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
except OSError:
    res["commit"] = None
res["commit"] = os.environ.get("ZADA_TREE") or res["commit"]


def med(xs):
    return {"median": statistics.median(xs), "runs": xs}


def sweep(t_z, zl, t_out, n, reg, runs):
    """inflate_par_device at every chunk size -> {chunk_kib: record}"""
    out = {}
    for ck in CHUNKS:
        enc.set_knob("inflate_par_chunk_kib", ck)
        wall, split = [], []
        for k in range(runs + 1):                            # (the first run is the warm-up: it books the workspace)
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = enc.inflate_par_device(t_z.data_ptr(), zl, t_out.data_ptr(), n)
            wall.append((time.perf_counter() - t) * 1e3)
            split.append({k2.split(":")[1]: v for k2, v in enc.last_timing() if k2.startswith("inflate_par:")})
        rec = enc.inflate_par_last()
        assert got == (n, zl, reg) and rec["fell_back"] == 0, (ck, got, rec)
        wall, split = wall[1:], split[1:]
        r = {"wall_ms": med(wall), "MBps": n / statistics.median(wall) / 1e3, "record": rec, "marker_share": rec["marker_bytes"] / n,
             "split_ms": {k2: statistics.median([s.get(k2, 0.0) for s in split]) for k2 in split[0]}}
        out[str(ck)] = r
        print("   chunk %4d KiB: %8.1f ms = %7.0f MB/s; live %d of %d chunks, %d repairs, markers %.0f %%; %s" % (
            ck, r["wall_ms"]["median"], r["MBps"], rec["live_chunks"], rec["chunks"], rec["repairs"], 100 * r["marker_share"],
            ", ".join("%s %.1f" % kv for kv in r["split_ms"].items())), flush=True)
    return out


def one_stream(n, runs, zruns):
    big = Z.silesia_mix(n, version=2)
    t_in = torch.from_numpy(big).cuda()
    t_z = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    t_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, zl, reg = enc.deflate_device(t_in.data_ptr(), n, t_z.data_ptr(), n + 64, Z.Method.Deflate_3)
    assert rc == 0
    r = {"bytes": n, "stream_bytes": zl, "chunks": sweep(t_z, zl, t_out, n, reg, runs)}
    assert torch.equal(t_out, t_in), "the stream read back differs from the input"
    stream = bytes(t_z[:zl].cpu().numpy())
    zt = []
    for _ in range(zruns):
        t = time.perf_counter()
        assert len(zlib.decompress(stream, -15)) == n
        zt.append((time.perf_counter() - t) * 1e3)
    r["zlib_1_thread_ms"] = med(zt)
    r["zlib_1_thread_MBps"] = n / statistics.median(zt) / 1e3
    best = min(r["chunks"], key=lambda ck: r["chunks"][ck]["wall_ms"]["median"])
    r["best_chunk_kib"] = int(best)
    r["best_over_zlib_1_thread"] = r["chunks"][best]["MBps"] / r["zlib_1_thread_MBps"]
    r["bar_met"] = r["best_over_zlib_1_thread"] >= 1.0
    print("   zlib, one thread: %.0f ms = %.0f MB/s; best chunk %s KiB: %.2f x" % (statistics.median(zt), r["zlib_1_thread_MBps"], best, r["best_over_zlib_1_thread"]), flush=True)
    return r, (t_z, zl, t_out, reg)


if "B" in parts:
    print("B. one Deflate_3 stream of 64 MiB", flush=True)
    res["B"], (t_z, zl, t_out, reg) = one_stream(64 << 20, 5, 3)
    t_out.zero_()
    torch.cuda.synchronize()
    t = time.perf_counter()
    got = enc.inflate_device(t_z.data_ptr(), zl, t_out.data_ptr(), 64 << 20)               # the parent's path, once
    res["B"]["one_wave_ms"] = (time.perf_counter() - t) * 1e3
    assert got == (64 << 20, zl, reg)
    print("   zada_inflate_device (one wave), once: %.0f ms" % res["B"]["one_wave_ms"], flush=True)
    del t_z, t_out

if "A" in parts:
    E, SZ = 10000, 16384
    small = Z.silesia_mix(E * SZ, version=2).tobytes()
    zc = Z.ZipCreate(enc, Z.Method.Deflate_3)
    zc.add_streams(["e%05d" % i for i in range(E)], [small[i * SZ:(i + 1) * SZ] for i in range(E)])
    t_arc = torch.from_numpy(np.frombuffer(zc.finish(), dtype=np.uint8).copy()).cuda()
    info = Z.ZipInfo.load_device(t_arc)
    res["A"] = {"entries": E, "entry_bytes": SZ}
    for name, uz in (("knob_off", Z.UnZip(enc)), ("knob_64", Z.UnZip(enc, parallel_inflate=64))):
        wall, dev = [], []
        for k in range(8):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = uz.extract_device(info, test_only=True)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(dict(enc.last_timing()).get("inflate:k_inflate", 0.0))
        assert all(v is None for v in got.values())
        res["A"][name] = {"wall_ms": med(wall[2:]), "k_inflate_ms": med(dev[2:])}
        print("A. %s: extract_device (test_only) of %d entries: %.1f ms by the wall clock, k_inflate %.2f ms" % (
            name, E, statistics.median(wall[2:]), statistics.median(dev[2:])), flush=True)
    res["A"]["parallel_streams"] = enc.inflate_par_last()["streams"]
    del t_arc

if "G" in parts:
    print("G. the 1 GiB benchmark stream", flush=True)
    res["G"], _ = one_stream(1 << 30, 3, 1)

print(json.dumps(res), flush=True)
if len(sys.argv) > 1 and sys.argv[1] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
enc.close()
