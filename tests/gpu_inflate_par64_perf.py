"""GPU script: what the parallel Inflate gives for one large Deflate64 stream (the knob "inflate_par_deflate64"), after
gpu_inflate_par_perf.py.  One process; a warm-up run, then the median of 5 runs; the figure of a run is the wall clock of the device-resident call,
which ends synchronised.
  The stream: the non-final blocks of _deflate64.py's period_49152 M times, joined at bit level, and a final empty fixed block: every block is a
  true block start and the output is M copies of what those blocks make, about 64 MiB.  The CPU models confirm the construction at M = 3.
  D. zada_inflate_par_device (format 9, knob 1) at "inflate_par_chunk_kib" 16 / 64 / 256 against zada_inflate_device (format 9, one wave: the
     path such a stream takes without the knob) on the same stream.
  E. for scale: the Deflate parallel path (format 8) on zlib's level 6 stream of the same bytes, at the same chunk sizes.
Arguments: the JSON file to write ("-": standard output only)."""
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
import _deflate64 as D
import _inflate_par64 as P
from _common import ROOT, product
from _inflate import model_inflate

Z = product()
enc = Z.Encoder(0)
CHUNKS = (16, 64, 256)
RUNS = 5
res = {"input": "period_49152 (tests/_deflate64.py), its non-final blocks repeated"}
try:
    res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
except OSError:
    res["commit"] = None
res["commit"] = os.environ.get("ZADA_TREE") or res["commit"]


def repeated(m):
    """-> (the stream of m copies, the bytes it makes)"""
    data, stream, _, info = D.streams()["period_49152"]
    e, made = info["block_bits"][-2], info["block_out"][-2]          # where the final block begins
    piece = int.from_bytes(stream, "little") & ((1 << e) - 1)
    acc = 0
    for k in range(m):
        acc |= piece << (k * e)
    acc |= 0b011 << (m * e)                                          # BFINAL = 1, BTYPE = 01, the end-of-block code: seven zero bits
    return acc.to_bytes((m * e + 10 + 7) // 8, "little"), data[:made] * m


def med(xs):
    return {"median": statistics.median(xs), "runs": xs}


def timed(fn):
    wall = []
    for _ in range(RUNS + 1):                                        # (the first run is the warm-up: it books the workspace)
        torch.cuda.synchronize()
        t = time.perf_counter()
        got = fn()
        wall.append((time.perf_counter() - t) * 1e3)
    return got, wall[1:]


def sweep(fmt, t_z, zl, t_out, n, want, must_run_parallel):
    out = {}
    for ck in CHUNKS:
        enc.set_knob("inflate_par_chunk_kib", ck)
        t_out.zero_()
        got, wall = timed(lambda: enc.inflate_par_device(t_z.data_ptr(), zl, t_out.data_ptr(), n, format=fmt))
        rec = enc.inflate_par_last()
        assert got[:2] == (n, zl) and torch.equal(t_out, want) and not (must_run_parallel and rec["fell_back"]), (fmt, ck, got, rec)
        split = {k.split(":")[1]: v for k, v in enc.last_timing() if k.startswith("inflate_par:")}
        out[str(ck)] = {"wall_ms": med(wall), "MBps": n / statistics.median(wall) / 1e3, "record": rec, "marker_share": rec["marker_bytes"] / n, "split_ms_last_run": split}
        print("   format %d, chunk %4d KiB: %8.1f ms = %7.0f MB/s; fell back %d; live %d of %d chunks, %d repairs, markers %.0f %%; %s" % (
            fmt, ck, statistics.median(wall), out[str(ck)]["MBps"], rec["fell_back"], rec["live_chunks"], rec["chunks"], rec["repairs"], 100 * out[str(ck)]["marker_share"],
            ", ".join("%s %.1f" % kv for kv in split.items())), flush=True)
    return out


# the construction, on the CPU models at a small M
s3, d3 = repeated(3)
assert model_inflate(s3, len(d3), 9)[:4] == (0, d3, len(d3), len(s3))
g3 = P.model_inflate_par64(s3, len(d3), 16)
assert g3[:2] == (0, d3) and g3[6]["fell_back"] == 0, g3[6]

M = -(-(64 << 20) // (len(d3) // 3))
stream, data = repeated(M)
n, zl = len(data), len(stream)
res.update(copies=M, bytes=n, stream_bytes=zl)
print("D. one Deflate64 stream: %d copies, %d bytes of output, %d bytes of stream" % (M, n, zl), flush=True)
want = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
t_z = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
t_out = torch.empty(n, dtype=torch.uint8, device="cuda")
enc.set_knob("inflate_par_deflate64", 1)
res["D"] = {"chunks": sweep(9, t_z, zl, t_out, n, want, True)}
enc.set_knob("inflate_par_deflate64", 0)
t_out.zero_()
got, wall = timed(lambda: enc.inflate_device(t_z.data_ptr(), zl, t_out.data_ptr(), n, format=9))
assert got[:2] == (n, zl) and torch.equal(t_out, want)
res["D"]["one_wave"] = {"wall_ms": med(wall), "MBps": n / statistics.median(wall) / 1e3}
best = min(res["D"]["chunks"], key=lambda ck: res["D"]["chunks"][ck]["wall_ms"]["median"])
res["D"]["best_chunk_kib"] = int(best)
res["D"]["best_over_one_wave"] = statistics.median(wall) / res["D"]["chunks"][best]["wall_ms"]["median"]
print("   zada_inflate_device (format 9, one wave): %.0f ms = %.1f MB/s; the parallel path at %s KiB: %.1f x" % (
    statistics.median(wall), res["D"]["one_wave"]["MBps"], best, res["D"]["best_over_one_wave"]), flush=True)

zs = zlib.compressobj(6, zlib.DEFLATED, -15)
zstream = zs.compress(data) + zs.flush()
print("E. zlib's level 6 stream of the same bytes: %d bytes of stream" % len(zstream), flush=True)
t_z = torch.from_numpy(np.frombuffer(zstream, dtype=np.uint8).copy()).cuda()
res["E"] = {"stream_bytes": len(zstream), "chunks": sweep(8, t_z, len(zstream), t_out, n, want, False)}

print(json.dumps(res), flush=True)
if len(sys.argv) > 1 and sys.argv[1] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
enc.close()
