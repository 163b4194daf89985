"""GPU script: what a password costs.  The Deflate_3 stream of 1 GiB of the benchmark corpus (silesia_mix_v2), resident in
device memory:
  1. device time of zada_crypt_encode_device over it (HIP events on the context's stream: last_timing), warm-up, then the median of eleven runs,
     next to the Deflate_3 step that made the stream, measured again here;
  2. the byte-serial C model (tests/crypt/crypt_model.c) over the same bytes on one core of the same box;
  3. zada_compress_data_pw against zada_compress_data on the same 1 GiB through host buffers;
  4. crypt_encode_batch over 10 000 entries of 16 KiB against the model's loop.
CRYPT_MIB: another input size.  Argument: the JSON file to write (default: standard output only)."""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _crypt
from _common import ROOT, product

Z = product()
enc = Z.Encoder(0)
L = enc.lib
MIB = int(os.environ.get("CRYPT_MIB", "1024"))
KEYS = _crypt.init_keys(b"benchmark")
res = {"input_mib": MIB, "corpus": "silesia_mix_v2"}
try:
    res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
except OSError:
    res["commit"] = None

d_np = Z.silesia_mix(MIB << 20, version=2)
n = len(d_np)
t_in = torch.from_numpy(d_np).cuda()
t_out = torch.empty(n + (n >> 3) + (1 << 20), dtype=torch.uint8, device="cuda")
enc.deflate_device(t_in.data_ptr(), min(n, 1 << 20), t_out.data_ptr(), t_out.numel(), 10)      # warm-up
step = []
for _ in range(5):
    torch.cuda.synchronize()
    t = time.perf_counter()
    rc, ol, _ = enc.deflate_device(t_in.data_ptr(), n, t_out.data_ptr(), t_out.numel(), 10)
    torch.cuda.synchronize()
    step.append((time.perf_counter() - t) * 1e3)
assert rc == 0
res["deflate3_step_ms"] = {"median": statistics.median(step), "runs": step}
res["stream_bytes"] = ol
print("Deflate_3 step, %d MiB device-resident: median %.1f ms (%s); stream %d bytes" % (MIB, statistics.median(step), " ".join("%.1f" % x for x in step), ol), flush=True)

# 1. the encode over the resident stream
stream_host = bytes(t_out[:ol].cpu().numpy())
want, kw = None, None
for _ in range(2):
    enc.crypt_encode_device(KEYS, t_out.data_ptr(), ol)                                          # warm-up (the second run encodes the first one's bytes: the time does not depend on them)
dev, wall = [], []
for _ in range(11):
    torch.cuda.synchronize()
    t = time.perf_counter()
    enc.crypt_encode_device(KEYS, t_out.data_ptr(), ol)
    wall.append((time.perf_counter() - t) * 1e3)
    dev.append(dict(enc.last_timing())["crypt:encode"])
res["encode_device_ms"] = {"median": statistics.median(dev), "runs": dev, "wall_median": statistics.median(wall)}
print("1. zada_crypt_encode_device over %d bytes: device median %.3f ms = %.1f GB/s (wall %.3f ms)" % (ol, statistics.median(dev), ol / statistics.median(dev) / 1e6, statistics.median(wall)), flush=True)
# (and once for the bytes: a fresh copy of the stream against the model)
t_chk = torch.frombuffer(bytearray(stream_host), dtype=torch.uint8).cuda()
k_gpu = enc.crypt_encode_device(KEYS, t_chk.data_ptr(), ol)

# 2. the model on one core
buf = np.frombuffer(stream_host, dtype=np.uint8).copy()
k = (ctypes.c_uint32 * 3)(*KEYS)
t = time.perf_counter()
_crypt.model().cm_encode(k, buf.ctypes.data, len(buf))
model_ms = (time.perf_counter() - t) * 1e3
assert tuple(k) == k_gpu and bytes(t_chk.cpu().numpy()) == buf.tobytes(), "GPU cipher text differs from the model"
res["model_one_core_ms"] = model_ms
res["encode_speedup_over_model"] = model_ms / statistics.median(dev)
res["encode_share_of_deflate3_step"] = statistics.median(dev) / statistics.median(step)
print("2. C model, one core, same bytes: %.1f ms = %.3f GB/s  (GPU %.0f x; the encode is %.2f %% of the Deflate_3 step)" % (
    model_ms, ol / model_ms / 1e6, res["encode_speedup_over_model"], 100 * res["encode_share_of_deflate3_step"]), flush=True)
del t_in, t_out, t_chk

# 3. end to end through host buffers
out = np.empty(n + 64 + 12, dtype=np.uint8)
olc, crc, zt = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint16(0)
h11 = bytes(range(11))


def plain():
    return L.zada_compress_data(enc.ctx, 10, d_np.ctypes.data, n, out.ctypes.data, len(out), ctypes.byref(olc), ctypes.byref(crc), ctypes.byref(zt))


def with_pw():
    return L.zada_compress_data_pw(enc.ctx, 10, 0, b"benchmark", 9, h11, d_np.ctypes.data, n, out.ctypes.data, len(out), ctypes.byref(olc), ctypes.byref(crc), ctypes.byref(zt), None)


for name, fn in (("compress_data_ms", plain), ("compress_data_pw_ms", with_pw)):
    assert fn() == 0
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        assert fn() == 0
        ts.append((time.perf_counter() - t) * 1e3)
    res[name] = {"median": statistics.median(ts), "runs": ts, "out_len": olc.value}
print("3. host buffers, %d MiB: zada_compress_data %.1f ms, zada_compress_data_pw %.1f ms (a password costs %.1f ms)" % (
    MIB, res["compress_data_ms"]["median"], res["compress_data_pw_ms"]["median"], res["compress_data_pw_ms"]["median"] - res["compress_data_ms"]["median"]), flush=True)

# 4. many small buffers
E, SZ = 10000, 16384
small = Z.silesia_mix(E * SZ, version=2)
datas = [bytes(small[i * SZ:(i + 1) * SZ]) for i in range(E)]
keys = [(i * 2654435761 & 0xFFFFFFFF, i ^ 0x5A5A5A5A, 0x34567890 + i) for i in range(E)]
lens = np.full(E, SZ, dtype=np.uint64)
arena = small.copy()
ptrs = (arena.ctypes.data + np.arange(E, dtype=np.uint64) * SZ).astype(np.uint64)
ks = np.array(keys, dtype=np.uint32)
assert L.zada_crypt_encode_batch(enc.ctx, E, ks.ctypes.data, ptrs.ctypes.data, lens.ctypes.data) == 0       # warm-up, and the bytes
chk = [0, 1, 4999, 9999]
for i in chk:
    assert (bytes(arena[i * SZ:(i + 1) * SZ]), tuple(int(x) for x in ks[i])) == _crypt.encode(keys[i], datas[i]), i
ts = []
for _ in range(5):
    ks = np.array(keys, dtype=np.uint32)
    t = time.perf_counter()
    assert L.zada_crypt_encode_batch(enc.ctx, E, ks.ctypes.data, ptrs.ctypes.data, lens.ctypes.data) == 0
    ts.append((time.perf_counter() - t) * 1e3)
M = _crypt.model()
mbuf = small.copy()
t = time.perf_counter()
for i in range(E):
    k = (ctypes.c_uint32 * 3)(*keys[i])
    M.cm_encode(k, mbuf.ctypes.data + i * SZ, SZ)
mloop = (time.perf_counter() - t) * 1e3
res["batch_10000x16k_ms"] = {"median": statistics.median(ts), "runs": ts, "model_loop_ms": mloop}
print("4. crypt_encode_batch, %d entries of %d bytes (host buffers, copies included): median %.1f ms; the model's loop %.1f ms" % (E, SZ, statistics.median(ts), mloop), flush=True)

print(json.dumps(res), flush=True)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
enc.close()
