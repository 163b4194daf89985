"""GPU script: what Deflate_R costs.  Device-resident zada_deflate_device on silesia_mix_v2 at 256 MiB and 1 GiB
(RICH_SIZES_MIB: a comma list instead) and on 64 MiB of two-symbol random data (every walk runs to the 4 096-candidate cap), split
into the Rich stage (the rich:* marks of last_timing) and the entropy stage (the rest); then the CPU model (tests/rich/rich_model.c,
one thread) on the same 64 MiB of silesia_mix_v2 and on the first MiB of the two-symbol data (the whole 64 MiB would take hours)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rich
from _common import product

Z = product()
enc = Z.Encoder(0)
R = 11


def run(name, d_np, reps=2):
    n = len(d_np)
    t_in = torch.from_numpy(d_np).cuda()
    t_out = torch.empty(n + (n >> 3) + (1 << 20), dtype=torch.uint8, device="cuda")
    enc.deflate_device(t_in.data_ptr(), min(n, 1 << 20), t_out.data_ptr(), t_out.numel(), R)      # warm-up
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.time()
        rc, ol, _ = enc.deflate_device(t_in.data_ptr(), n, t_out.data_ptr(), t_out.numel(), R)
        torch.cuda.synchronize()
        dt = time.time() - t
        tm = [(k, v) for k, v in enc.last_timing() if not k.startswith("#")]
        rich = sum(v for k, v in tm if k.startswith("rich:"))
        stages = " ".join("%s=%.1f" % (k, v) for k, v in tm if k.startswith("rich:"))
        if best is None or dt < best[0]:
            best = (dt, rc, ol, rich, sum(v for _, v in tm) - rich, stages)
    dt, rc, ol, rich, ent, stages = best
    print("%s: %d MiB rc=%d ratio %.4f  %.3f s = %.0f MB/s  (Rich stage %.1f ms = %.0f MB/s [%s], entropy stage %.1f ms)" % (
        name, n >> 20, rc, ol / n, dt, n / dt / 1e6, rich, n / rich / 1e3 if rich else 0, stages, ent), flush=True)
    del t_in, t_out


for mib in [int(x) for x in os.environ.get("RICH_SIZES_MIB", "256,1024").split(",") if x]:
    run("silesia_mix_v2", Z.silesia_mix(mib << 20, version=2))
two = np.random.RandomState(1).randint(0, 2, 64 << 20).astype(np.uint8)
run("two_symbol_random", two, reps=1)
if os.environ.get("RICH_MODEL", "1") == "1":
    d = bytes(Z.silesia_mix(64 << 20, version=2))
    t = time.time()
    _rich.restate(d)
    dt = time.time() - t
    print("model (restatement, one thread) silesia_mix_v2 64 MiB: %.1f s = %.2f MB/s" % (dt, len(d) / dt / 1e6), flush=True)
    d = bytes(two[:1 << 20])
    t = time.time()
    _rich.restate(d)
    dt = time.time() - t
    print("model (restatement, one thread) two_symbol_random first 1 MiB: %.1f s = %.3f MB/s" % (dt, len(d) / dt / 1e6), flush=True)
