"""A measurement aid, not a test: ReZip.rezip_device, zada_compare_device and CompZip.compare_device on the GPU (profiles/rezip/NOTES.md holds what
it printed).

  python tests/gpu_rezip_perf.py [--mib 1024] [--entries 2000] [--kib 256] [--out FILE] [--only STEP]

Every step runs in a child process of its own with a time limit, and the script ends at the first step that fails.  A step's limit covers its whole
process: the import, the making of its inputs on the host (the archives of the compzip and rezip steps are written by zipfile before anything is
timed) and the timed calls; it is sized for the slowest of these, the host's Deflate of the compzip step and the LZMA_3 batches of the rezip step.
Each figure is the median of 9 runs after one warm-up run (the host yardstick of the rezip step: of 3 per method -- one pass over the seven methods of
the 256 KiB case takes 20 s, and its runs lie within a per cent of each other), timed by a host clock around a call that ends in a device
synchronise (the calls synchronise before they return).
  rezip      ReZip.rezip_device with the default approaches on 10 000 stored entries of 16 KiB and on 2 000 of 256 KiB, split by phase through
             last_timing; beside it the sum of what ZipCreate (m).add_streams + finish take from host bytes for the same distinct methods.
  compare    zada_compare_device on --mib MiB of equal bytes, at alignments (0, 0) and (3, 7), with last_timing's kernel time beside the call's;
             next to it the box's device-to-device copy of the same size (the probe of bench.py --full), read as bytes read per second.
  compzip    CompZip.compare_device on two archives of --entries stored entries of --kib KiB each (equal; Store, so that the figure is the
             extraction's copies and the compare kernel, not a decoder), and the same with Deflate_1 on side 2."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 9


def timed(fn):
    fn()                                                       # warm-up: code objects, workspace
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def step_compare(args):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _common import product
    za = product()
    enc = za.Encoder(0)
    n = args.mib << 20
    a = torch.randint(0, 256, (n + 16,), dtype=torch.uint8, device="cuda")
    b = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    out = {"bytes": n}
    # the copy probe of bench.py --full (hbm_copy_gbs), RESTATED here, not called: a device-to-device copy, best of 5, HIP events; bench.py counts
    # read + write, this counts the bytes read, half of it
    c = torch.empty(n, dtype=torch.uint8, device="cuda")
    best = 0.0
    c.copy_(a[:n])
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); c.copy_(a[:n]); e1.record(); e1.synchronize()
        best = max(best, n / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    out["copy_probe_read_gbs"] = round(best, 1)
    del c
    for al in ((0, 0), (3, 7)):
        b[al[1]:al[1] + n].copy_(a[al[0]:al[0] + n])
        torch.cuda.synchronize()
        kern = []

        def call():
            assert enc.compare_device(a.data_ptr() + al[0], b.data_ptr() + al[1], n) == n
            kern.append(sum(ms for nm, ms in enc.last_timing() if nm == "compare:k_cz_compare"))
        med, lo, hi = timed(call)
        k = statistics.median(kern[1:])
        out["a%d_b%d" % al] = {"call_ms": round(med * 1e3, 3), "call_ms_min_max": [round(lo * 1e3, 3), round(hi * 1e3, 3)], "kernel_ms": round(k, 3),
                               "read_gbs_call": round(2 * n / med / 1e9, 1), "read_gbs_kernel": round(2 * n / (k * 1e-3) / 1e9, 1)}
    # a difference in the last byte is found there (every piece was looked at); then one in the first piece: what the early exit of the pieces
    # behind it is worth
    b[al[1] + n - 1] ^= 1
    torch.cuda.synchronize()
    assert enc.compare_device(a.data_ptr() + al[0], b.data_ptr() + al[1], n) == n - 1
    b[al[1] + n - 1] ^= 1
    b[:n].copy_(a[:n])
    b[5] ^= 1
    torch.cuda.synchronize()
    med, _, _ = timed(lambda: enc.compare_device(a.data_ptr(), b.data_ptr(), n))
    out["difference_at_5_call_ms"] = round(med * 1e3, 3)
    enc.close()
    return out


def step_compzip(args):
    import io
    import zipfile
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _common import product, silesia_mix
    za = product()
    enc = za.Encoder(0)
    size = args.kib << 10
    text = silesia_mix(size + args.entries * 64)
    out = {"entries": args.entries, "entry_bytes": size}

    def archive(method, level=None):
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w", method, compresslevel=level) as z:
            for k in range(args.entries):
                z.writestr("e%05d" % k, text[k * 64:k * 64 + size])
        return torch.from_numpy(np.frombuffer(b.getvalue(), dtype=np.uint8).copy()).cuda()
    t1 = archive(zipfile.ZIP_STORED)
    for label, t2 in (("store_store", archive(zipfile.ZIP_STORED)), ("store_deflate", archive(zipfile.ZIP_DEFLATED, 1))):
        i1, i2 = za.ZipInfo.load_device(t1), za.ZipInfo.load_device(t2)
        cz = za.CompZip(enc)

        def call():
            r = cz.compare_device(i1, i2)
            assert r.total_differences == 0 and r.total_bytes == args.entries * size
        med, lo, hi = timed(call)
        out[label] = {"call_ms": round(med * 1e3, 2), "call_ms_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
                      "entry_gbs": round(args.entries * size / med / 1e9, 2)}
    enc.close()
    return out


def step_rezip(args):
    import io
    import zipfile
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _common import product, silesia_mix
    za = product()
    enc = za.Encoder(0)
    out = {}
    for label, count, size, runs in (("small16k", 10000, 16 << 10, RUNS), ("mid256k", 2000, 256 << 10, RUNS)):
        text = silesia_mix(size + count * 64)
        datas = [text[k * 64:k * 64 + size] for k in range(count)]
        names = ["e%05d.bin" % k for k in range(count)]
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w", zipfile.ZIP_STORED) as z:
            for nm, d in zip(names, datas):
                z.writestr(nm, d)
        t = torch.from_numpy(np.frombuffer(b.getvalue(), dtype=np.uint8).copy()).cuda()
        info = za.ZipInfo.load_device(t)
        rz = za.ReZip(enc)
        phases, got = [], {}

        def call():
            arc, rep = rz.rezip_device(info, report=True)
            got["len"], got["totals"] = arc.numel(), {a: v for a, v in rep["totals"].items() if v["count"]}
            phases.append(dict((nm, ms) for nm, ms in enc.last_timing() if not nm.startswith("#")))
        call()
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        ph = {nm: round(statistics.median(p.get(nm, 0.0) for p in phases[1:]), 3) for nm in phases[-1]}
        # the yardstick: the same distinct methods from host bytes, one archive each
        methods = sorted({za.preselect(m, za.guess_type_from_name(names[0]), size) for m in (34, 35)} | {10, 11, 12, 13, 14, 17, 18})
        host = {}
        for m in methods:
            def one():
                zc = za.ZipCreate(enc, m)
                zc.add_streams(names, datas)
                zc.finish()
            one()
            hs = []
            for _ in range(3):
                t0 = time.perf_counter(); one(); hs.append(time.perf_counter() - t0)
            host[m] = round(statistics.median(hs) * 1e3, 1)
        out[label] = {"entries": count, "entry_bytes": size, "runs": runs, "call_ms": round(med * 1e3, 1), "call_ms_min_max": [round(min(ts) * 1e3, 1), round(max(ts) * 1e3, 1)],
                      "archive_bytes": got["len"], "wins": got["totals"], "phase_ms": ph, "kernel_ms": round(sum(ph.values()), 1),
                      "host_add_streams_finish_ms_by_method": host, "host_sum_ms": round(sum(host.values()), 1)}
        del t, info
    enc.close()
    return out


STEPS = {"rezip": (step_rezip, 900), "compare": (step_compare, 300), "compzip": (step_compzip, 420)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--entries", type=int, default=2000)
    ap.add_argument("--kib", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="run this step alone")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(STEPS[args.step][0](args)))
        return 0
    results = {}
    for name, (_, limit) in STEPS.items():
        if args.only and name != args.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--mib", str(args.mib), "--entries", str(args.entries), "--kib", str(args.kib)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print("step %s: no result within %d s" % (name, limit))
            return 1
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print("step %s failed (exit %d)\n%s" % (name, r.returncode, r.stderr[-3000:]))
            return 1
        results[name] = json.loads(line[7:])
        print(name, json.dumps(results[name]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
