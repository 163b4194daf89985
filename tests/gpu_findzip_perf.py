"""A measurement aid, not a test: zada_find_device and FindZip.find_device on the GPU (profiles/findzip/NOTES.md holds what it printed).

  python tests/gpu_findzip_perf.py [--out FILE] [--only STEP]

Every step runs in a child process of its own with a time limit, and the script ends at the first step that fails.  Each figure is the median of 9
runs after one warm-up run, timed by a host clock around a call that ends in a device synchronise (the calls synchronise before they return), with
last_timing's kernel time beside it.
  find       zada_find_device on 1 GiB and 4 GiB of the benchmark text (silesia_mix version 2: a tile of 64 MiB made on the host, repeated on the
             device) at alignment 3, with: an 8-byte string whose last four bytes occur nowhere, an 8-byte string whose last four bytes are a common four-gram of the
             text (both the filter alone), a 12-byte string whose last eight bytes occur in the text (the filter's survivors go through the wave-wide
             confirmation), a
             1024-byte string cut from the text, a 3-byte string (no confirmation at all), and -- on 256 MiB of "a" -- "b" + 40 "a", where every
             position survives the filter and none is an occurrence.  Yardsticks: zada_compare_device on the same number of bytes (it reads twice as
             many) and the closed form (bytes.translate + bytes.find) on one CPU core over the 64 MiB tile.
  findzip    FindZip.find_device on 10 000 entries of 16 KiB and on 2 000 of 256 KiB, stored and Deflate (zipfile, level 1), against
             UnZip.extract_device followed by one copy of the extracted bytes to the host -- the way to the bytes without this tool; the host's
             own search of them would come on top."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 9
TILE = 64 << 20


def timed(fn):
    fn()                                                       # warm-up: code objects, workspace
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def step_find(args):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _findzip
    from _common import product
    za = product()
    enc = za.Encoder(0)
    tile = za.silesia_mix(TILE, version=2).tobytes()
    common4 = tile[200000:200004]
    strings = {"rare8_rare_tail": b"Zq#R\x01\x02\x03\x04", "rare8_common_tail": b"#@!~" + common4, "rare12_common_tail": b"#@!~" + tile[199996:200004], "cut1024": tile[5000:6024], "three": tile[200000:200003]}
    out = {"tile_bytes": TILE, "strings": {k: v[:16].hex() for k, v in strings.items()}}
    # the closed form on one CPU core: To_Upper as a table, then bytes.find from hit to hit
    up = bytes(_findzip.to_upper_char(c) for c in range(256))
    want = {}
    for nm, s in strings.items():
        t0 = time.perf_counter()
        x, su = tile.translate(up), s.translate(up)
        occ, at = 0, x.find(su)
        first = at
        while at >= 0:
            occ += 1
            at = x.find(su, at + 1)
        dt = time.perf_counter() - t0
        want[nm] = (occ, first + len(s) - 1 if occ else None)
        out.setdefault("cpu_closed_form", {})[nm] = {"ms": round(dt * 1e3, 1), "gbs": round(TILE / dt / 1e9, 2), "occurrences_per_tile": occ, "last_four_per_tile": x.count(su[-4:])}
    t_tile = torch.from_numpy(np.frombuffer(tile, dtype=np.uint8).copy()).cuda()
    for gib in (1, 4):
        n = gib << 30
        a = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
        a[3:3 + n].view(-1, TILE).copy_(t_tile.expand(n // TILE, TILE))
        torch.cuda.synchronize()
        res = {}
        for nm, s in strings.items():
            kern, got = [], {}

            def call():
                got["r"] = enc.find_device(a.data_ptr() + 3, n, s)
                kern.append(sum(ms for k, ms in enc.last_timing() if k == "find:k_fz_search"))
            med, lo, hi = timed(call)
            k = statistics.median(kern[1:])
            # (an occurrence across the seam of two tiles would add to the count: none of these strings has one unless the figures say so)
            res[nm] = {"call_ms": round(med * 1e3, 3), "call_ms_min_max": [round(lo * 1e3, 3), round(hi * 1e3, 3)], "kernel_ms": round(k, 3),
                       "read_gbs_kernel": round(n / (k * 1e-3) / 1e9, 1), "occurrences": got["r"][0], "first": got["r"][1],
                       "cpu_says_per_tile": list(want[nm])}
            assert got["r"][0] >= want[nm][0] * (n // TILE) and got["r"][1] == (n if want[nm][1] is None else want[nm][1]), (nm, got, want[nm])
        # the yardstick: the compare kernel on the same number of bytes (two buffers: twice the bytes read)
        b = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
        b[3:3 + n].copy_(a[3:3 + n])
        torch.cuda.synchronize()
        kern = []

        def cmp_call():
            assert enc.compare_device(a.data_ptr() + 3, b.data_ptr() + 3, n) == n
            kern.append(sum(ms for k, ms in enc.last_timing() if k == "compare:k_cz_compare"))
        med, lo, hi = timed(cmp_call)
        k = statistics.median(kern[1:])
        res["compare_device"] = {"call_ms": round(med * 1e3, 3), "kernel_ms": round(k, 3), "read_gbs_kernel": round(2 * n / (k * 1e-3) / 1e9, 1)}
        out["gib%d" % gib] = res
        del a, b
    # dense candidates: every position survives the filter, none is an occurrence
    n = 256 << 20
    a = torch.full((n + 16,), 0x61, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for nm, s in (("dense_b_40a", b"b" + b"a" * 40), ("dense_aaa", b"aaa")):
        kern, got = [], {}

        def call():
            got["r"] = enc.find_device(a.data_ptr() + 3, n, s)
            kern.append(sum(ms for k, ms in enc.last_timing() if k == "find:k_fz_search"))
        med, lo, hi = timed(call)
        k = statistics.median(kern[1:])
        out[nm] = {"bytes": n, "call_ms": round(med * 1e3, 3), "kernel_ms": round(k, 3), "read_gbs_kernel": round(n / (k * 1e-3) / 1e9, 1),
                   "occurrences": got["r"][0], "ns_per_candidate": round(k * 1e6 / n, 3)}
    assert out["dense_b_40a"]["occurrences"] == 0 and out["dense_aaa"]["occurrences"] == n - 2
    enc.close()
    return out


def step_findzip(args):
    import io
    import zipfile
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _common import product
    za = product()
    enc = za.Encoder(0)
    out = {}
    for label, count, size in (("small16k", 10000, 16 << 10), ("mid256k", 2000, 256 << 10)):
        text = za.silesia_mix(size + count * 64, version=2).tobytes()
        s = text[size // 2:size // 2 + 8]
        for mname, method, level in (("store", zipfile.ZIP_STORED, None), ("deflate", zipfile.ZIP_DEFLATED, 1)):
            b = io.BytesIO()
            with zipfile.ZipFile(b, "w", method, compresslevel=level) as z:
                for k in range(count):
                    z.writestr("e%05d.bin" % k, text[k * 64:k * 64 + size])
            t = torch.from_numpy(np.frombuffer(b.getvalue(), dtype=np.uint8).copy()).cuda()
            info = za.ZipInfo.load_device(t)
            fz, uz = za.FindZip(enc), za.UnZip(enc)
            phases, got = [], {}

            def call():
                r = fz.find_device(info, s)
                got["hits"], got["damaged"] = len(r.in_contents), r.damaged
                phases.append(dict((nm, ms) for nm, ms in enc.last_timing() if not nm.startswith("#")))
            med, lo, hi = timed(call)
            ph = {nm: round(statistics.median(p.get(nm, 0.0) for p in phases[1:]), 3) for nm in phases[-1]}

            def old_way():
                views = uz.extract_device(info)
                base = next(iter(views.values()))._base
                got["host_bytes"] = base.cpu().numel()
            med2, lo2, hi2 = timed(old_way)
            assert got["damaged"] == 0 and got["hits"] >= 1
            out["%s_%s" % (label, mname)] = {"string": s.hex(), "entries": count, "entry_bytes": size, "archive_bytes": t.numel(), "entries_with_hits": got["hits"],
                                            "find_device_ms": round(med * 1e3, 2), "find_device_ms_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
                                            "phase_ms": ph, "search_kernel_ms": ph.get("findzip:k_fz_search"),
                                            "extract_device_and_copy_to_host_ms": round(med2 * 1e3, 2), "extract_copy_ms_min_max": [round(lo2 * 1e3, 2), round(hi2 * 1e3, 2)],
                                            "entry_gbs": round(count * size / med / 1e9, 2)}
            del t, info
    enc.close()
    return out


STEPS = {"find": (step_find, 540), "findzip": (step_findzip, 540)}


def main():
    ap = argparse.ArgumentParser()
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
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name]
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
