"""GPU script: what the batched parallel Inflate ("inflate_par_batch") gives for archives of many large entries, after
gpu_inflate_par_perf.py.  One process.  Archives written by zada_zip_device (ZipCreate.write_device, Deflate_3) from silesia_mix_v2:
  S16. 16 entries of 64 MiB;  S256. 256 entries of 4 MiB;  S2000. 2 000 entries of 256 KiB.
Each goes through zada_unzip_device, test-only and into outputs, three ways in the same process, alternating run by run:
  off   : the knobs off (one wave per entry);
  seq   : "inflate_par_min_kib" = 64 alone: the entries one after the other, the reference for the gain;
  batch : "inflate_par_min_kib" = 64 with "inflate_par_batch" = 1.
One warm-up, then the median of RUNS runs by the wall clock of the call, which ends synchronised; a way whose warm-up took more than SLOW_S
seconds gets SLOW_RUNS runs and one whose warm-up took more than VERY_SLOW_S gets one (the result's "runs_ms" says how many there were: the
sequential way takes a minute per run on S2000).  The spread is max - min of the runs; the split is last_timing of the last run.  The outputs
of the three ways are compared byte for byte.  S2000 also sweeps "inflate_par_min_kib" over 64 / 256 / 1 024 with the batch on.
Arguments: the JSON file to write ("-": standard output only), then the shapes to run (default: S16 S256 S2000; "S2000-sweep": the sweep alone)."""
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
shapes = sys.argv[2:] or ["S16", "S256", "S2000"]
SHAPES = {"S16": (16, 64 << 20), "S256": (256, 4 << 20), "S2000": (2000, 256 << 10)}
RUNS, SLOW_S, SLOW_RUNS, VERY_SLOW_S = 5, 4.0, 3, 30.0
WAYS = {"off": (0, 0), "seq": (64, 0), "batch": (64, 1)}
res = {"corpus": "silesia_mix_v2", "runs": RUNS, "slow_s": SLOW_S, "slow_runs": SLOW_RUNS, "very_slow_s": VERY_SLOW_S}
mix = Z.silesia_mix(max(SHAPES[s.split("-")[0]][0] * SHAPES[s.split("-")[0]][1] for s in shapes), version=2)


def table_of(info):
    n = len(info.entries)
    tab = np.zeros(n, dtype=enc.unzip_dtypes()[0])
    tab["in_off"], tab["n_in"] = [e.data_offset for e in info.entries], [e.csize for e in info.entries]
    tab["cap"], tab["method"] = [e.usize for e in info.entries], [e.method for e in info.entries]
    slots = (tab["cap"] + np.uint64(255)) & ~np.uint64(255)
    tab["out_off"] = np.cumsum(slots) - slots
    return tab, int(slots.sum())


def one_call(t_arc, tab, t_out, total, min_kib, batch):
    enc.set_knob("inflate_par_min_kib", min_kib)
    enc.set_knob("inflate_par_batch", batch)
    torch.cuda.synchronize()
    t = time.perf_counter()
    rc, r = enc.unzip_device(t_arc.data_ptr(), t_arc.numel(), None if t_out is None else t_out.data_ptr(), 0 if t_out is None else total, tab)
    ms = (time.perf_counter() - t) * 1e3
    enc.set_knob("inflate_par_min_kib", 0)
    enc.set_knob("inflate_par_batch", 0)
    assert rc == 0 and (r["rc"] == 0).all() and (r["out_len"] == tab["cap"]).all()
    return ms, r["crc"].copy(), dict(enc.last_timing()), enc.inflate_par_last()


def measure(t_arc, tab, total, crcs, ways, into):
    t_out = {w: torch.empty(total, dtype=torch.uint8, device="cuda") for w in ways} if into else {w: None for w in ways}
    wall, split, rec, want = {w: [] for w in ways}, {}, {}, {}
    for rep in range(RUNS + 1):
        for w, (min_kib, batch) in ways.items():
            if rep > want.get(w, RUNS):
                continue
            ms, crc, split[w], rec[w] = one_call(t_arc, tab, t_out[w], total, min_kib, batch)
            assert (crc == crcs).all(), w
            if rep == 0:
                want[w] = 1 if ms > VERY_SLOW_S * 1e3 else SLOW_RUNS if ms > SLOW_S * 1e3 else RUNS          # (the warm-up books the workspaces: not counted)
            else:
                wall[w].append(ms)
    if into:
        first = next(iter(ways))
        for w in ways:
            assert torch.equal(t_out[w], t_out[first]), "the outputs of %s and %s differ" % (w, first)
    out = {}
    for w in ways:
        xs = wall[w]
        out[w] = {"median_ms": statistics.median(xs), "spread_ms": max(xs) - min(xs), "runs_ms": xs, "split_ms": split[w], "record": rec[w] if ways[w][0] else None}
        print("   %-9s %-10s %9.1f ms  (spread %.1f, %d runs)  %s" % ("outputs" if into else "test-only", w, out[w]["median_ms"], out[w]["spread_ms"], len(xs),
                                                                    "" if not ways[w][0] else "rounds %d, repairs %d, fell back %d of %d" % (
                                                                        rec[w]["scout_rounds"], rec[w]["repairs"], rec[w]["fell_back"], rec[w]["streams"])), flush=True)
    return out


for s in shapes:
    E, SZ = SHAPES[s.split("-")[0]]
    sweep_only = s.endswith("-sweep")
    print("%s. %d entries of %d KiB" % (s, E, SZ >> 10), flush=True)
    tensors = [torch.from_numpy(mix[k * SZ:(k + 1) * SZ]).cuda() for k in range(E)]
    zc = Z.ZipCreate(enc, Z.Method.Deflate_3)
    t_arc = zc.write_device(["e%05d" % k for k in range(E)], tensors).clone()
    del tensors
    info = Z.ZipInfo.load_device(t_arc)
    tab, total = table_of(info)
    crcs = np.array([e.crc ^ 0xFFFFFFFF for e in info.entries], dtype=np.uint32)
    r = {"entries": E, "entry_bytes": SZ, "archive_bytes": int(t_arc.numel()), "stream_bytes_median": int(statistics.median(e.csize for e in info.entries))}
    if not sweep_only:
        r["into_outputs"] = measure(t_arc, tab, total, crcs, WAYS, True)
        r["test_only"] = measure(t_arc, tab, total, crcs, WAYS, False)
    for form in () if sweep_only else ("into_outputs", "test_only"):
        m = r[form]
        slower = max(("off", "seq"), key=lambda w: m[w]["median_ms"])
        r[form]["bar_met"] = all(m["batch"]["median_ms"] + m[slower]["spread_ms"] < m[w]["median_ms"] for w in ("off", "seq"))
    if s.startswith("S2000"):
        r["sweep_min_kib"] = measure(t_arc, tab, total, crcs, {"off": (0, 0), "batch_64": (64, 1), "batch_256": (256, 1), "batch_1024": (1024, 1)}, True)
    res[s] = r
    del t_arc

print(json.dumps(res), flush=True)
if len(sys.argv) > 1 and sys.argv[1] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
enc.close()
