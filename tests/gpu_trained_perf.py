"""GPU script: what Trained_Compression's forks give (profiles/trained/NOTES.md).  One process; warm-up, then the median of 9 runs;
device times from HIP events on the context's stream (last_timing), the call's wall clock beside them.
Workload: gs1.xls + the ten noise bytes as the trainer (tests/golden/trained), E messages (default 10 000) of 4 KiB cut from gs2.xls / gs3.xls at seeded
offsets, all in device memory.
  new, forked      zada_trained_encode_device / zada_trained_decode_device as they are
  new, unforked    the same calls with the knob "trained_fork" = 0: every entry codes / decodes its whole stream
  yardstick        what the library could do before: the E concatenations trainer & message through zada_lzma_batch (LZMA_3; its dictionary is the
                   ENTRY'S SIZE, not 2 ** 19, so its streams are not the reference's), and those streams through zada_unlzma_batch.  Both take host
                   buffers; only their device time between the marks is counted (for the encoder without the copy in: "lzma:bt4" + "lzma:end", the
                   copy out included; for the decoder the kernel alone, "unlzma:k_unlzma").
  CPU              one core of the oracle (the reference's coder) and of liblzma (raw LZMA1, preset 6, dictionary 2 ** 19, trainer & message each
                   time) on a sample of the same work, scaled to E.
Arguments: the JSON file to write (default: standard output only), E, the CPU sample's size."""
import json
import lzma
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import product
from _lzmah import oracle_lzma_encode
from _trained import DICT, fixture, message_of

Z = product()
enc = Z.Encoder(0)
E = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
SAMPLE = int(sys.argv[3]) if len(sys.argv) > 3 else 40
MSG, RUNS = 4096, 9
trainer = fixture("gs1.xls") + fixture("rnd_10.bin")
T = len(trainer)
rng = np.random.default_rng(2018)
src = (fixture("gs2.xls"), fixture("gs3.xls"))
msgs = []
for k in range(E):
    s = src[k & 1]
    o = int(rng.integers(0, len(s) - MSG))
    msgs.append(s[o:o + MSG])
res = {"entries": E, "message_bytes": MSG, "trainer_bytes": T, "runs": RUNS, "compute_units": torch.cuda.get_device_properties(0).multi_processor_count}


def med(xs):
    return {"median": statistics.median(xs), "runs": [round(x, 3) for x in xs]}


def split(prefixes):
    out = {}
    for name, ms in enc.last_timing():
        if name.startswith(prefixes):
            out[name] = out.get(name, 0.0) + ms
    return out


def measure(call, prefixes, pick=None):
    """RUNS runs of call () behind one warm-up -> wall ms, device ms (the marks of `pick`, or all with the prefixes), the last split"""
    call()
    wall, dev, sp = [], [], {}
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
        sp = split(prefixes)
        dev.append(sum(v for k, v in sp.items() if pick is None or k in pick))
    return {"wall_ms": med(wall), "device_ms": med(dev), "last_split_ms": {k: round(v, 3) for k, v in sp.items()}}


# ---- the new code ----
tc = Z.TrainedCompression(enc, trainer)
td = Z.TrainedCompression.for_decoding(enc, tc.stub, tc.skip, tc.trainer_len)
res.update(stub_bytes=len(tc.stub), skip=tc.skip, encoder_info=tc.info(), decoder_info=td.info())
dev = torch.device("cuda", 0)
blob = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()).to(dev)
CAPM = MSG + MSG // 8 + 512
out_m = torch.empty(E * CAPM, dtype=torch.uint8, device=dev)
rows_e = [(blob.data_ptr() + k * MSG, MSG, out_m.data_ptr() + k * CAPM, CAPM) for k in range(E)]
state = {}


def run_encode():
    state["enc"] = tc.encode_raw(rows_e)
    assert state["enc"][0] == 0


enc.set_knob("trained_fork", 1)
res["encode_forked"] = measure(run_encode, ("lzma:",))
res["encode_forked"]["coder_ms"] = res["encode_forked"]["last_split_ms"].get("lzma:end")
assert tc.info()["forked"] == E
ols = state["enc"][1]
host_m = out_m.cpu().numpy()
coded = [host_m[k * CAPM:k * CAPM + ols[k]].tobytes() for k in range(E)]
for k in range(0, E, max(1, E // 8)):
    assert coded[k] == message_of(trainer, msgs[k], tc.skip), "message %d differs from the oracle" % k
res["trained_bytes"] = sum(ols)
print("encode, forked: device %.1f ms (wall %.1f); %d bytes of messages for %d of data" % (
    res["encode_forked"]["device_ms"]["median"], res["encode_forked"]["wall_ms"]["median"], sum(ols), E * MSG), flush=True)
enc.set_knob("trained_fork", 0)
res["encode_unforked"] = measure(run_encode, ("lzma:",))
assert tc.info()["unforked"] == E and state["enc"][1] == ols
print("encode, unforked: device %.1f ms" % res["encode_unforked"]["device_ms"]["median"], flush=True)

mblob = torch.from_numpy(np.frombuffer(b"".join(coded), dtype=np.uint8).copy()).to(dev)
moff = np.concatenate(([0], np.cumsum(ols)))
out_d = torch.empty(E * MSG, dtype=torch.uint8, device=dev)
rows_d = [(mblob.data_ptr() + int(moff[k]), ols[k], out_d.data_ptr() + k * MSG, MSG) for k in range(E)]


def run_decode():
    state["dec"] = td.decode_raw(rows_d)
    assert state["dec"][0] == 0


enc.set_knob("trained_fork", 1)
res["decode_forked"] = measure(run_decode, ("trained:",))
assert td.info()["forked"] == E and out_d.cpu().numpy().tobytes() == b"".join(msgs), "decoded messages differ from the data"
print("decode, forked: device %.2f ms (wall %.1f)" % (res["decode_forked"]["device_ms"]["median"], res["decode_forked"]["wall_ms"]["median"]), flush=True)
enc.set_knob("trained_fork", 0)
res["decode_unforked"] = measure(run_decode, ("trained:",))
assert td.info()["unforked"] == E and out_d.cpu().numpy().tobytes() == b"".join(msgs)
enc.set_knob("trained_fork", 1)
print("decode, unforked: device %.2f ms" % res["decode_unforked"]["device_ms"]["median"], flush=True)

# ---- the yardstick: what the library could do before ----
cats = [trainer + m for m in msgs]
state["y"] = None


def run_y_encode():
    state["y"] = enc.lzma_batch(cats, Z.Method.LZMA_3)


res["yardstick_encode"] = measure(run_y_encode, ("lzma:",), pick=("lzma:bt4", "lzma:end"))
payloads = [p[1] for p in state["y"]]
res["yardstick_stream_bytes"] = sum(len(p) for p in payloads)
print("yardstick encode (zada_lzma_batch on trainer & message): device %.1f ms" % res["yardstick_encode"]["device_ms"]["median"], flush=True)
sizes = [T + MSG] * E


def run_y_decode():
    state["yd"] = enc.unlzma_batch(payloads, sizes, True, deliver=False)


res["yardstick_decode"] = measure(run_y_decode, ("unlzma:",), pick=("unlzma:k_unlzma",))
print("yardstick decode (zada_unlzma_batch on those streams): kernel %.1f ms" % res["yardstick_decode"]["device_ms"]["median"], flush=True)
untrained = enc.lzma_batch(msgs, Z.Method.LZMA_3)
res["untrained_bytes"] = sum(len(p[1]) - 4 for p in untrained)          # (without the four bytes of the Zip prefix; the 5-byte header stays)
res["ratio_encode"] = res["encode_forked"]["device_ms"]["median"] / res["yardstick_encode"]["device_ms"]["median"]
res["ratio_decode"] = res["decode_forked"]["device_ms"]["median"] / res["yardstick_decode"]["device_ms"]["median"]
print("forked / yardstick: encode %.3f, decode %.3f; sizes: trained %d, untrained %d" % (res["ratio_encode"], res["ratio_decode"], res["trained_bytes"], res["untrained_bytes"]), flush=True)

# ---- one CPU core on a sample of the same work ----
t = time.perf_counter()
for m in msgs[:SAMPLE]:
    oracle_lzma_encode(trainer + m, 3, 3, 0, 2, end_marker=True, dictionary_size=DICT)
res["cpu_oracle_encode_ms_scaled"] = (time.perf_counter() - t) * 1e3 * E / SAMPLE
flt = [{"id": lzma.FILTER_LZMA1, "preset": 6, "dict_size": DICT, "lc": 3, "lp": 0, "pb": 2}]
streams = []
t = time.perf_counter()
for m in msgs[:SAMPLE * 5]:
    c = lzma.LZMACompressor(lzma.FORMAT_RAW, filters=flt)
    streams.append(c.compress(trainer + m) + c.flush())
res["cpu_liblzma_encode_ms_scaled"] = (time.perf_counter() - t) * 1e3 * E / (SAMPLE * 5)
t = time.perf_counter()
for s in streams:
    lzma.LZMADecompressor(lzma.FORMAT_RAW, filters=flt).decompress(s)
res["cpu_liblzma_decode_ms_scaled"] = (time.perf_counter() - t) * 1e3 * E / (SAMPLE * 5)
res["cpu_sample"] = SAMPLE
print("one CPU core, scaled to %d entries: oracle encode %.0f ms, liblzma encode %.0f ms, liblzma decode %.0f ms" % (
    E, res["cpu_oracle_encode_ms_scaled"], res["cpu_liblzma_encode_ms_scaled"], res["cpu_liblzma_decode_ms_scaled"]), flush=True)

print(json.dumps(res), flush=True)
if len(sys.argv) > 1 and sys.argv[1] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
tc.close(); td.close()
enc.close()
