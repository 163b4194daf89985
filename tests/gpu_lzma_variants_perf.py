"""GPU script: what the data-type LZMA methods cost.  zada_lzma_batch over LZ_ENTRIES (default 4096) entries of 16 KiB of the
benchmark corpus for every method 19 .. 33 next to LZMA_2 / LZMA_3 on the same entries, and ONE 4 MiB stream of LZMA_3_for_Zip_in_Zip next to
LZMA_3 (zada_lzma, bounded launches, four waves).  Prints MB/s and the HBM literal table of one entry.  LZ_METHODS / LZ_STREAM_METHODS: comma
lists instead (LZ_STREAM_METHODS=18 with ZADA_LIB=<an older library>: the A/B of the default methods)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _common import product

Z = product()
enc = Z.Encoder(0)
lib = Z.load_library()
E = int(os.environ.get("LZ_ENTRIES", "4096"))
size = 16 << 10
mix = Z.silesia_mix(E * size, version=2)
datas = [bytes(mix[i * size:(i + 1) * size]) for i in range(E)]
methods = [int(m) for m in os.environ["LZ_METHODS"].split(",")] if os.environ.get("LZ_METHODS") else [17, 18] + list(range(19, 34))
enc.lzma_batch(datas[:8], 18)
for m in methods:
    t = time.time()
    res = enc.lzma_batch(datas, m)
    dt = time.time() - t
    print("batch method %d: %d x 16 KiB in %.2f s = %.1f MB/s, ratio %.3f, literal table %d bytes per entry" % (
        m, E, dt, E * size / dt / 1e6, sum(len(z) for _, z, _ in res) / (E * size), lib.zada_lzma_lit_table_bytes(m) if hasattr(lib, "zada_preselect") else 0), flush=True)
smethods = [int(m) for m in os.environ.get("LZ_STREAM_METHODS", "18,20").split(",") if m]
if smethods:
    d = bytes(Z.silesia_mix((4 << 20) + 12345, seed=0x5A1E51A))
    for m in smethods:
        t = time.time()
        rc, z, crc = enc.lzma(d, m)
        dt = time.time() - t
        print("stream method %d: %d bytes in %.2f s = %.2f MB/s, %d bytes out" % (m, len(d), dt, len(d) / dt / 1e6, len(z)), flush=True)
