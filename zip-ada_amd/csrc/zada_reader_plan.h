// zada_reader_plan.h -- how the batch calls of the stream readers (zada_inflate_batch, zada_bunzip2_batch, zada_unlzma_batch, zada_unlegacy_batch:
// zada_reader_host.h) cut their entries into launch groups and lay a group out in its arena.  Pure host arithmetic, no HIP: compiled into the product
// and into tests/reader/reader_plan_host.cpp, which tests/test_reader_plan.py holds against a restatement in Python and runs under ASan + UBSan.
//
// The entry points refuse a stream or an output of 2 ** 40 bytes and more, and a limit is below 2 ** 40 as well (its knob counts MiB), so the sums
// below stay under limit + 2 ** 42: nothing wraps.
#pragma once
#include <stdint.h>

namespace zada {

constexpr uint64_t reader_pad16(uint64_t x) { return (x + 15) & ~15ull; }

struct ReaderGroup { int g0, g1; uint64_t in_bytes, out_bytes; };      // entries g0 .. g1 - 1; the bytes of their padded inputs / outputs

// a group: entries g0 .. g1 - 1, inputs then outputs in one arena, every buffer at a multiple of 16; the first entry is always taken
inline ReaderGroup reader_plan_group(int g0, int count, const uint64_t *n_in, const uint64_t *cap, uint64_t limit) {
  ReaderGroup G{g0, g0, 0, 0};
  while (G.g1 < count) {
    const uint64_t a = reader_pad16(n_in[G.g1]), b = reader_pad16(cap[G.g1]);
    if (G.g1 > g0 && G.in_bytes + G.out_bytes + a + b > limit) break;
    G.in_bytes += a; G.out_bytes += b; G.g1++;
  }
  return G;
}

// where the input (io [k]) and the output (oo [k]) of entry g0 + k lie in the group's arena: the inputs from 0, the outputs from in_bytes
inline void reader_plan_offsets(const ReaderGroup &G, const uint64_t *n_in, const uint64_t *cap, uint64_t *io, uint64_t *oo) {
  uint64_t a = 0, b = G.in_bytes;
  for (int i = G.g0; i < G.g1; i++) {
    io[i - G.g0] = a; oo[i - G.g0] = b;
    a += reader_pad16(n_in[i]); b += reader_pad16(cap[i]);
  }
}

// the outputs come back in one piece up to the last byte any entry wrote: that many bytes from the arena's offset in_bytes on.  wrote (k): the bytes
// entry g0 + k wrote, 0 where it failed
template <class Wrote> inline uint64_t reader_plan_extent(const ReaderGroup &G, const uint64_t *oo, Wrote wrote) {
  uint64_t hi = 0;
  for (int k = 0; k < G.g1 - G.g0; k++) if (const uint64_t n = wrote(k)) hi = oo[k] + n - G.in_bytes;
  return hi;
}

}  // namespace zada
