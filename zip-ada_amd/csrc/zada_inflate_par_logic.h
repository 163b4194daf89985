// zada_inflate_par_logic.h -- one large raw Deflate (Zip format 8) or Deflate64 (format 9) stream decoded by many waves: two-stage decoding with window markers, as in
// pugz and rapidgzip.  Host + device inline code with no HIP calls, in the style of zada_inflate_logic.h: the kernels of zada_inflate_par.hip run
// it with one wave per chunk, tests/inflate_par/inflate_par_host.cpp compiles the same text into a CPU model with one "lane".
//
// The compressed stream is cut into chunks of S bytes; chunk k covers the bits [k S 8, (k + 1) S 8).  Chunk 0 starts at bit 0 and is exact.
//   scout  : per chunk, FIND the first candidate start of a dynamic, non-final block in the chunk's range (infp_filter on every bit offset, then
//            inf_dynamic_header with all its rules), then COUNT: decode from there without writing, up to the first block end that is final or
//            lies at or beyond the chunk's boundary (infp_stop).  InfpRec says where the chunk began and ended and how many bytes it made.
//   chain  : the host walks from chunk 0 (infp_walk).  A chunk that ends at bit e is followed by the chunk whose range holds e, and that chunk's
//            start must EQUAL e: the walk started from an exact chunk, so equality proves a true block start and correctness never rests on the
//            finder.  Otherwise the chunk is repaired: scouted again from the exact start e, no search.  Chunks the chain steps over are dead.
//   decode : per live chunk, tokens into 16-bit symbols at the chunk's now known output offset.  A match source before the chunk's first byte
//            becomes a marker (infp_marker); sources inside the chunk copy symbols, so markers propagate by themselves.
//   window : the live chunks in order: the markers in the last 32 KiB of a chunk's symbols are replaced by the symbols they point at, which lie
//            in the already resolved tail of an earlier chunk (a marker reaches at most 32 768 back from its chunk's first byte).
//   finish : symbols to bytes, all chunks in parallel; a marker that is left reads the resolved tail in front of its chunk.
// Damaged streams, too many repairs, fewer than two live chunks: the stream goes to the one-wave decoder, whose verdict is the answer.
// The above is said for Deflate.  Deflate64 differs by its 32 distance codes and its length code 285 (d64 = true in zada_inflate_logic.h), by its
// window of 65 536 and by the symbol: a marker's offset then takes 16 bits, so the symbol is 32 bits wide (InfpFmt <9>).
#pragma once
#include "zada_inflate_logic.h"

namespace zada {

constexpr uint32_t INFP_MARK = 0x8000u;               // a symbol with this bit is a marker; Deflate's window of 32 768 fits the other 15 bits (Deflate64's does not)
constexpr uint32_t INFP_WINDOW = 32768u;
// What depends on the format.  A marker's offset is base - 1 - sp, in 0 .. WINDOW - 1; Deflate64's 65 536 offsets and the 256 literals are 65 792
// values, more than 16 bits hold: its symbol has 32 bits, the flag in the topmost, far from the offset.
template <int FORMAT> struct InfpFmt;
template <> struct InfpFmt<8> { typedef uint16_t sym_t; static constexpr bool D64 = false; static constexpr uint32_t MARK = INFP_MARK, WINDOW = INFP_WINDOW; };
template <> struct InfpFmt<9> { typedef uint32_t sym_t; static constexpr bool D64 = true; static constexpr uint32_t MARK = 0x80000000u, WINDOW = 65536u; };
constexpr uint64_t INFP_SEARCH = ~0ull;               // InfpJob::start_bit: find the start
constexpr uint32_t INFP_REPAIR_FLOOR = 2;             // repairs allowed whatever the share says: a stream's final block is never a candidate

enum { INFP_F_FOUND = 1, INFP_F_FINAL = 2, INFP_F_EXACT = 4 };
struct InfpJob { uint64_t start_bit; uint32_t chunk, pad; };                            // scout: chunk, and the exact start or INFP_SEARCH
struct InfpRec { uint64_t start_bit, end_bit, bytes; uint32_t flags, rule; };          // what the scout leaves per chunk
struct InfpLive { uint64_t start_bit, stop_bits, off, bytes, end_bit; uint32_t rule, final; };   // decode: a live chunk, its output offset; end_bit, rule, final: what the decode found
enum InfpReason { INFP_NONE = 0, INFP_DAMAGED = 1, INFP_REPAIRS = 2, INFP_SINGLE_CHUNK = 3, INFP_FORMAT = 4, INFP_MEMORY = 5 };

// ---- the candidate filter: the 81 bits at a bit offset, lo = bits 0 .. 63, hi = bits 64 .. ----
// BFINAL = 0 and BTYPE = 2; HLIT <= 29 and HDIST <= 29 (Deflate64: any HDIST, it has 32 distance codes); the HCLEN + 4 lengths of the code-length
// code exactly complete by their Kraft sum.
ZINF_HD bool infp_filter(uint64_t lo, uint64_t hi, bool d64 = false) {
  if ((lo & 7u) != 4u) return false;
  if (((lo >> 3) & 31u) > 29u || (!d64 && ((lo >> 8) & 31u) > 29u)) return false;
  const uint32_t ncl = (uint32_t)((lo >> 13) & 15u) + 4u;
  // the lengths from bit 17 on: 15 of them in lo (bits 17 .. 61), the rest from bit 62
  uint32_t kraft = 0;
  for (uint32_t i = 0; i < ncl; i++) {
    const uint32_t at = 17u + 3u * i;
    const uint32_t l = at + 3u <= 64u ? (uint32_t)(lo >> at) & 7u : at >= 64u ? (uint32_t)(hi >> (at - 64u)) & 7u : (uint32_t)((lo >> at) | (hi << (64u - at))) & 7u;
    if (l) kraft += 128u >> l;
  }
  return kraft == 128u;
}

// the scout's (and the decode's) stop rule, asked after every block's end
ZINF_HD bool infp_stop(bool final, uint64_t bitpos, uint64_t stop_bits) { return final || bitpos >= stop_bits; }

// ---- marker arithmetic: base = output position of the chunk's first byte, sp < base = the position a match reads ----
template <int FORMAT = 8> ZINF_HD uint32_t infp_marker(uint64_t base, uint64_t sp) { return InfpFmt<FORMAT>::MARK | (uint32_t)(base - 1u - sp); }
template <int FORMAT = 8> ZINF_HD uint64_t infp_marker_source(uint64_t base, uint32_t sym) { return base - 1u - (uint64_t)(sym & (InfpFmt<FORMAT>::WINDOW - 1u)); }

// a reader R (zada_inflate_logic.h) that stands at `bit`; Env::reopen (br, byte) opens it at a byte
template <class R, class Env> ZINF_HD void infp_seek(R &br, Env &env, uint64_t bit) {
  env.reopen(br, bit >> 3);
  br.need32();
  br.drop((uint32_t)(bit & 7u));
}

// is a dynamic, non-final block's whole header valid at the reader's position?  (every rule of inf_dynamic_header)
template <class R> ZINF_HD bool infp_candidate(R &br, InfTables &T, uint32_t lane, uint32_t nl, bool d64 = false) {
  br.need32();
  const uint32_t hdr = (uint32_t)br.hold & 7u;
  br.drop(3);
  if (hdr != 4u) return false;
  return inf_dynamic_header(br, T, d64, lane, nl) == INF_OK && !br.overrun();
}

// Blocks from the reader's position to the first block end where infp_stop says so.  Env takes what they hold:
//   env.stored (at, len): len bytes of the input from byte `at`; env.token (len, dist, val): a literal `val` (dist = 0, len = 1) or a match;
//   both return an InfRule; env.reopen (br, byte).
// Returns the InfRule broken; final: the last block was the stream's.
template <class R, class Env> ZINF_HD uint32_t infp_blocks(R &br, InfTables &T, uint64_t n_in, uint64_t stop_bits, uint32_t lane, uint32_t nl, Env &env, uint32_t &final,
                                                      bool d64 = false) {
  int loaded = INF_TAB_NONE;
  final = 0;
  for (;;) {
    br.need32();
    const uint32_t hdr = (uint32_t)br.hold & 7u;
    br.drop(3);
    if (br.overrun()) return INF_R_TRUNCATED;
    const uint32_t type = hdr >> 1;
    if (type == 3) return INF_R_BLOCK_TYPE;
    if (type == 0) {
      uint64_t at = (br.used_bits() + 7) / 8;
      if (at + 4 > n_in) return INF_R_TRUNCATED;
      br.hold = 0; br.nb = 0; br.ip = at;
      br.need32();
      const uint32_t w = (uint32_t)br.hold;
      const uint32_t len = w & 0xFFFFu, nlen = w >> 16;
      if (len != (nlen ^ 0xFFFFu)) return INF_R_STORED_LEN;
      at += 4;
      if (at + len > n_in) return INF_R_TRUNCATED;
      const uint32_t rule = env.stored(at, len);
      if (rule) return rule;
      env.reopen(br, at + len);
    } else {
      if (type == 1) {
        if (loaded != INF_TAB_FIXED) {
          inf_fixed_lengths(T, lane, nl);
          inf_build(T, INF_T_LIT, T.lens, INF_NLIT, lane, nl);
          inf_build(T, INF_T_DIST, T.lens + INF_NLIT, INF_NDIST, lane, nl);
        }
        loaded = INF_TAB_FIXED;
      } else {
        loaded = INF_TAB_DYNAMIC;
        const uint32_t rule = inf_dynamic_header(br, T, d64, lane, nl);
        if (rule) return rule;
      }
      for (;;) {
        uint32_t a = 0, b = 0;
        const int32_t k = inf_token(br, T, d64, a, b);
        if (k < 0) return (uint32_t)-k;
        if (br.overrun()) return INF_R_TRUNCATED;
        if (k == 2) break;
        const uint32_t rule = k == 1 ? env.token(a, b, 0u) : env.token(1u, 0u, a);
        if (rule) return rule;
      }
    }
    if (hdr & 1u) { final = 1; return INF_OK; }
    if (infp_stop(false, br.used_bits(), stop_bits)) return INF_OK;
  }
}

// ---- the chain ----
// infp_walk goes on from where it stood: W.cur is the chunk to take, W.expect the bit it has to start at.  Returns
//   INFP_W_DONE   : the chain reached the final block; live [k], off [k] and W.total are set;
//   INFP_W_REPAIR : chunk W.cur has to be scouted again from the exact start W.expect (a finder miss -- a fixed, stored or final block there --,
//                   a false positive, or a dead chunk); call again with its new record;
//   INFP_W_DAMAGED: a live chunk broke a rule, or the input ran out before a final block.
enum { INFP_W_DONE = 0, INFP_W_REPAIR = 1, INFP_W_DAMAGED = 2 };
struct InfpWalk { uint32_t cur = 0, live = 0, repairs = 0, last = 0; uint64_t expect = 0, total = 0; };
inline int infp_walk(InfpWalk &W, const InfpRec *recs, uint32_t nchunks, uint64_t chunk_bits, uint8_t *live, uint64_t *off) {
  for (;;) {
    const InfpRec &R = recs[W.cur];
    if (!(R.flags & INFP_F_FOUND) || R.start_bit != W.expect) {
      if (R.flags & INFP_F_EXACT) return INFP_W_DAMAGED;          // (a repaired chunk starts where it was told to: not reached)
      W.repairs++;
      return INFP_W_REPAIR;
    }
    live[W.cur] = 1; off[W.cur] = W.total; W.live++; W.last = W.cur;
    if (R.rule) return INFP_W_DAMAGED;
    W.total += R.bytes;
    if (R.flags & INFP_F_FINAL) return INFP_W_DONE;
    const uint64_t next = R.end_bit / chunk_bits;
    if (next <= W.cur || next >= nchunks) return INFP_W_DAMAGED;  // (the stop rule puts the end beyond the chunk; beyond the input: it ran out)
    W.cur = (uint32_t)next; W.expect = R.end_bit;
  }
}
// the repairs one stream may take before it goes to the one-wave decoder: a share of its chunks, and INFP_REPAIR_FLOOR
ZINF_HD uint64_t infp_repair_bound(uint64_t nchunks, uint32_t pct) { return nchunks * pct / 100u + INFP_REPAIR_FLOOR; }

}  // namespace zada
