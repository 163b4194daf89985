// zada_unlzma_logic.h -- the LZMA decoder (LZMA.Decoding.Decode, lzma-decoding.adb, as UnZip.Decompress.LZMA_Decode calls it for Zip format 14,
// unzip-decompress.adb:1917-1940), written once as host+device inline code with no HIP calls.  The kernel of zada_unlzma.hip runs it with one
// wave per entry (every decision wave-uniform, the model in LDS / HBM, the window = the entry's output); tests/unlzma/unlzma_host.cpp compiles
// the same text into a CPU model with one "lane", so that every validity rule is tested -- also under ASan + UBSan -- on a machine without a
// GPU before a device sees a damaged stream.
//
// Input: the Zip payload of a method-14 entry -- 2 bytes SDK version (ignored), 2 bytes properties size (5), the properties (lc / lp / pb in
// one byte d < 225, the dictionary size as a little-endian u32), the range-coded stream.  Per entry: eos = bit 1 of the general-purpose flags
// (the reference's marker_expected), cap = the directory's uncompressed size (given_size with has_size => False).  What is valid is what
// Decode accepts with (has_size => False, given_size => cap, marker_expected => eos, fail_on_bad_range_code => True); the rules are at UlzRule.
//
// The normalisation is the reference's: right behind every bit (liblzma normalises in front of the next bit and once more at the end, so both
// have consumed the same bytes wherever a stream ends).  A byte beyond n_in reads as 0 and is found out at the next check of io.over, at the
// latest behind the token that needed it: a stream that needs a byte it does not have is not valid (where liblzma would wait for more).
//
// An IO type gives the surroundings: byte () -- the next input byte, 0 and over = true beyond the input --, ip (bytes taken), pget / pset (the
// 1846 probabilities that are no literal's), lget / lset (the literal table, 0x300 << (lc + lp)), put (pos, b) -- a literal --, peek (pos,
// dist) -- the byte dist behind pos --, copy (pos, dist, len) -- a match, returns its last byte.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ULZ_HD __host__ __device__ __forceinline__
#else
#define ULZ_HD inline
#endif

namespace zada {

// the rule a stream broke, in the order the reference meets them (zada_last_error names it with the input byte); every one is ZADA_E_DATA
enum UlzRule {
  ULZ_OK = 0,
  ULZ_R_PROPERTIES = 1,      // R1: properties size not 5, or properties byte >= 225 ("Incorrect LZMA properties")
  ULZ_R_OUTPUT_FULL,         // R2: a literal, a match or a rep match with cap bytes written, or a match that runs past cap
  ULZ_R_DISTANCE,            // R3: not rep0 < min (dict_size, bytes written), dict_size raised to Min_dictionary_size = 4096
  ULZ_R_EMPTY_WINDOW,        // R4: a rep match with no byte written yet
  ULZ_R_MARKER,              // R5: the marker (distance 0xFFFFFFFF of a simple match) with code /= 0: "range decoder not finished on marker"
  ULZ_R_NO_MARKER,           // R6: (never raised by itself: with eos = 1 a stream without marker runs into R2 or R8) kept for the numbering
  ULZ_R_RANGE_CORRUPTED,     // R7: first range-coder byte not 0, code = range after the initial load or inside the direct bits; refused at the end
  ULZ_R_INPUT_END,           // R8: the input ends before one of the ends
  ULZ_NRULES
};
ULZ_HD const char *ulz_rule_name(uint32_t r) {
  switch (r) {
    case ULZ_OK: return "ok";
    case ULZ_R_PROPERTIES: return "incorrect LZMA properties";
    case ULZ_R_OUTPUT_FULL: return "output beyond cap";
    case ULZ_R_DISTANCE: return "invalid distance";
    case ULZ_R_EMPTY_WINDOW: return "rep match with an empty window";
    case ULZ_R_MARKER: return "range decoder not finished on marker";
    case ULZ_R_NO_MARKER: return "end without the marker the flags promise";
    case ULZ_R_RANGE_CORRUPTED: return "range decoder had a corrupted value";
    case ULZ_R_INPUT_END: return "input exhausted before the end of the stream";
    default: return "?";
  }
}
enum { ULZ_END_NONE = 0, ULZ_END_MARKER = 1, ULZ_END_NO_MARKER = 2, ULZ_END_FORK = 3 };   // _FORK: stopped between two symbols (ulz_decode_f)

// the probabilities that are no literal's: 1846 of them
constexpr uint32_t ULZ_IS_MATCH = 0;                          // [12][16]
constexpr uint32_t ULZ_IS_REP = ULZ_IS_MATCH + 192;           // [12]
constexpr uint32_t ULZ_REP_G0 = ULZ_IS_REP + 12;
constexpr uint32_t ULZ_REP_G1 = ULZ_REP_G0 + 12;
constexpr uint32_t ULZ_REP_G2 = ULZ_REP_G1 + 12;
constexpr uint32_t ULZ_REP0_LONG = ULZ_REP_G2 + 12;           // [12][16]
constexpr uint32_t ULZ_SLOT = ULZ_REP0_LONG + 192;            // [4][64]
constexpr uint32_t ULZ_SPEC = ULZ_SLOT + 256;                 // 114: pos_coder, reached as ULZ_SPEC - 1 + dist - slot + m with m >= 1
constexpr uint32_t ULZ_ALIGN = ULZ_SPEC + 114;                // [16]
constexpr uint32_t ULZ_LEN = ULZ_ALIGN + 16;                  // choice_1, choice_2, low [16][8], mid [16][8], high [256]
constexpr uint32_t ULZ_LEN_SIZE = 2 + 128 + 128 + 256;
constexpr uint32_t ULZ_REP_LEN = ULZ_LEN + ULZ_LEN_SIZE;
constexpr uint32_t ULZ_NPROBS = ULZ_REP_LEN + ULZ_LEN_SIZE;   // 1846
static_assert(ULZ_NPROBS == 1846, "the model without its literal table");
constexpr uint32_t ULZ_PROB_INIT = 1024;
constexpr uint32_t ULZ_MIN_DICT = 1u << 12;                   // Min_dictionary_size, lzma.ads:209
constexpr uint32_t ULZ_LIT_LDS_MAX = 0x300u << 3;             // lc + lp <= 3: the literal table fits the wave's LDS

// what a decoder leaves per entry
struct UlzResult {
  int32_t rc;                 // 0, or ZADA_E_DATA (-7)
  uint32_t rule;              // the UlzRule broken
  uint64_t out_len;           // bytes written (0 unless rc = 0)
  uint64_t in_used;           // bytes through the last one the normalisation consumed (0 unless rc = 0)
  uint64_t in_pos, out_pos;   // where the decoder stood when it ended or gave up
  uint32_t crc, end;          // the CRC-32 register behind the output; ULZ_END_*
};
constexpr int32_t ULZ_E_DATA = -7;

struct UlzRc { uint32_t range, code, corrupted; };

template <class IO> ULZ_HD void ulz_norm(IO &io, UlzRc &rc) {
  if (rc.range < (1u << 24)) { rc.range <<= 8; rc.code = (rc.code << 8) | io.byte(); }
}
// Decode_Bit; LIT: the probability is one of the literal table
template <bool LIT, class IO> ULZ_HD uint32_t ulz_bit(IO &io, UlzRc &rc, uint32_t idx) {
  const uint32_t p = LIT ? io.lget(idx) : io.pget(idx);
  const uint32_t bound = (rc.range >> 11) * p;
  uint32_t sym, np;
  if (rc.code < bound) { np = p + ((2048u - p) >> 5); rc.range = bound; sym = 0; }
  else { np = p - (p >> 5); rc.code -= bound; rc.range -= bound; sym = 1; }
  if (LIT) io.lset(idx, np); else io.pset(idx, np);
  ulz_norm(io, rc);
  return sym;
}
template <class IO> ULZ_HD uint32_t ulz_tree(IO &io, UlzRc &rc, uint32_t base, uint32_t bits) {
  uint32_t m = 1;
  for (uint32_t i = 0; i < bits; i++) m = 2 * m + ulz_bit<false>(io, rc, base + m);
  return m - (1u << bits);
}
template <class IO> ULZ_HD uint32_t ulz_tree_rev(IO &io, UlzRc &rc, uint32_t base, uint32_t bits) {
  uint32_t m = 1, v = 0;
  for (uint32_t i = 0; i < bits; i++) { const uint32_t b = ulz_bit<false>(io, rc, base + m); m = 2 * m + b; v |= b << i; }
  return v;
}
// Decode_Length: 0 .. 271 (the match is 2 longer)
template <class IO> ULZ_HD uint32_t ulz_len(IO &io, UlzRc &rc, uint32_t base, uint32_t pos_state) {
  if (ulz_bit<false>(io, rc, base) == 0) return ulz_tree(io, rc, base + 2 + pos_state * 8, 3);
  if (ulz_bit<false>(io, rc, base + 1) == 0) return 8 + ulz_tree(io, rc, base + 2 + 128 + pos_state * 8, 3);
  return 16 + ulz_tree(io, rc, base + 2 + 256, 8);
}
// Decode_Distance: rep0 (0xFFFFFFFF: the marker)
template <class IO> ULZ_HD uint32_t ulz_dist(IO &io, UlzRc &rc, uint32_t len) {
  const uint32_t slot = ulz_tree(io, rc, ULZ_SLOT + (len < 3 ? len : 3) * 64, 6);
  if (slot < 4) return slot;
  const uint32_t nd = (slot >> 1) - 1;
  uint32_t dist = (2u | (slot & 1u)) << nd;
  if (slot < 14) return dist | ulz_tree_rev(io, rc, ULZ_SPEC - 1 + dist - slot, nd);
  uint32_t dd = 0;
  for (uint32_t i = 0; i < nd - 4; i++) {
    rc.range >>= 1;
    rc.code -= rc.range;
    const uint32_t t = 0u - (rc.code >> 31);
    rc.code += rc.range & t;
    if (rc.code == rc.range) rc.corrupted = 1;
    ulz_norm(io, rc);
    dd = dd + dd + t + 1;
  }
  dist += dd << 4;
  return dist | ulz_tree_rev(io, rc, ULZ_ALIGN, 4);
}

ULZ_HD void ulz_fail(UlzResult &res, uint32_t rule, uint64_t in_pos, uint64_t out_pos) {
  res.rc = ULZ_E_DATA; res.rule = rule; res.out_len = 0; res.in_used = 0; res.in_pos = in_pos; res.out_pos = out_pos; res.end = ULZ_END_NONE;
}

// The header of the payload.  Returns a UlzRule; lit_elems: the entries of the literal table.
struct UlzProps { uint32_t lc, lp, pb, dict; };
ULZ_HD uint32_t ulz_props(const uint8_t *h9, uint64_t n_in, UlzProps &P) {
  if (n_in < 4) return ULZ_R_INPUT_END;
  if (h9[2] != 5 || h9[3] != 0) return ULZ_R_PROPERTIES;
  if (n_in < 9) return ULZ_R_INPUT_END;
  uint32_t d = h9[4];
  if (d >= 225) return ULZ_R_PROPERTIES;
  P.lc = d % 9; d /= 9; P.lp = d % 5; P.pb = d / 5;
  P.dict = (uint32_t)h9[5] | (uint32_t)h9[6] << 8 | (uint32_t)h9[7] << 16 | (uint32_t)h9[8] << 24;
  if (P.dict < ULZ_MIN_DICT) P.dict = ULZ_MIN_DICT;
  return ULZ_OK;
}
ULZ_HD uint64_t ulz_lit_elems(const UlzProps &P) { return (uint64_t)0x300 << (P.lc + P.lp); }

// The decoder between two symbols (Trained_Compression): everything Decode_Contents carries from one turn of its loop to the next, but
// the probability model and the window, which stay where the IO keeps them.  in_pos: input bytes taken, out_pos: bytes written.
struct UlzFork { uint32_t range, code, corrupted, state, rep0, rep1, rep2, rep3, prev, pad; uint64_t in_pos, out_pos; };
// where a decoder that may stop does so: at the first symbol boundary from which fewer than ULZ_FORK_MARGIN input bytes remain before in_limit, or
// the first one behind `symbols` symbols (a test's way to every boundary).  One symbol takes fewer than 64 bytes: at most 22 adaptive bits, each
// narrowing the range by less than 2 ** 7 (a probability stays within 31 .. 2017 of 2048), and 26 direct bits -- under 180 bits.
constexpr uint64_t ULZ_FORK_MARGIN = 64;
struct UlzStop { uint64_t in_limit, symbols; };

// Decode_Contents behind the nine header bytes (io stands at byte 9, the model is initialised).  res.crc is the caller's.
// FORK (Trained_Compression): start, when given, is a state to go on from in place of the initial one (io and the model are the caller's to set); with
// stop the decoder ends at the boundary UlzStop names, leaves its state in *fork and reports ULZ_END_FORK.  Without FORK none of this is compiled.
template <bool FORK, class IO> ULZ_HD void ulz_decode_f(IO &io, const UlzProps &P, uint64_t cap, uint32_t eos, UlzResult &res, const UlzFork *start, const UlzStop *stop,
                                                       UlzFork *fork) {
  const uint32_t lc = P.lc, lpm = (1u << P.lp) - 1u, pbm = (1u << P.pb) - 1u, dict = P.dict;
  UlzRc rc{0xFFFFFFFFu, 0u, 0u};
  uint32_t state = 0, rep0 = 0, rep1 = 0, rep2 = 0, rep3 = 0, prev = 0;
  uint64_t pos = 0, nsym = 0;
  res.rc = 0; res.rule = 0; res.out_len = 0; res.in_used = 0; res.in_pos = 0; res.out_pos = 0; res.end = ULZ_END_NONE;
#define ULZ_FAIL(r) do { ulz_fail(res, (r), io.ip, pos); return; } while (0)
#define ULZ_OVER() do { if (io.over) ULZ_FAIL(ULZ_R_INPUT_END); } while (0)
  bool resumed = false;
  if constexpr (FORK) {
    if (start) {
      rc.range = start->range; rc.code = start->code; rc.corrupted = start->corrupted;
      state = start->state; rep0 = start->rep0; rep1 = start->rep1; rep2 = start->rep2; rep3 = start->rep3; prev = start->prev; pos = start->out_pos;
      resumed = true;
    }
  }
  if (!resumed) {
    // Init
    if (io.byte() != 0) rc.corrupted = 1;
    for (int i = 0; i < 4; i++) rc.code = (rc.code << 8) | io.byte();
    ULZ_OVER();
    if (rc.code == rc.range) rc.corrupted = 1;
  }
  uint32_t end = ULZ_END_NONE;
  for (;;) {
    if constexpr (FORK) {
      if (stop && (io.ip + ULZ_FORK_MARGIN > stop->in_limit || nsym >= stop->symbols)) {
        *fork = UlzFork{rc.range, rc.code, rc.corrupted, state, rep0, rep1, rep2, rep3, prev, 0u, io.ip, pos};
        res.out_len = pos; res.in_used = io.ip; res.in_pos = io.ip; res.out_pos = pos; res.end = ULZ_END_FORK;
        return;
      }
      nsym++;
    }
    if (!eos && pos == cap && rc.code == 0) { end = ULZ_END_NO_MARKER; break; }
    const uint32_t ps = (uint32_t)pos & pbm;
    if (ulz_bit<false>(io, rc, ULZ_IS_MATCH + state * 16 + ps) == 0) {
      ULZ_OVER();
      if (pos == cap) ULZ_FAIL(ULZ_R_OUTPUT_FULL);
      const uint32_t base = 0x300u * ((((uint32_t)pos & lpm) << lc) + (prev >> (8 - lc)));
      uint32_t sym = 1;
      if (state >= 7) {
        uint32_t mb = io.peek(pos, (uint64_t)rep0 + 1);
        for (;;) {
          mb += mb;
          const uint32_t mbit = mb & 0x100u;
          const uint32_t b = ulz_bit<true>(io, rc, base + 0x100u + mbit + sym);
          sym = 2 * sym | b;
          if (sym >= 0x100u) break;
          if (mbit != (b << 8)) {
            while (sym < 0x100u) sym = 2 * sym | ulz_bit<true>(io, rc, base + sym);
            break;
          }
        }
      } else {
        while (sym < 0x100u) sym = 2 * sym | ulz_bit<true>(io, rc, base + sym);
      }
      ULZ_OVER();
      prev = sym - 0x100u;
      io.put(pos, prev);
      pos++;
      state = state < 4 ? 0 : state < 10 ? state - 3 : state - 6;
      continue;
    }
    uint32_t len;
    if (ulz_bit<false>(io, rc, ULZ_IS_REP + state) == 0) {
      rep3 = rep2; rep2 = rep1; rep1 = rep0;
      len = ulz_len(io, rc, ULZ_LEN, ps);
      state = state < 7 ? 7 : 10;
      rep0 = ulz_dist(io, rc, len);
      ULZ_OVER();
      if (rep0 == 0xFFFFFFFFu) {
        if (rc.code != 0) ULZ_FAIL(ULZ_R_MARKER);
        end = ULZ_END_MARKER;
        break;
      }
      if (pos == cap) ULZ_FAIL(ULZ_R_OUTPUT_FULL);
      if (!((uint64_t)rep0 < (pos < dict ? pos : (uint64_t)dict))) ULZ_FAIL(ULZ_R_DISTANCE);
    } else {
      ULZ_OVER();
      if (pos == cap) ULZ_FAIL(ULZ_R_OUTPUT_FULL);
      if (pos == 0) ULZ_FAIL(ULZ_R_EMPTY_WINDOW);
      if (ulz_bit<false>(io, rc, ULZ_REP_G0 + state) == 0) {
        if (ulz_bit<false>(io, rc, ULZ_REP0_LONG + state * 16 + ps) == 0) {
          ULZ_OVER();
          state = state < 7 ? 9 : 11;
          prev = io.peek(pos, (uint64_t)rep0 + 1);
          io.put(pos, prev);
          pos++;
          continue;
        }
      } else {
        uint32_t dist;
        if (ulz_bit<false>(io, rc, ULZ_REP_G1 + state) == 0) dist = rep1;
        else {
          if (ulz_bit<false>(io, rc, ULZ_REP_G2 + state) == 0) dist = rep2;
          else { dist = rep3; rep3 = rep2; }
          rep2 = rep1;
        }
        rep1 = rep0; rep0 = dist;
      }
      len = ulz_len(io, rc, ULZ_REP_LEN, ps);
      state = state < 7 ? 8 : 11;
      ULZ_OVER();
    }
    len += 2;
    if (pos + len > cap) ULZ_FAIL(ULZ_R_OUTPUT_FULL);
    prev = io.copy(pos, (uint64_t)rep0 + 1, len);
    pos += len;
  }
  if (rc.corrupted) ULZ_FAIL(ULZ_R_RANGE_CORRUPTED);
#undef ULZ_FAIL
#undef ULZ_OVER
  res.out_len = pos; res.in_used = io.ip; res.in_pos = io.ip; res.out_pos = pos; res.end = end;
}
template <class IO> ULZ_HD void ulz_decode(IO &io, const UlzProps &P, uint64_t cap, uint32_t eos, UlzResult &res) {
  ulz_decode_f<false>(io, P, cap, eos, res, nullptr, nullptr, nullptr);
}

// The five header bytes of a stream as LZMA.Encoding.Encode writes it with no size field (Trained_Compression: has_size => False).  Returns a UlzRule.
ULZ_HD uint32_t ulz_props5(const uint8_t *h5, uint64_t n_in, UlzProps &P) {
  if (n_in < 5) return ULZ_R_INPUT_END;
  uint32_t d = h5[0];
  if (d >= 225) return ULZ_R_PROPERTIES;
  P.lc = d % 9; d /= 9; P.lp = d % 5; P.pb = d / 5;
  P.dict = (uint32_t)h5[1] | (uint32_t)h5[2] << 8 | (uint32_t)h5[3] << 16 | (uint32_t)h5[4] << 24;
  if (P.dict < ULZ_MIN_DICT) P.dict = ULZ_MIN_DICT;
  return ULZ_OK;
}

// ---- the surroundings of the CPU model, and the whole decoder with one lane ----
struct UlzHostIO {
  const uint8_t *in; uint64_t n, ip; bool over;
  uint16_t *probs, *lit;
  uint8_t *out;
  uint32_t byte() { if (ip < n) return in[ip++]; over = true; return 0; }
  uint32_t pget(uint32_t i) const { return probs[i]; }
  void pset(uint32_t i, uint32_t v) { probs[i] = (uint16_t)v; }
  uint32_t lget(uint32_t i) const { return lit[i]; }
  void lset(uint32_t i, uint32_t v) { lit[i] = (uint16_t)v; }
  void put(uint64_t pos, uint32_t b) { out[pos] = (uint8_t)b; }
  uint32_t peek(uint64_t pos, uint64_t dist) const { return out[pos - dist]; }
  uint32_t copy(uint64_t pos, uint64_t dist, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) out[pos + i] = out[pos + i - dist];
    return out[pos + len - 1];
  }
};

// probs: ULZ_NPROBS values; lit: room for ulz_lit_elems of the entry's properties (the caller sizes it after ulz_props)
inline void ulz_serial(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint32_t eos, const UlzProps &P, uint16_t *probs, uint16_t *lit, UlzResult &res) {
  for (uint32_t i = 0; i < ULZ_NPROBS; i++) probs[i] = ULZ_PROB_INIT;
  const uint64_t nl = ulz_lit_elems(P);
  for (uint64_t i = 0; i < nl; i++) lit[i] = ULZ_PROB_INIT;
  UlzHostIO io{in, n_in, 9, false, probs, lit, out};
  ulz_decode(io, P, cap, eos, res);
}

}  // namespace zada
