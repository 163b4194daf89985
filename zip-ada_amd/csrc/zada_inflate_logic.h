// zada_inflate_logic.h -- the Inflate decoder (UnZip.Decompress.Inflate, unzip-decompress.adb:1463-1889; Zip formats 8 and 9), written once as
// host+device inline code with no HIP calls.  The kernel of zada_inflate.hip runs it with one wave per entry (tables and the staged input in
// LDS, every decision wave-uniform); tests/inflate/inflate_host.cpp compiles the same text into a CPU model with one "lane", so that every
// validity rule is tested -- also under ASan + UBSan -- on a machine without a GPU before a device sees a damaged stream.
//
// What is valid is what zlib's inflate.c / inftrees.c accept (raw stream, no dictionary); the rules are listed at InfRule.  Deflate64
// (format 9, unzip-decompress.adb:61, 148, 1859, 2035): length code 285 = 3 + 16 extra bits, distance codes 30 / 31 with 14 extra bits, 32
// distance codes in a dynamic header, a window of 64 KiB -- the window here is the entry's whole output, so only the codes differ.
//
// A reader type R gives the bits: need32 () -- at least 32 bits are in R.hold afterwards (the widest reader, a length code and its extra bits, takes 31), zeros behind the end of the input --, drop (k),
// used_bits (), overrun ().  Bits beyond the input decode as zeros and are found out by overrun () after every token:
// nothing is read beyond n_in, and a code word that needs a bit the input does not have is an error exactly when zlib would wait for more.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZINF_HD __host__ __device__ __forceinline__
#else
#define ZINF_HD inline
#endif
// wave-level points of the shared text: all lanes of the wave (the only one of its workgroup) meet; a value all lanes hold alike moves to the scalar side
#if defined(__HIP_DEVICE_COMPILE__)
#define ZINF_SYNC() __syncthreads()
#define ZINF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define ZINF_SYNC() ((void)0)
#define ZINF_UNI(x) ((uint32_t)(x))
#endif

// ZINF_STAT (x): the CPU model's counters of how symbols are found (tests/inflate/inflate_host.cpp defines it); nothing in the product
#ifndef ZINF_STAT
#define ZINF_STAT(x) ((void)0)
#endif

namespace zada {

// the rule a stream broke (zada_last_error names it with the bit position); every one of them is ZADA_E_DATA
enum InfRule {
  INF_OK = 0,
  INF_R_BLOCK_TYPE = 1,      // block type 3
  INF_R_STORED_LEN,          // stored block: LEN != ~NLEN
  INF_R_TOO_MANY_CODES,      // HLIT > 286 or HDIST > 30 (Deflate64: 32)
  INF_R_CL_CODE,             // code-length code over-subscribed or incomplete
  INF_R_REPEAT_FIRST,        // repeat code 16 with no previous length
  INF_R_REPEAT_LONG,         // a repeat runs past HLIT + HDIST
  INF_R_NO_END_OF_BLOCK,     // the length of symbol 256 is 0
  INF_R_LIT_CODE,            // literal/length code over-subscribed or incomplete (other than one code of length 1)
  INF_R_DIST_CODE,           // distance code over-subscribed or incomplete (other than one code of length 1, or none)
  INF_R_BAD_SYMBOL,          // literal/length symbol 286 / 287, Deflate: distance symbol 30 / 31
  INF_R_UNASSIGNED_CODE,     // a bit pattern no symbol has
  INF_R_DISTANCE_TOO_FAR,    // a distance beyond the bytes written so far
  INF_R_TRUNCATED,           // input exhausted before the final block's end-of-block
  INF_R_OUTPUT_FULL,         // output beyond cap
  INF_R_EMPTY_INPUT,         // n_in = 0
  INF_NRULES
};
ZINF_HD const char *inf_rule_name(uint32_t r) {
  switch (r) {
    case INF_OK: return "ok";
    case INF_R_BLOCK_TYPE: return "block type 3";
    case INF_R_STORED_LEN: return "stored block: LEN is not the complement of NLEN";
    case INF_R_TOO_MANY_CODES: return "too many literal/length or distance codes";
    case INF_R_CL_CODE: return "code-length code over-subscribed or incomplete";
    case INF_R_REPEAT_FIRST: return "repeat code 16 with no previous length";
    case INF_R_REPEAT_LONG: return "a repeat runs past HLIT + HDIST";
    case INF_R_NO_END_OF_BLOCK: return "no code for end-of-block";
    case INF_R_LIT_CODE: return "literal/length code over-subscribed or incomplete";
    case INF_R_DIST_CODE: return "distance code over-subscribed or incomplete";
    case INF_R_BAD_SYMBOL: return "symbol outside the format";
    case INF_R_UNASSIGNED_CODE: return "unassigned code";
    case INF_R_DISTANCE_TOO_FAR: return "distance beyond the bytes written so far";
    case INF_R_TRUNCATED: return "input exhausted before the final block's end-of-block";
    case INF_R_OUTPUT_FULL: return "output beyond cap";
    case INF_R_EMPTY_INPUT: return "empty input";
    default: return "?";
  }
}

constexpr int INF_LIT_BITS = 10, INF_DIST_BITS = 8, INF_CL_BITS = 7;     // primary lookup tables: 1024 + 256 entries of 2 bytes
constexpr int INF_NLIT = 288, INF_NDIST = 32;
enum { INF_T_LIT = 0, INF_T_DIST = 1, INF_T_CL = 2 };                     // (the code-length code borrows the distance code's rooms)
enum { INF_TAB_NONE = 0, INF_TAB_FIXED = 1, INF_TAB_DYNAMIC = 2 };

// Code tables of one entry in flight: 3 648 bytes (in LDS on the device).  A primary entry is (symbol << 4) | code length, 0 = this bit
// pattern is no complete short code: a longer code (walked canonically through cnt / sym, bit by bit) or an unassigned one.
struct InfTables {
  uint16_t lit[1 << INF_LIT_BITS];
  uint16_t dist[1 << INF_DIST_BITS];
  uint16_t sym[INF_NLIT + INF_NDIST];      // symbols in canonical order: literal/length from 0, distance (or code-length code) from 288
  uint16_t cnt[2][16];                     // codes per length
  uint16_t first[2][16];                   // first canonical code of a length
  uint16_t offs[2][16];                    // where a length's symbols start in sym (relative to the code's part of it)
  uint8_t lens[INF_NLIT + INF_NDIST];      // code lengths as the header gives them: HLIT of them, then HDIST
  uint8_t cl[20];                          // lengths of the code-length code
  uint32_t total[2];                       // codes in all
  uint32_t status;                         // what the lane that counted found (an InfRule), for all lanes
};

ZINF_HD uint32_t inf_bitrev(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; i++) { r = (r << 1) | (code & 1u); code >>= 1; }
  return r;
}

// Canonical code of n lengths: counts, Kraft sum, symbols in order (one lane: a few hundred steps), then the primary table filled by all
// `nl` lanes, one symbol of the sorted order each at a time.  inftrees.c: over-subscribed is an error; incomplete is an error unless the
// code is one code of length 1 (never for the code-length code) or, for the distance code only, empty.
ZINF_HD uint32_t inf_build(InfTables &T, int which, const uint8_t *lens, uint32_t n, uint32_t lane, uint32_t nl) {
  const int h = which == INF_T_LIT ? 0 : 1;
  uint16_t *tab = which == INF_T_LIT ? T.lit : T.dist;
  const uint32_t bits = which == INF_T_LIT ? INF_LIT_BITS : which == INF_T_DIST ? INF_DIST_BITS : INF_CL_BITS;
  uint16_t *sym = T.sym + (h ? INF_NLIT : 0);
  ZINF_SYNC();
  if (lane == 0) {
    for (int l = 0; l < 16; l++) T.cnt[h][l] = 0;
    for (uint32_t i = 0; i < n; i++) T.cnt[h][lens[i]]++;
    int32_t left = 1;
    uint32_t mx = 0, rule = INF_OK;
    const uint32_t bad = which == INF_T_LIT ? INF_R_LIT_CODE : which == INF_T_DIST ? INF_R_DIST_CODE : INF_R_CL_CODE;
    for (int l = 1; l < 16; l++) {
      left = left * 2 - (int32_t)T.cnt[h][l];
      if (left < 0) { rule = bad; break; }
      if (T.cnt[h][l]) mx = l;
    }
    if (!rule && left > 0) {                                     // incomplete
      if (mx == 0) { if (which != INF_T_DIST && which != INF_T_CL) rule = bad; }      // no code at all: inftrees.c builds a table of invalid entries
      else if (which == INF_T_CL || mx != 1) rule = bad;
    }
    if (!rule) {
      uint32_t code = 0, o = 0;
      for (int l = 1; l < 16; l++) { T.first[h][l] = (uint16_t)code; T.offs[h][l] = (uint16_t)o; code = (code + T.cnt[h][l]) << 1; o += T.cnt[h][l]; }
      T.first[h][0] = T.offs[h][0] = 0;
      for (uint32_t i = 0; i < n; i++) if (lens[i]) sym[T.offs[h][lens[i]]++] = (uint16_t)i;
      for (int l = 1; l < 16; l++) T.offs[h][l] = (uint16_t)(T.offs[h][l] - T.cnt[h][l]);
      T.total[h] = o;
    }
    T.status = rule;
  }
  ZINF_SYNC();
  for (uint32_t k = lane; k < (1u << bits); k += nl) tab[k] = 0;
  ZINF_SYNC();
  const uint32_t rule = ZINF_UNI(T.status);
  if (!rule) {
    const uint32_t total = ZINF_UNI(T.total[h]);
    for (uint32_t k = lane; k < total; k += nl) {
      const uint32_t s = sym[k], l = lens[s];
      if (l > bits) continue;
      const uint32_t rev = inf_bitrev(T.first[h][l] + (k - T.offs[h][l]), l);
      for (uint32_t j = rev; j < (1u << bits); j += 1u << l) tab[j] = (uint16_t)((s << 4) | l);
    }
  }
  ZINF_SYNC();
  return rule;
}

// One symbol: the primary table, or the canonical walk for codes longer than it (and the patterns no symbol has).  -1: unassigned code.
template <class R> ZINF_HD int32_t inf_symbol(R &br, const InfTables &T, int which) {
  const int h = which == INF_T_LIT ? 0 : 1;
  const uint16_t *tab = which == INF_T_LIT ? T.lit : T.dist;
  const uint32_t bits = which == INF_T_LIT ? INF_LIT_BITS : which == INF_T_DIST ? INF_DIST_BITS : INF_CL_BITS;
  const uint32_t e = ZINF_UNI(tab[(uint32_t)br.hold & ((1u << bits) - 1u)]);
  if (e) { ZINF_STAT(0); br.drop(e & 15u); return (int32_t)(e >> 4); }
  ZINF_STAT(1);
  const uint16_t *sym = T.sym + (h ? INF_NLIT : 0);
  uint32_t code = 0, first = 0, index = 0, w = (uint32_t)br.hold;
  for (uint32_t l = 1; l < 16; l++) {
    code |= w & 1u; w >>= 1;
    const uint32_t count = ZINF_UNI(T.cnt[h][l]);
    if (code < first + count) { br.drop(l); return (int32_t)ZINF_UNI(sym[index + (code - first)]); }
    index += count; first = (first + count) << 1; code <<= 1;
  }
  return -1;
}

ZINF_HD void inf_length_code(uint32_t s, bool d64, uint32_t &base, uint32_t &extra) {          // s = 257 .. 285
  const uint32_t c = s - 257u;
  if (c < 8u) { base = 3u + c; extra = 0; }
  else if (c == 28u) { base = d64 ? 3u : 258u; extra = d64 ? 16u : 0u; }
  else { extra = (c >> 2) - 1u; base = 3u + ((4u + (c & 3u)) << extra); }
}
ZINF_HD void inf_distance_code(uint32_t d, uint32_t &base, uint32_t &extra) {                 // d = 0 .. 31 (30, 31: Deflate64)
  if (d < 4u) { base = 1u + d; extra = 0; }
  else { extra = (d >> 1) - 1u; base = 1u + ((2u + (d & 1u)) << extra); }
}

// the lengths of the fixed codes into T.lens (HLIT = 288, HDIST = 32), lane by lane
ZINF_HD void inf_fixed_lengths(InfTables &T, uint32_t lane, uint32_t nl) {
  ZINF_SYNC();
  for (uint32_t i = lane; i < (uint32_t)(INF_NLIT + INF_NDIST); i += nl) T.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
  ZINF_SYNC();
}

// A dynamic block's header up to its three tables.  Returns an InfRule.
template <class R> ZINF_HD uint32_t inf_dynamic_header(R &br, InfTables &T, bool d64, uint32_t lane, uint32_t nl) {
  br.need32();
  const uint32_t w = (uint32_t)br.hold;
  const uint32_t nlen = (w & 31u) + 257u, ndist = ((w >> 5) & 31u) + 1u, ncl = ((w >> 10) & 15u) + 4u;
  br.drop(14);
  if (nlen > 286u || ndist > (d64 ? 32u : 30u)) return INF_R_TOO_MANY_CODES;
  ZINF_SYNC();
  if (lane < 19u) T.cl[lane] = 0;
  if (nl == 1) for (uint32_t i = 1; i < 19u; i++) T.cl[i] = 0;
  ZINF_SYNC();
  for (uint32_t i = 0; i < ncl; i++) {
    if ((i & 7u) == 0) br.need32();
    // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    const uint32_t at = i < 3 ? 16u + i : i == 3 ? 0u : (i & 1u) ? 7u - ((i - 5u) >> 1) : 8u + ((i - 4u) >> 1);
    if (lane == 0) T.cl[at] = (uint8_t)((uint32_t)br.hold & 7u);
    br.drop(3);
  }
  uint32_t rule = inf_build(T, INF_T_CL, T.cl, 19, lane, nl);
  if (rule) return rule;
  const bool cl_empty = ZINF_UNI(T.total[1]) == 0;
  uint32_t have = 0, prev = 0;
  const uint32_t want = nlen + ndist;
  while (have < want) {
    br.need32();
    const int32_t s = inf_symbol(br, T, INF_T_CL);
    if (s < 0) {
      // a code-length code with no code at all (every length 0) reads as length 0, one bit at a time (inflate.c takes val of inftrees.c's invalid entry)
      if (cl_empty) { br.drop(1); if (lane == 0) T.lens[have] = 0; have++; prev = 0; continue; }
      return INF_R_UNASSIGNED_CODE;
    }
    if (s < 16) { if (lane == 0) T.lens[have] = (uint8_t)s; have++; prev = (uint32_t)s; continue; }
    uint32_t rep, val = 0;
    if (s == 16) { if (have == 0) return INF_R_REPEAT_FIRST; val = prev; rep = 3u + ((uint32_t)br.hold & 3u); br.drop(2); }
    else if (s == 17) { rep = 3u + ((uint32_t)br.hold & 7u); br.drop(3); }
    else { rep = 11u + ((uint32_t)br.hold & 127u); br.drop(7); }
    if (have + rep > want) return INF_R_REPEAT_LONG;
    if (lane == 0) for (uint32_t j = 0; j < rep; j++) T.lens[have + j] = (uint8_t)val;
    have += rep; prev = val;
  }
  if (br.overrun()) return INF_R_TRUNCATED;
  ZINF_SYNC();
  if (ZINF_UNI(T.lens[256]) == 0) return INF_R_NO_END_OF_BLOCK;
  rule = inf_build(T, INF_T_LIT, T.lens, nlen, lane, nl);
  if (rule) return rule;
  return inf_build(T, INF_T_DIST, T.lens + nlen, ndist, lane, nl);
}

// One token.  Returns 0: literal `a`; 1: match of length `a` at distance `b`; 2: end of block; otherwise -(InfRule).
template <class R> ZINF_HD int32_t inf_token(R &br, const InfTables &T, bool d64, uint32_t &a, uint32_t &b) {
  br.need32();
  int32_t s = inf_symbol(br, T, INF_T_LIT);
  if (s < 0) return -(int32_t)INF_R_UNASSIGNED_CODE;
  if (s < 256) { a = (uint32_t)s; return 0; }
  if (s == 256) return 2;
  if (s > 285) return -(int32_t)INF_R_BAD_SYMBOL;
  uint32_t base, extra;
  inf_length_code((uint32_t)s, d64, base, extra);
  a = base + ((uint32_t)br.hold & ((1u << extra) - 1u));
  br.drop(extra);
  br.need32();
  s = inf_symbol(br, T, INF_T_DIST);
  if (s < 0) return -(int32_t)INF_R_UNASSIGNED_CODE;
  if (s > (d64 ? 31 : 29)) return -(int32_t)INF_R_BAD_SYMBOL;
  inf_distance_code((uint32_t)s, base, extra);
  b = base + ((uint32_t)br.hold & ((1u << extra) - 1u));
  br.drop(extra);
  return 1;
}

// what a decoder leaves per entry
struct InfResult {
  int32_t rc;                 // 0, or ZADA_E_DATA (-7)
  uint32_t rule;              // the InfRule broken
  uint64_t out_len;           // bytes written (0 unless rc = 0)
  uint64_t in_used;           // bytes up to and including the one that holds the last bit of the final block (0 unless rc = 0)
  uint64_t bitpos;            // where the decoder stood when it gave up
  uint32_t crc, pad;          // the CRC-32 register behind the output (k_inf_crc)
};
constexpr int32_t INF_E_DATA = -7;

// ---- the reader of the CPU model, and the whole decoder with one lane ----
struct InfHostReader {
  const uint8_t *in; uint64_t n, ip; uint64_t hold; uint32_t nb;
  ZINF_HD void open(const uint8_t *p, uint64_t len, uint64_t at) { in = p; n = len; ip = at; hold = 0; nb = 0; }
  ZINF_HD void need32() {
    if (nb > 32) return;
    uint32_t w = 0;
    for (int k = 0; k < 4; k++) if (ip + k < n) w |= (uint32_t)in[ip + k] << (8 * k);
    hold |= (uint64_t)w << nb; nb += 32; ip += 4;
  }
  ZINF_HD void drop(uint32_t k) { hold >>= k; nb -= k; }
  ZINF_HD uint64_t used_bits() const { return ip * 8 - nb; }
  ZINF_HD bool overrun() const { return used_bits() > n * 8; }
};

ZINF_HD void inf_fail(InfResult &res, uint32_t rule, uint64_t bitpos) { res.rc = INF_E_DATA; res.rule = rule; res.out_len = 0; res.in_used = 0; res.bitpos = bitpos; }

inline void inf_serial(int format, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, InfTables &T, InfResult &res) {
  const bool d64 = format == 9;
  res.rc = 0; res.rule = 0; res.out_len = 0; res.in_used = 0; res.bitpos = 0; res.crc = 0; res.pad = 0;
  if (n_in == 0) { inf_fail(res, INF_R_EMPTY_INPUT, 0); return; }
  InfHostReader br;
  br.open(in, n_in, 0);
  uint64_t pos = 0;
  int loaded = INF_TAB_NONE;
  for (;;) {
    br.need32();
    const uint32_t hdr = (uint32_t)br.hold & 7u;
    br.drop(3);
    if (br.overrun()) { inf_fail(res, INF_R_TRUNCATED, br.used_bits()); return; }
    const uint32_t type = hdr >> 1;
    if (type == 3) { inf_fail(res, INF_R_BLOCK_TYPE, br.used_bits()); return; }
    if (type == 0) {
      uint64_t at = (br.used_bits() + 7) / 8;
      if (at + 4 > n_in) { inf_fail(res, INF_R_TRUNCATED, at * 8); return; }
      const uint32_t len = in[at] | (uint32_t)in[at + 1] << 8, nlen = in[at + 2] | (uint32_t)in[at + 3] << 8;
      if (len != (nlen ^ 0xFFFFu)) { inf_fail(res, INF_R_STORED_LEN, at * 8); return; }
      at += 4;
      if (pos + len > cap) { inf_fail(res, INF_R_OUTPUT_FULL, at * 8); return; }
      if (at + len > n_in) { inf_fail(res, INF_R_TRUNCATED, at * 8); return; }
      for (uint32_t i = 0; i < len; i++) out[pos + i] = in[at + i];
      pos += len;
      br.open(in, n_in, at + len);
    } else {
      if (type == 1) {
        if (loaded != INF_TAB_FIXED) { inf_fixed_lengths(T, 0, 1); inf_build(T, INF_T_LIT, T.lens, INF_NLIT, 0, 1); inf_build(T, INF_T_DIST, T.lens + INF_NLIT, INF_NDIST, 0, 1); }
        loaded = INF_TAB_FIXED;
      } else {
        loaded = INF_TAB_DYNAMIC;
        const uint32_t rule = inf_dynamic_header(br, T, d64, 0, 1);
        if (rule) { inf_fail(res, rule, br.used_bits()); return; }
      }
      for (;;) {
        uint32_t a = 0, b = 0;
        const int32_t k = inf_token(br, T, d64, a, b);
        if (k < 0) { inf_fail(res, (uint32_t)-k, br.used_bits()); return; }
        if (br.overrun()) { inf_fail(res, INF_R_TRUNCATED, br.used_bits()); return; }
        if (k == 2) break;
        if (k == 0) {
          if (pos + 1 > cap) { inf_fail(res, INF_R_OUTPUT_FULL, br.used_bits()); return; }
          out[pos++] = (uint8_t)a;
        } else {
          if (b > pos) { inf_fail(res, INF_R_DISTANCE_TOO_FAR, br.used_bits()); return; }
          if (pos + a > cap) { inf_fail(res, INF_R_OUTPUT_FULL, br.used_bits()); return; }
          for (uint32_t i = 0; i < a; i++) out[pos + i] = out[pos - b + i];
          pos += a;
        }
      }
    }
    if (hdr & 1u) break;
  }
  res.out_len = pos;
  res.in_used = (br.used_bits() + 7) / 8;
  res.bitpos = br.used_bits();
}

}  // namespace zada
