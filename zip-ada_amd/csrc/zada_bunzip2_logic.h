// zada_bunzip2_logic.h -- the BZip2 decoder (BZip2.Decoding.Decompress, bzip2-decoding.adb; Zip format 12) up to a block's last column, written
// once as host+device inline code with no HIP calls.  k_bzd_block of zada_bunzip2.hip runs it with one wave per block (tables, the selectors and
// the MTF list in LDS, every decision wave-uniform); tests/bunzip2/bunzip2_host.cpp compiles the same text into a CPU model with one "lane"
// and runs every later stage (BWT_Detransform, the chase of RLE_1, the block CRC) as a plain serial loop behind it.
//
// What is valid is what libbz2 1.0.8 accepts (BZ2_bzDecompress, one stream).  The reference ports libbz2's decompress.c, so non-canonical and
// over-subscribed length sets decode alike in all three; where the reference's text is laxer than libbz2, libbz2 is followed:
// the randomised flag (a rule of its own), the origin (below the symbol count), the coder count (2 .. 6), the selector count (at least 1; those
// beyond 18 002 are read and dropped), a selector's MTF index (below the coder count), a code length (1 .. 20 at every step of its delta chain),
// input that ends before the footer's last bit, and both CRCs.
//
// A reader type R gives the bits, most significant first: bits (k), 1 <= k <= 24 -- zeros behind the end of the input --, used_bits (),
// overrun ().  Nothing is read beyond n_in; whatever a decoder finds wrong once it has taken a bit the input does not have is "input exhausted".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZBZD_HD __host__ __device__ __forceinline__
#else
#define ZBZD_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define ZBZD_SYNC() __syncthreads()
#define ZBZD_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define ZBZD_SYNC() ((void)0)
#define ZBZD_UNI(x) ((uint32_t)(x))
#endif

namespace zada {

// the rule a stream broke (zada_last_error names it with the block number and the bit position); every one of them is ZADA_E_DATA
enum BzdRule {
  BZD_OK = 0,
  BZD_R_STREAM_MAGIC = 1,     // the stream does not begin with BZh1 .. BZh9
  BZD_R_BLOCK_MAGIC,          // neither the block magic nor the footer magic where a block has to begin
  BZD_R_RANDOMISED,           // the randomised flag is set (no writer since bzip2 0.9.5 sets it; de-randomising is not built)
  BZD_R_ORIGIN,               // the origin is not below the block's symbol count (a block with no symbols has no valid origin)
  BZD_R_NO_BYTE_IN_USE,       // the mapping table names no byte value
  BZD_R_CODER_COUNT,          // entropy coder count outside 2 .. 6
  BZD_R_SELECTOR_COUNT,       // selector count 0
  BZD_R_SELECTOR_INDEX,       // a selector's MTF index is not below the coder count
  BZD_R_CODE_LENGTH,          // a code length outside 1 .. 20
  BZD_R_SELECTORS_EXHAUSTED,  // Get_MTF_Value: more groups of 50 symbols than selectors
  BZD_R_CODE_TOO_LONG,        // Get_MTF_Value [1]: no code of up to 20 bits matches
  BZD_R_CODE_VECTOR,          // Get_MTF_Value [2]: the code vector left the positive range
  BZD_R_PERM_INDEX,           // Get_MTF_Value [3]: the index into the permutation is outside 0 .. 257
  BZD_R_RUN_TOO_LONG,         // a RUNA / RUNB run of 2 Mi and more
  BZD_R_BLOCK_OVERFLOW,       // more symbols than 100 000 x level
  BZD_R_BLOCK_CRC,            // the block's CRC differs from the stored one
  BZD_R_STREAM_CRC,           // the combined CRC differs from the footer's
  BZD_R_TRUNCATED,            // input exhausted before the last bit of the footer's CRC
  BZD_R_OUTPUT_FULL,          // output beyond cap
  BZD_NRULES
};
ZBZD_HD const char *bzd_rule_name(uint32_t r) {
  switch (r) {
    case BZD_OK: return "ok";
    case BZD_R_STREAM_MAGIC: return "no BZh1 .. BZh9 stream header";
    case BZD_R_BLOCK_MAGIC: return "neither block nor footer magic";
    case BZD_R_RANDOMISED: return "randomised block";
    case BZD_R_ORIGIN: return "origin not below the block's symbol count";
    case BZD_R_NO_BYTE_IN_USE: return "mapping table names no byte value";
    case BZD_R_CODER_COUNT: return "entropy coder count outside 2 .. 6";
    case BZD_R_SELECTOR_COUNT: return "no selectors";
    case BZD_R_SELECTOR_INDEX: return "selector index not below the coder count";
    case BZD_R_CODE_LENGTH: return "code length outside 1 .. 20";
    case BZD_R_SELECTORS_EXHAUSTED: return "more symbol groups than selectors";
    case BZD_R_CODE_TOO_LONG: return "no code of up to 20 bits matches";
    case BZD_R_CODE_VECTOR: return "code vector out of range";
    case BZD_R_PERM_INDEX: return "code outside the permutation";
    case BZD_R_RUN_TOO_LONG: return "run of 2 Mi symbols or more";
    case BZD_R_BLOCK_OVERFLOW: return "more symbols than the block size";
    case BZD_R_BLOCK_CRC: return "block CRC mismatch";
    case BZD_R_STREAM_CRC: return "combined CRC mismatch";
    case BZD_R_TRUNCATED: return "input exhausted";
    case BZD_R_OUTPUT_FULL: return "output beyond cap";
    default: return "?";
  }
}

constexpr uint64_t BZD_BLOCK_MAGIC = 0x314159265359ull, BZD_FOOTER_MAGIC = 0x177245385090ull;
constexpr uint32_t BZD_MAX_SELECTORS = 18002, BZD_MAX_ALPHA = 258, BZD_MAX_CODE_LEN = 23, BZD_GROUP = 50, BZD_MAX_CODERS = 6;
constexpr int32_t BZD_E_DATA = -7;

// Tables of one block in flight: 27 KiB (in LDS on the device).  limit / base / perm: Create_Huffman_Decoding_Tables, as signed 32-bit values as in libbz2.
struct BzdTables {
  int32_t limit[BZD_MAX_CODERS][BZD_MAX_CODE_LEN + 1];
  int32_t base[BZD_MAX_CODERS][BZD_MAX_CODE_LEN + 1];
  uint16_t perm[BZD_MAX_CODERS][BZD_MAX_ALPHA];
  uint8_t len[BZD_MAX_CODERS][BZD_MAX_ALPHA + 2];
  uint8_t minlen[8];
  uint8_t seq[256];                        // seq_to_unseq
  uint8_t mtf[256];                        // the MTF list, front first
  uint32_t counts[256];                    // bytes of every value in the block's last column (cf_tab before Setup_Table)
  uint8_t selector[BZD_MAX_SELECTORS + 2];
};

// what the header of a block says
struct BzdBlockHdr { uint32_t stored_crc, origin, n_inuse, ncoders, nsel; };

// Symbols a block's slot holds.  RLE_1 writes a count byte behind every four equal bytes, so n symbols stand for at least n - n / 5 output bytes:
// a block of more than cap + cap / 4 symbols is over cap whatever it holds.
ZBZD_HD uint32_t bzd_slot_cap(uint32_t level, uint64_t cap) {
  const uint64_t nmax = 100000ull * level, most = cap + cap / 4;
  return (uint32_t)(most < nmax ? most : nmax);
}

// the stream header, byte by byte as libbz2 takes it; level 1 .. 9
ZBZD_HD uint32_t bzd_stream_header(const uint8_t h[4], uint64_t n_in, uint32_t &level) {
  const uint8_t want[3] = {'B', 'Z', 'h'};
  level = 0;
  for (uint32_t i = 0; i < 3; i++) {
    if (i >= n_in) return BZD_R_TRUNCATED;
    if (h[i] != want[i]) return BZD_R_STREAM_MAGIC;
  }
  if (n_in < 4) return BZD_R_TRUNCATED;
  if (h[3] < '1' || h[3] > '9') return BZD_R_STREAM_MAGIC;
  level = h[3] - '0';
  return BZD_OK;
}

// Create_Huffman_Decoding_Tables (bzip2-decoding.adb:182-220 = BZ2_hbCreateDecodeTables) of coder t, by one lane
ZBZD_HD void bzd_make_table(BzdTables &T, uint32_t t, uint32_t alpha) {
  uint32_t mn = 32, mx = 0;
  for (uint32_t i = 0; i < alpha; i++) { const uint32_t l = T.len[t][i]; if (l > mx) mx = l; if (l < mn) mn = l; }
  uint32_t pp = 0;
  for (uint32_t i = mn; i <= mx; i++)
    for (uint32_t j = 0; j < alpha; j++) if (T.len[t][j] == i) T.perm[t][pp++] = (uint16_t)j;
  for (; pp < BZD_MAX_ALPHA; pp++) T.perm[t][pp] = 0;
  int32_t *base = T.base[t], *limit = T.limit[t];
  for (uint32_t i = 0; i <= BZD_MAX_CODE_LEN; i++) { base[i] = 0; limit[i] = 0; }
  for (uint32_t i = 0; i < alpha; i++) base[T.len[t][i] + 1]++;
  for (uint32_t i = 1; i < BZD_MAX_CODE_LEN; i++) base[i] += base[i - 1];
  int32_t vec = 0;
  for (uint32_t i = mn; i <= mx; i++) { vec += base[i + 1] - base[i]; limit[i] = vec - 1; vec <<= 1; }
  for (uint32_t i = mn + 1; i <= mx; i++) base[i] = ((limit[i - 1] + 1) << 1) - base[i];
  T.minlen[t] = (uint8_t)mn;
}

// A block's header behind its magic, up to the decoding tables.  Returns a BzdRule.
template <class R> ZBZD_HD uint32_t bzd_block_header(R &br, BzdTables &T, uint32_t level, BzdBlockHdr &H, uint32_t lane, uint32_t nl) {
  H.stored_crc = br.bits(16) << 16;
  H.stored_crc |= br.bits(16);
  const uint32_t randomised = br.bits(1);
  H.origin = br.bits(24);
  if (randomised) return BZD_R_RANDOMISED;
  if (H.origin > 10u + 100000u * level) return BZD_R_ORIGIN;
  // Receive_Mapping_Table
  const uint32_t used16 = br.bits(16);
  uint32_t n_inuse = 0;
  ZBZD_SYNC();
  for (uint32_t i = 0; i < 16; i++) {
    if (!((used16 >> (15 - i)) & 1u)) continue;
    const uint32_t piece = br.bits(16);
    for (uint32_t j = 0; j < 16; j++)
      if ((piece >> (15 - j)) & 1u) { if (lane == 0) T.seq[n_inuse] = (uint8_t)(16 * i + j); n_inuse++; }
  }
  if (n_inuse == 0) return BZD_R_NO_BYTE_IN_USE;
  H.n_inuse = n_inuse;
  const uint32_t alpha = n_inuse + 2;
  // Receive_Selectors, the MTF of the selectors undone on the way (the list of up to six coders: four bits each of one word)
  H.ncoders = br.bits(3);
  if (H.ncoders < 2 || H.ncoders > BZD_MAX_CODERS) return BZD_R_CODER_COUNT;
  const uint32_t nsel = br.bits(15);
  if (nsel < 1) return BZD_R_SELECTOR_COUNT;
  uint32_t pos = 0x543210u;
  for (uint32_t i = 0; i < nsel; i++) {
    uint32_t j = 0;
    while (br.bits(1)) { j++; if (j >= H.ncoders) return BZD_R_SELECTOR_INDEX; }
    const uint32_t v = (pos >> (4 * j)) & 15u, low = pos & ((1u << (4 * j)) - 1u);
    pos = (pos & ~((1u << (4 * j + 4)) - 1u)) | (low << 4) | v;
    if (i < BZD_MAX_SELECTORS && lane == 0) T.selector[i] = (uint8_t)v;
    if ((i & 255u) == 255u && br.overrun()) return BZD_R_TRUNCATED;
  }
  H.nsel = nsel > BZD_MAX_SELECTORS ? BZD_MAX_SELECTORS : nsel;
  // Receive_Huffman_Bit_Lengths: the range is asked at every step of the delta chain, as libbz2 does
  for (uint32_t t = 0; t < H.ncoders; t++) {
    uint32_t cur = br.bits(5);
    for (uint32_t i = 0; i < alpha; i++) {
      for (;;) {
        if (cur < 1 || cur > 20) return BZD_R_CODE_LENGTH;
        if (!br.bits(1)) break;
        if (br.bits(1)) cur--; else cur++;
      }
      if (lane == 0) T.len[t][i] = (uint8_t)cur;
    }
    if (br.overrun()) return BZD_R_TRUNCATED;
  }
  ZBZD_SYNC();
  for (uint32_t t = lane; t < H.ncoders; t += nl) bzd_make_table(T, t, alpha);
  ZBZD_SYNC();
  return BZD_OK;
}

// Get_MTF_Value (bzip2-decoding.adb:316-355) with its three range checks
struct BzdGroup { int32_t group_no; uint32_t group_pos, sel, minlen; };
template <class R> ZBZD_HD uint32_t bzd_mtf_value(R &br, const BzdTables &T, BzdGroup &G, uint32_t nsel, uint32_t &sym) {
  if (G.group_pos == 0) {
    G.group_no++;
    if ((uint32_t)G.group_no >= nsel) return BZD_R_SELECTORS_EXHAUSTED;
    G.group_pos = BZD_GROUP;
    G.sel = ZBZD_UNI(T.selector[G.group_no]);
    G.minlen = ZBZD_UNI(T.minlen[G.sel]);
  }
  G.group_pos--;
  uint32_t zn = G.minlen, zvec = br.bits(zn);
  for (;;) {
    if (zn > 20) return BZD_R_CODE_TOO_LONG;
    if ((int32_t)zvec <= (int32_t)ZBZD_UNI(T.limit[G.sel][zn])) break;
    zn++;
    zvec = (zvec << 1) | br.bits(1);
  }
  if (zvec >> 31) return BZD_R_CODE_VECTOR;
  const int32_t pi = (int32_t)zvec - (int32_t)ZBZD_UNI(T.base[G.sel][zn]);
  if (pi < 0 || pi >= (int32_t)BZD_MAX_ALPHA) return BZD_R_PERM_INDEX;
  sym = ZBZD_UNI(T.perm[G.sel][pi]);
  return BZD_OK;
}

// the value at place nn of the MTF list moves to its front; on the device all lanes shift the list, on the host one loop does
ZBZD_HD uint32_t bzd_mtf_front(BzdTables &T, uint32_t nn, uint32_t lane) {
  const uint32_t v = ZBZD_UNI(T.mtf[nn]);
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) { const uint32_t i = lane + 64u * k; r[k] = (i >= 1 && i <= nn) ? T.mtf[i - 1] : 0u; if (64u * (k + 1) > nn) break; }
  ZBZD_SYNC();
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) { const uint32_t i = lane + 64u * k; if (i >= 1 && i <= nn) T.mtf[i] = (uint8_t)r[k]; if (64u * (k + 1) > nn) break; }
  if (lane == 0) T.mtf[0] = (uint8_t)v;
  ZBZD_SYNC();
#else
  (void)lane;
  for (uint32_t i = nn; i > 0; i--) T.mtf[i] = T.mtf[i - 1];
  T.mtf[0] = (uint8_t)v;
#endif
  return v;
}

// Receive_MTF_Values (bzip2-decoding.adb:293-468): the symbols of a block into its last column through a sink S -- put (byte, at) and
// run (byte, at, count), called by all lanes -- with T.counts kept beside.  The loop is bounded by nmax = 100 000 x level symbols, by the slot
// (bzd_slot_cap) and by the input's end.
template <class R, class S>
ZBZD_HD uint32_t bzd_block_symbols(R &br, BzdTables &T, const BzdBlockHdr &H, uint32_t nmax, uint32_t slot_cap, S &sink, uint32_t &nblock, uint32_t lane, uint32_t nl) {
  const uint32_t eob = H.n_inuse + 1;
  BzdGroup G{-1, 0, 0, 0};
  nblock = 0;
  ZBZD_SYNC();
  for (uint32_t i = lane; i < 256; i += nl) { T.mtf[i] = (uint8_t)i; T.counts[i] = 0; }
  ZBZD_SYNC();
  uint32_t sym = 0;
  uint32_t rule = bzd_mtf_value(br, T, G, H.nsel, sym);
  if (rule) return rule;
  for (;;) {
    if (br.overrun()) return BZD_R_TRUNCATED;
    if (sym == eob) break;
    if (sym <= 1) {
      uint32_t es = 0, N = 1;
      do {
        if (N >= 2u * 1024u * 1024u) return BZD_R_RUN_TOO_LONG;
        es += (sym + 1u) * N;
        N <<= 1;
        rule = bzd_mtf_value(br, T, G, H.nsel, sym);
        if (rule) return rule;
        if (br.overrun()) return BZD_R_TRUNCATED;
      } while (sym <= 1);
      const uint32_t uc = ZBZD_UNI(T.seq[ZBZD_UNI(T.mtf[0])]);
      if (nblock + es > nmax) return BZD_R_BLOCK_OVERFLOW;
      if (nblock + es > slot_cap) return BZD_R_OUTPUT_FULL;
      sink.run(uc, nblock, es);
      if (lane == 0) T.counts[uc] += es;
      nblock += es;
    } else {
      if (nblock >= nmax) return BZD_R_BLOCK_OVERFLOW;
      if (nblock >= slot_cap) return BZD_R_OUTPUT_FULL;
      const uint32_t uc = ZBZD_UNI(T.seq[bzd_mtf_front(T, sym - 1u, lane)]);
      sink.put(uc, nblock);
      if (lane == 0) T.counts[uc] += 1u;
      nblock++;
      rule = bzd_mtf_value(br, T, G, H.nsel, sym);
      if (rule) return rule;
    }
  }
  ZBZD_SYNC();
  return BZD_OK;
}

// One block from behind its magic to its end-of-block symbol; a failure behind the input's end is "input exhausted"
template <class R, class S>
ZBZD_HD uint32_t bzd_block(R &br, BzdTables &T, uint32_t level, uint32_t slot_cap, S &sink, BzdBlockHdr &H, uint32_t &nblock, uint32_t lane, uint32_t nl) {
  nblock = 0;
  uint32_t rule = bzd_block_header(br, T, level, H, lane, nl);
  if (!rule) rule = bzd_block_symbols(br, T, H, 100000u * level, slot_cap, sink, nblock, lane, nl);
  if (!rule && H.origin >= nblock) rule = BZD_R_ORIGIN;
  if (br.overrun()) rule = BZD_R_TRUNCATED;
  return rule;
}

// bzip2's CRC: polynomial 0x04C11DB7, most significant bit first (not the Zip CRC)
ZBZD_HD uint32_t bzd_crc_byte(uint32_t r, uint32_t b) {
  r ^= b << 24;
  for (int k = 0; k < 8; k++) r = (r & 0x80000000u) ? (r << 1) ^ 0x04C11DB7u : r << 1;
  return r;
}

// RLE_1 (bzip2-decoding.adb:489-542) as a machine over the bytes behind the inverse BWT: state 0 .. 3 = equal bytes seen since the run began
// (the byte before is `old`), 4 = four were seen and this byte is a count.  Returns the output bytes the byte stands for.
ZBZD_HD uint32_t bzd_rle_step(uint32_t &state, uint32_t old, uint32_t d) {
  if (state == 4) { state = 0; return d; }
  if (state > 0 && d != old) state = 1; else state++;
  return 1;
}

// what a decoder leaves per entry
struct BzdResult {
  int32_t rc;                 // 0, or ZADA_E_DATA (-7)
  uint32_t rule;              // the BzdRule broken
  uint64_t out_len;           // bytes written (0 unless rc = 0)
  uint64_t in_used;           // bytes up to and including the one that holds the last bit of the footer's CRC (0 unless rc = 0)
  uint64_t bitpos;            // where the decoder stood when it gave up
  uint32_t block, crc;        // the block it gave up in (from 1; 0: before the first); the Zip CRC-32 register behind the output
};

// ---- the reader of the CPU model ----
struct BzdHostReader {
  const uint8_t *in; uint64_t n, ip; uint64_t hold; uint32_t nb;
  ZBZD_HD void need32() {
    if (nb > 32) return;
    uint32_t w = 0;
    for (int k = 0; k < 4; k++) if (ip + k < n) w |= (uint32_t)in[ip + k] << (24 - 8 * k);
    hold |= (uint64_t)w << (32 - nb); nb += 32; ip += 4;
  }
  ZBZD_HD uint32_t bits(uint32_t k) { need32(); const uint32_t v = (uint32_t)(hold >> (64 - k)); hold <<= k; nb -= k; return v; }
  ZBZD_HD void open(const uint8_t *p, uint64_t len, uint64_t bit) { in = p; n = len; ip = bit >> 3; hold = 0; nb = 0; if (bit & 7u) (void)bits((uint32_t)(bit & 7u)); }
  ZBZD_HD uint64_t used_bits() const { return ip * 8 - nb; }
  ZBZD_HD bool overrun() const { return used_bits() > n * 8; }
};

}  // namespace zada
