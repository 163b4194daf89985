// bunzip2_host.cpp -- the CPU model of the BZip2 reader: zip-ada_amd/csrc/zada_bunzip2_logic.h compiled for the host with one "lane", and every
// later stage (BWT_Detransform, the chase of RLE_1, the block CRC; bzip2-decoding.adb:470-542) as a plain serial loop behind it.
// tests/_bunzip2.py builds it into libbunzip2_host.so (and once more with -fsanitize=address,undefined) and calls it through ctypes.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../zip-ada_amd/csrc/zada_bunzip2_logic.h"

namespace {

struct Sink {
  uint8_t *L;
  void put(uint32_t uc, uint32_t at) { L[at] = (uint8_t)uc; }
  void run(uint32_t uc, uint32_t at, uint32_t es) { memset(L + at, (int)uc, es); }
};

uint32_t bz_tab[256], zip_tab[256];
void tables() {
  if (bz_tab[1]) return;
  for (uint32_t t = 0; t < 256; t++) {
    bz_tab[t] = zada::bzd_crc_byte(0, t);
    uint32_t l = t;
    for (int b = 0; b < 8; b++) l = (l & 1u) ? (l >> 1) ^ 0xEDB88320u : l >> 1;
    zip_tab[t] = l;
  }
}

void fail(zada::BzdResult &res, uint32_t rule, uint64_t bit, uint32_t block) {
  res.rc = zada::BZD_E_DATA; res.rule = rule; res.out_len = 0; res.in_used = 0; res.bitpos = bit; res.block = block;
}

// rec: per block 4 values (symbols, origin, stored CRC, end bit), up to cap_rec blocks; *nrec: blocks decoded
void serial(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, zada::BzdTables &T, zada::BzdResult &res, uint64_t *rec, uint64_t cap_rec, uint64_t *nrec) {
  using namespace zada;
  res.rc = 0; res.rule = 0; res.out_len = 0; res.in_used = 0; res.bitpos = 0; res.block = 0; res.crc = 0;
  *nrec = 0;
  uint8_t h[4] = {0, 0, 0, 0};
  for (uint64_t i = 0; i < 4 && i < n_in; i++) h[i] = in[i];
  uint32_t level = 0;
  uint32_t rule = bzd_stream_header(h, n_in, level);
  if (rule) { fail(res, rule, 0, 0); return; }
  const uint32_t nmax = 100000u * level, slot_cap = zada::bzd_slot_cap(level, cap);
  uint8_t *L = (uint8_t *)malloc(slot_cap ? slot_cap : 1);            // (exact sizes on the heap: a sanitizer sees a symbol too many)
  uint32_t *tt = (uint32_t *)malloc(slot_cap ? (size_t)slot_cap * 4 : 4);
  BzdHostReader br;
  br.open(in, n_in, 32);
  uint64_t pos = 0;
  uint32_t comb = 0, blockno = 0;
  for (;;) {
    const uint64_t at = br.used_bits();
    uint64_t magic = (uint64_t)br.bits(24) << 24;
    magic |= br.bits(24);
    if (br.overrun()) { fail(res, BZD_R_TRUNCATED, at, blockno); break; }
    if (magic == BZD_FOOTER_MAGIC) {
      uint32_t stored = br.bits(16) << 16;
      stored |= br.bits(16);
      if (br.overrun()) { fail(res, BZD_R_TRUNCATED, at, blockno); break; }
      if (stored != comb) { fail(res, BZD_R_STREAM_CRC, at, blockno); break; }
      res.out_len = pos; res.in_used = (br.used_bits() + 7) / 8; res.bitpos = br.used_bits(); res.block = blockno;
      break;
    }
    if (magic != BZD_BLOCK_MAGIC) { fail(res, BZD_R_BLOCK_MAGIC, at, blockno); break; }
    blockno++;
    Sink sink{L};
    BzdBlockHdr H{};
    uint32_t n = 0;
    rule = bzd_block(br, T, level, slot_cap, sink, H, n, 0, 1);
    if (rule) { fail(res, rule, br.used_bits(), blockno); break; }
    if (*nrec < cap_rec && rec) { uint64_t *r = rec + 4 * *nrec; r[0] = n; r[1] = H.origin; r[2] = H.stored_crc; r[3] = br.used_bits(); }
    ++*nrec;
    // Setup_Table, BWT_Detransform
    uint32_t cf[256], t = 0;
    for (int i = 0; i < 256; i++) { cf[i] = t; t += T.counts[i]; }
    for (uint32_t p = 0; p < n; p++) tt[p] = L[p];
    for (uint32_t p = 0; p < n; p++) tt[cf[L[p]]++] |= p << 8;
    // RLE_1 along the chase, the block CRC beside it
    uint32_t idx = tt[H.origin] >> 8, state = 0, old = 0, crc = 0xFFFFFFFFu;
    bool full = false;
    for (uint32_t k = 0; k < n && !full; k++) {
      const uint32_t w = tt[idx];
      const uint32_t d = w & 0xFFu;
      idx = w >> 8;
      const bool count = state == 4;
      const uint32_t m = bzd_rle_step(state, old, d);
      const uint32_t by = count ? old : d;
      if (pos + m > cap) { full = true; break; }
      for (uint32_t i = 0; i < m; i++) { out[pos + i] = (uint8_t)by; crc = (crc << 8) ^ bz_tab[(crc >> 24) ^ by]; }
      pos += m;
      if (!count) old = d;
    }
    if (full) { fail(res, BZD_R_OUTPUT_FULL, br.used_bits(), blockno); break; }
    crc = ~crc;
    if (crc != H.stored_crc) { fail(res, BZD_R_BLOCK_CRC, br.used_bits(), blockno); break; }
    comb = ((comb << 1) | (comb >> 31)) ^ crc;
  }
  free(tt);
  free(L);
}

}  // namespace

extern "C" {

// returns 0 or -7 (ZADA_E_DATA); res8 = out_len, in_used, rule, bit position, Zip CRC-32 register behind the output (from crc_in), block, blocks decoded, 0
int bm_bunzip2(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint32_t crc_in, uint64_t *res8, uint64_t *rec, uint64_t cap_rec) {
  tables();
  zada::BzdTables *T = (zada::BzdTables *)malloc(sizeof(zada::BzdTables));
  if (!T) return -2;
  zada::BzdResult R;
  uint64_t nrec = 0;
  serial(in, n_in, out, cap, *T, R, rec, cap_rec, &nrec);
  free(T);
  uint32_t r = crc_in;
  for (uint64_t i = 0; i < R.out_len; i++) r = zip_tab[(r ^ out[i]) & 0xFF] ^ (r >> 8);
  res8[0] = R.out_len; res8[1] = R.in_used; res8[2] = R.rule; res8[3] = R.bitpos; res8[4] = r; res8[5] = R.block; res8[6] = nrec; res8[7] = 0;
  return R.rc;
}

const char *bm_rule_name(unsigned rule) { return zada::bzd_rule_name(rule); }

}
