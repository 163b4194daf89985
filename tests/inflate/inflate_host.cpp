// inflate_host.cpp -- the CPU model of the Inflate kernel: zip-ada_amd/csrc/zada_inflate_logic.h compiled for the host with one "lane".
// tests/_inflate.py builds it into libinflate_host.so (and once more with -fsanitize=address,undefined) and calls it through ctypes.
#include <stdint.h>
#include <stdlib.h>
static uint64_t im_stat[2];                    // symbols found in a primary table / by the canonical walk (codes longer than the table)
#define ZINF_STAT(x) (im_stat[x]++)
#include "../../zip-ada_amd/csrc/zada_inflate_logic.h"

extern "C" {

// returns 0 or -7 (ZADA_E_DATA); res6 = out_len, in_used, rule, bit position, CRC-32 register behind the output (from crc_in), 0
int im_inflate(int format, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint32_t crc_in, uint64_t *res6) {
  if (format != 8 && format != 9) return -1;
  zada::InfTables *T = (zada::InfTables *)malloc(sizeof(zada::InfTables));      // (on the heap: ASan then guards both of its ends)
  if (!T) return -2;
  zada::InfResult R;
  zada::inf_serial(format, in, n_in, out, cap, *T, R);
  free(T);
  uint32_t r = crc_in;
  for (uint64_t i = 0; i < R.out_len; i++) {                                    // Update, zip-crc_crypto.adb:49-60, bit by bit
    r ^= out[i];
    for (int b = 0; b < 8; b++) r = (r & 1u) ? (r >> 1) ^ 0xEDB88320u : r >> 1;
  }
  res6[0] = R.out_len; res6[1] = R.in_used; res6[2] = R.rule; res6[3] = R.bitpos; res6[4] = r; res6[5] = 0;
  return R.rc;
}

// the counters since the last call with reset != 0 (not thread-safe: the model is a test tool)
void im_symbol_stats(uint64_t out2[2], int reset) { out2[0] = im_stat[0]; out2[1] = im_stat[1]; if (reset) im_stat[0] = im_stat[1] = 0; }

const char *im_rule_name(unsigned rule) { return zada::inf_rule_name(rule); }

// Decode (zip-crc_crypto.adb:130-137) of n bytes in place, byte-serially
void im_crypt_decode(uint32_t keys[3], uint8_t *buf, uint64_t n) {
  static uint32_t tab[256];
  if (!tab[1]) for (uint32_t t = 0; t < 256; t++) { uint32_t l = t; for (int b = 0; b < 8; b++) l = (l & 1u) ? (l >> 1) ^ 0xEDB88320u : l >> 1; tab[t] = l; }
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t t = (keys[2] & 0xFFFFu) | 2u;
    const uint8_t p = (uint8_t)(buf[i] ^ ((t * (t ^ 1u)) >> 8));
    keys[0] = tab[(keys[0] ^ p) & 0xFF] ^ (keys[0] >> 8);
    keys[1] = (keys[1] + (keys[0] & 0xFFu)) * 134775813u + 1u;
    keys[2] = tab[(keys[2] ^ (keys[1] >> 24)) & 0xFF] ^ (keys[2] >> 8);
    buf[i] = p;
  }
}

}
