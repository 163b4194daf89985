// unlzma_host.cpp -- the CPU model of the LZMA reader: zip-ada_amd/csrc/zada_unlzma_logic.h compiled for the host with one "lane".
// tests/_unlzma.py builds it into libunlzma_host.so (and once more with -fsanitize=address,undefined) and calls it through ctypes.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../zip-ada_amd/csrc/zada_unlzma_logic.h"

namespace {
uint32_t zip_tab[256];
void tables() {
  if (zip_tab[1]) return;
  for (uint32_t t = 0; t < 256; t++) {
    uint32_t l = t;
    for (int b = 0; b < 8; b++) l = (l & 1u) ? (l >> 1) ^ 0xEDB88320u : l >> 1;
    zip_tab[t] = l;
  }
}
}  // namespace

extern "C" {

// returns 0 or -7 (ZADA_E_DATA); res8 = out_len, in_used, rule, input byte, Zip CRC-32 register behind the output (from crc_in), output position,
// how the stream ended (1: marker, 2: without), 0.  The stream and the output are worked on in exact-size heap copies (a sanitizer sees a byte
// too many); out receives out_len bytes.
int um_unlzma(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint32_t eos, uint32_t crc_in, uint64_t *res8) {
  using namespace zada;
  tables();
  uint8_t *src = (uint8_t *)malloc(n_in ? n_in : 1);
  uint8_t *dst = (uint8_t *)malloc(cap ? cap : 1);
  uint16_t *probs = (uint16_t *)malloc(ULZ_NPROBS * 2);
  if (!src || !dst || !probs) { free(src); free(dst); free(probs); return -2; }
  if (n_in) memcpy(src, in, n_in);
  UlzResult R;
  UlzProps P{};
  uint8_t h[9] = {0};
  for (uint64_t i = 0; i < 9 && i < n_in; i++) h[i] = src[i];
  const uint32_t rule = ulz_props(h, n_in, P);
  if (rule) ulz_fail(R, rule, n_in < 9 ? n_in : 4, 0);
  else {
    uint16_t *lit = (uint16_t *)malloc((size_t)ulz_lit_elems(P) * 2);
    if (!lit) { free(src); free(dst); free(probs); return -2; }
    ulz_serial(src, n_in, dst, cap, eos, P, probs, lit, R);
    free(lit);
  }
  uint32_t r = crc_in;
  for (uint64_t i = 0; i < R.out_len; i++) r = zip_tab[(r ^ dst[i]) & 0xFF] ^ (r >> 8);
  if (R.out_len) memcpy(out, dst, R.out_len);
  res8[0] = R.out_len; res8[1] = R.in_used; res8[2] = R.rule; res8[3] = R.in_pos; res8[4] = r; res8[5] = R.out_pos; res8[6] = R.end; res8[7] = 0;
  free(src); free(dst); free(probs);
  return R.rc;
}

const char *um_rule_name(unsigned rule) { return zada::ulz_rule_name(rule); }

}
