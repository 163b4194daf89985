// par_batch_check_main.cpp -- the CPU model of the batched parallel Inflate (inflate_par_batch_host.cpp) under ASan + UBSan, as a program of its
// own: nothing is loaded into another process.  It reads a file of tables -- per table six little-endian u32 (streams, chunk KiB, repair per cent,
// the Deflate64 knob, min KiB, batch MiB), then per stream three u32 (stream bytes, cap, format) and the stream -- and runs each table through
// ipb_inflate on heap buffers of exactly each stream's and each cap's size, and every stream through the one-wave decoder (inf_serial) on buffers
// of its own: return code, rule (where the one wave judged), bytes written, input used and the bytes have to agree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_inflate_logic.h"

extern "C" int ipb_inflate(uint32_t n, const uint32_t *format, const uint8_t *const *in, const uint64_t *n_in, uint8_t *const *out, const uint64_t *cap, const uint32_t *crc_in,
                           uint32_t chunk_kib, uint32_t repair_pct, uint32_t deflate64, uint32_t min_kib, uint32_t batch_mib, int32_t *rc, uint64_t *res6, uint64_t *info8,
                           uint32_t *pass_ends, uint32_t *n_passes);

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s TABLES\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint64_t tables = 0, streams = 0, taken = 0, accepted = 0;
  uint32_t h[6];
  while (fread(h, 4, 6, f) == 6) {
    const uint32_t n = h[0];
    std::vector<uint32_t> format(n), crc(n, 0xFFFFFFFFu), ends(n + 1);
    std::vector<uint8_t *> in(n), out(n);
    std::vector<uint64_t> n_in(n), cap(n), res((size_t)n * 6);
    std::vector<int32_t> rc(n);
    for (uint32_t k = 0; k < n; k++) {
      uint32_t s[3];
      if (fread(s, 4, 3, f) != 3) { fprintf(stderr, "table %llu: short file\n", (unsigned long long)tables); return 2; }
      n_in[k] = s[0]; cap[k] = s[1]; format[k] = s[2];
      in[k] = (uint8_t *)malloc(s[0] ? s[0] : 1); out[k] = (uint8_t *)malloc(s[1] ? s[1] : 1);
      if (!in[k] || !out[k] || (s[0] && fread(in[k], 1, s[0], f) != s[0])) { fprintf(stderr, "table %llu: short file\n", (unsigned long long)tables); return 2; }
    }
    uint64_t info[8];
    uint32_t npass = 0;
    const int r = ipb_inflate(n, format.data(), in.data(), n_in.data(), out.data(), cap.data(), crc.data(), h[1], h[2], h[3], h[4], h[5], rc.data(), res.data(), info, ends.data(), &npass);
    if (r) { fprintf(stderr, "table %llu: ipb_inflate %d\n", (unsigned long long)tables, r); return 1; }
    zada::InfTables *T = (zada::InfTables *)malloc(sizeof(zada::InfTables));
    for (uint32_t k = 0; k < n; k++) {
      uint8_t *ref = (uint8_t *)malloc(cap[k] ? cap[k] : 1);
      zada::InfResult R;
      zada::inf_serial((int)format[k], in[k], n_in[k], ref, cap[k], *T, R);
      const uint64_t *g = &res[(size_t)k * 6];
      const bool same = rc[k] == R.rc && g[0] == R.out_len && g[1] == R.in_used && (g[4] == 1 || g[2] == R.rule) && memcmp(out[k], ref, R.out_len) == 0;
      if (!same) {
        fprintf(stderr, "table %llu stream %u: model rc %d out_len %llu in_used %llu, one wave rc %d out_len %llu in_used %llu\n", (unsigned long long)tables, k, rc[k],
                (unsigned long long)g[0], (unsigned long long)g[1], R.rc, (unsigned long long)R.out_len, (unsigned long long)R.in_used);
        return 1;
      }
      streams++; taken += g[4]; accepted += rc[k] == 0;
      free(ref); free(in[k]); free(out[k]);
    }
    free(T);
    if (info[7] - info[5] != 0 && info[3] == 0) { fprintf(stderr, "table %llu: streams taken and no scout launch\n", (unsigned long long)tables); return 1; }
    tables++;
  }
  fclose(f);
  printf("par batch check ok: %llu tables, %llu streams, %llu accepted, %llu in parallel\n", (unsigned long long)tables, (unsigned long long)streams, (unsigned long long)accepted,
         (unsigned long long)taken);
  return 0;
}
