// par64_check_main.cpp -- the CPU model of the parallel Inflate on Deflate64 streams (inflate_par64_host.cpp) under ASan + UBSan, as a program of its own: nothing is
// loaded into another process.  It reads a file of cases -- per case four little-endian u32 (stream bytes, cap, chunk KiB, repair per cent) and
// the stream -- and runs each one through ipm64_inflate on heap buffers of exactly the stream's and the cap's size, and through the one-wave
// decoder (inf_serial) on buffers of its own: return code, rule, bytes written, input used and the bytes have to agree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../zip-ada_amd/csrc/zada_inflate_logic.h"

extern "C" int ipm64_inflate(int format, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint32_t crc_in, uint32_t chunk_kib, uint32_t repair_pct, uint64_t *res6,
                           uint64_t *info8);

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint64_t cases = 0, parallel = 0, accepted = 0;
  uint32_t h[4];
  while (fread(h, 4, 4, f) == 4) {
    const uint64_t n = h[0], cap = h[1];
    uint8_t *in = (uint8_t *)malloc(n ? n : 1), *out = (uint8_t *)malloc(cap ? cap : 1), *ref = (uint8_t *)malloc(cap ? cap : 1);
    if (!in || !out || !ref || (n && fread(in, 1, n, f) != n)) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)cases); return 2; }
    uint64_t res[6], info[8];
    const int rc = ipm64_inflate(9, n ? in : nullptr, n, cap ? out : nullptr, cap, 0xFFFFFFFFu, h[2], h[3], res, info);
    zada::InfTables *T = (zada::InfTables *)malloc(sizeof(zada::InfTables));
    zada::InfResult R;
    zada::inf_serial(9, n ? in : nullptr, n, cap ? ref : nullptr, cap, *T, R);
    free(T);
    const bool same = rc == R.rc && res[0] == R.out_len && res[1] == R.in_used && (info[5] == 0 || res[2] == R.rule) && memcmp(out, ref, R.out_len) == 0;
    if (!same) {
      fprintf(stderr, "case %llu: model rc %d out_len %llu in_used %llu, one wave rc %d out_len %llu in_used %llu\n", (unsigned long long)cases, rc,
              (unsigned long long)res[0], (unsigned long long)res[1], R.rc, (unsigned long long)R.out_len, (unsigned long long)R.in_used);
      return 1;
    }
    cases++; parallel += info[5] == 0; accepted += rc == 0;
    free(in); free(out); free(ref);
  }
  fclose(f);
  printf("par64 check ok: %llu cases, %llu accepted, %llu in parallel\n", (unsigned long long)cases, (unsigned long long)accepted, (unsigned long long)parallel);
  return 0;
}
