// unzip_plan_host.cpp -- the host plan of zada_unzip_device (zip-ada_amd/csrc/zada_unzip_plan.h) for the CPU tests: a C interface for ctypes
// (tests/test_unzip_plan.py), and -- with -DUNZIP_PLAN_MAIN -- a program of its own that reads entry lists from a text file and prints what the plan
// makes of them, which the test builds with -fsanitize=address,undefined and runs as a child process.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_unzip_plan.h"

using namespace zada;

extern "C" {

int up_check(const zada_unzip_entry *ent, int count, uint64_t archive_len, uint64_t out_bytes, int have_out, int have_keys, int *bad, int *why) {
  return uz_check(ent, count, archive_len, out_bytes, have_out, have_keys, bad, why);
}
uint64_t up_payload(const zada_unzip_entry *e) { return uz_payload(*e); }
// the pieces of n entries of len [k] bytes: up to cap of them into off / entry / plen, first [n + 1]; returns how many there are
uint64_t up_pieces(const uint64_t *len, uint32_t n, uint32_t plog, uint64_t *off, uint32_t *entry, uint32_t *plen, uint64_t cap, uint64_t *first) {
  std::vector<uint32_t> id(n);
  for (uint32_t k = 0; k < n; k++) id[k] = k;
  std::vector<UzPiece> pieces;
  std::vector<uint64_t> f;
  uz_pieces(len, id.data(), n, plog, pieces, f);
  for (uint64_t i = 0; i < pieces.size() && i < cap; i++) { off[i] = pieces[i].off; entry[i] = pieces[i].entry; plen[i] = pieces[i].len; }
  for (uint32_t k = 0; k <= n; k++) first[k] = f[k];
  return pieces.size();
}
// the groups of the test-only form: up to cap ends; returns how many groups there are
int up_groups(const zada_unzip_entry *ent, int count, uint64_t limit, int *ends, int cap) {
  std::vector<int> e;
  uz_groups(ent, count, limit, e);
  for (size_t i = 0; i < e.size() && (int)i < cap; i++) ends[i] = e[i];
  return (int)e.size();
}

}

#ifdef UNZIP_PLAN_MAIN
// input: per list a line "count archive_len out_bytes have_out have_keys limit plog", then count lines "in_off n_in out_off cap method flags".
// output: per list a line "rc bad why | groups: ends ... | pieces: count, sum of (off + 3 * entry + 7 * len) mod 2 ** 64 over the stored entries' pieces"
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int count, have_out, have_keys;
  unsigned plog;
  unsigned long long archive_len, out_bytes, limit;
  while (fscanf(f, "%d %llu %llu %d %d %llu %u", &count, &archive_len, &out_bytes, &have_out, &have_keys, &limit, &plog) == 7) {
    // exact-size heap blocks: a read or a write beyond the table is the sanitizer's to see
    zada_unzip_entry *ent = (zada_unzip_entry *)malloc(count ? (size_t)count * sizeof(zada_unzip_entry) : 1);
    for (int i = 0; i < count; i++) {
      unsigned long long a, b, c, d;
      unsigned m, fl;
      if (fscanf(f, "%llu %llu %llu %llu %u %u", &a, &b, &c, &d, &m, &fl) != 6) return 2;
      ent[i] = zada_unzip_entry{a, b, c, d, (uint16_t)m, (uint8_t)fl, 0, 0};
    }
    int bad, why;
    const int rc = uz_check(ent, count, archive_len, out_bytes, have_out, have_keys, &bad, &why);
    printf("%d %d %d | groups:", rc, bad, why);
    std::vector<int> ends;
    uz_groups(ent, count, limit, ends);
    for (int e : ends) printf(" %d", e);
    std::vector<uint64_t> len;
    std::vector<uint32_t> id;
    for (int i = 0; i < count; i++) if (ent[i].method == 0) { len.push_back(uz_payload(ent[i]) & 0xFFFFF); id.push_back((uint32_t)i); }
    std::vector<UzPiece> pieces;
    std::vector<uint64_t> first;
    uz_pieces(len.data(), id.data(), (uint32_t)len.size(), plog, pieces, first);
    uint64_t sum = 0;
    for (const UzPiece &p : pieces) sum += p.off + 3ull * p.entry + 7ull * p.len;
    printf(" | pieces: %llu %llu\n", (unsigned long long)pieces.size(), (unsigned long long)sum);
    free(ent);
  }
  fclose(f);
  printf("plan ok\n");
  return 0;
}
#endif
