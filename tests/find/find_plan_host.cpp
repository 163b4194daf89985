// find_plan_host.cpp -- the host plan and the lane arithmetic of Find_Zip on the device (zip-ada_amd/csrc/zada_find_plan.h) for the CPU tests: a C
// interface for ctypes (tests/test_find_plan.py), and -- with -DFIND_PLAN_MAIN -- a program of its own that reads cases from a text file and prints
// what the model of the kernel makes of them, which the test builds with -fsanitize=address,undefined and runs as a child process.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_find_plan.h"

using namespace zada;

extern "C" {

const uint8_t *fp_upper_table(void) { return FZ_UPPER.v; }
const uint8_t *fp_lower_table(void) { return FZ_LOWER.v; }
int fp_check_len(uint64_t n) { return fz_check_len(n); }
uint32_t fp_upper4(uint32_t x) { return fz_upper4(x); }
void fp_upper16(uint32_t *w) { fz_upper16(w); }
uint32_t fp_eq_mask4(uint32_t x, uint32_t c) { return fz_eq_mask4(x, c * 0x01010101u); }
uint32_t fp_piece_log(void) { return FZ_PIECE_LOG; }
uint64_t fp_piece_count(uint64_t n) { return fz_piece_count(n); }
// the string as the kernel takes it: buf (1024 bytes), then len, pat, pmask, last4, fold, pat2, pmask2 into out [0 .. 7)
int fp_needle(const uint8_t *text, uint64_t len, uint32_t flags, uint8_t *buf, uint32_t *out) {
  FzNeedle N;
  const int rc = fz_needle(text, len, flags, N);
  if (rc) return rc;
  memcpy(buf, N.buf, FZ_MAX);
  out[0] = N.p.len; out[1] = N.p.pat; out[2] = N.p.pmask; out[3] = N.p.last4; out[4] = N.p.fold; out[5] = N.p.pat2; out[6] = N.p.pmask2;
  return 0;
}
// The model of k_fz_search on the entry x [0 .. n) laid at `phase` bytes (0 .. 15) behind a 16-byte boundary, with `front` in front of it and
// `behind` behind it (2048 bytes each, what a kernel that read too far would see).  Returns 0, ZADA_E_INVALID for a refused string, or 1 when the
// model loaded a word that holds no byte of the entry.
int fp_model(const uint8_t *x, uint64_t n, uint32_t phase, const uint8_t *front, const uint8_t *behind, const uint8_t *text, uint64_t len, uint32_t flags,
             uint64_t *occurrences, uint64_t *first) {
  FzNeedle N;
  const int rc = fz_needle(text, len, flags, N);
  if (rc) return rc;
  const uint64_t base = 2048 + phase;
  std::vector<uint8_t> mem(base + n + 2048);
  memcpy(mem.data() + base - 2048, front, 2048);
  if (n) memcpy(mem.data() + base, x, n);
  memcpy(mem.data() + base + n, behind, 2048);
  int bad = 0;
  fz_model(mem.data(), mem.size(), base, n, N, occurrences, first, &bad);
  return bad;
}
int fp_check(const zada_unzip_entry *ent, int count, uint64_t archive_len, int have_keys, int *bad, int *why) { return fz_check(ent, count, archive_len, have_keys, bad, why); }
int fp_groups(const zada_unzip_entry *ent, int count, uint64_t limit, int *ends, int cap) {
  std::vector<int> e;
  fz_groups(ent, count, limit, e);
  for (size_t i = 0; i < e.size() && (int)i < cap; i++) ends[i] = e[i];
  return (int)e.size();
}

}  // extern "C"

#ifdef FIND_PLAN_MAIN
// Lines of the file: "S flags phase <text in hex or -> <entry in hex or ->" -> "occurrences first" (or "refused") by the model, the bytes in front of
// the entry being the string itself and the bytes behind it the string's last character; "T" -> the two tables in hex; "U <dword in hex> <byte in hex>" -> fz_upper4 and fz_eq_mask4.
static std::vector<uint8_t> unhex(const char *s) {
  std::vector<uint8_t> v;
  if (!strcmp(s, "-")) return v;
  for (; s[0] && s[1]; s += 2) { unsigned b; sscanf(s, "%2x", &b); v.push_back((uint8_t)b); }
  return v;
}
int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<char> line(1 << 20), a(1 << 20), b(1 << 20);
  while (fgets(line.data(), (int)line.size(), f)) {
    unsigned flags, phase, x, c;
    if (line[0] == 'T') {
      for (int i = 0; i < 256; i++) printf("%02x", FZ_UPPER.v[i]);
      printf(" ");
      for (int i = 0; i < 256; i++) printf("%02x", FZ_LOWER.v[i]);
      printf("\n");
    } else if (sscanf(line.data(), "U %x %x", &x, &c) == 2) {
      printf("%08x %08x\n", fz_upper4(x), fz_eq_mask4(x, c * 0x01010101u));
    } else if (sscanf(line.data(), "S %u %u %s %s", &flags, &phase, a.data(), b.data()) == 4) {
      const std::vector<uint8_t> text = unhex(a.data()), entry = unhex(b.data());
      std::vector<uint8_t> front(2048, 0x21), behind(2048, text.empty() ? 0x21 : text.back());
      for (size_t i = 0; i < text.size() && i < 2048; i++) front[2048 - text.size() + i] = text[i];
      uint64_t occ = 0, first = 0;
      const int rc = fp_model(entry.data(), entry.size(), phase, front.data(), behind.data(), text.data(), text.size(), flags, &occ, &first);
      if (rc < 0) printf("refused\n");
      else if (rc) printf("stray load\n");
      else printf("%llu %llu\n", (unsigned long long)occ, (unsigned long long)first);
    }
  }
  fclose(f);
  printf("plan ok\n");
  return 0;
}
#endif
