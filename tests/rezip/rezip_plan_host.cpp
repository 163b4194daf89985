// rezip_plan_host.cpp -- the host plans of zada_rezip_device and zada_compzip_device (zip-ada_amd/csrc/zada_rezip_plan.h) for the CPU tests: a C interface for ctypes
// (tests/test_rezip_plan.py), and -- with -DREZIP_PLAN_MAIN -- a program of its own that reads lists from a text file and prints what the plan makes
// of them, which the test builds with -fsanitize=address,undefined and runs as a child process.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_rezip_plan.h"

using namespace zada;

extern "C" {

int rp_verdict(uint64_t la, uint64_t lb, uint64_t d, uint64_t *position, uint64_t *compared) { return cz_verdict(la, lb, d, position, compared); }
int rp_check(const zada_unzip_entry *a, const zada_unzip_entry *b, int count, uint64_t len_a, uint64_t len_b, int have_keys, int *bad, int *side, int *why) {
  return cz_check(a, b, count, len_a, len_b, have_keys, bad, side, why);
}
const char *rp_why_text(int why) { return uz_why_text(why); }
uint64_t rp_slot(const zada_unzip_entry *a, const zada_unzip_entry *b) { return cz_slot(*a, *b); }
// the groups: up to cap ends; returns how many groups there are
int rp_groups(const zada_unzip_entry *a, const zada_unzip_entry *b, int count, uint64_t limit, int *ends, int cap) {
  std::vector<int> e;
  cz_groups(a, b, count, limit, e);
  for (size_t i = 0; i < e.size() && (int)i < cap; i++) ends[i] = e[i];
  return (int)e.size();
}
uint64_t rp_piece_count(uint64_t n) { return cz_piece_count(n); }
uint32_t rp_piece_log(void) { return CZ_PIECE_LOG; }

// ---- ReZip ----
uint32_t rp_considered(uint32_t approaches, uint32_t formats) { return rz_considered(approaches, formats); }
int rp_choose(const uint64_t *size, int original_allowed) { return rz_choose(size, original_allowed != 0); }
// the distinct methods of an entry: up to 12 into out; returns how many
int rp_methods(uint32_t considered, int p2, int p1, int *out) {
  std::vector<int> m;
  rz_methods(considered, p2, p1, m);
  for (size_t i = 0; i < m.size(); i++) out[i] = m[i];
  return (int)m.size();
}
int rp_rz_check(const zada_rezip_entry *ent, int count, uint64_t d_src, uint64_t src_len, uint64_t d_archive, uint64_t cap, int *bad, int *why) {
  return rz_check(ent, count, d_src, src_len, d_archive, cap, bad, why);
}
const char *rp_rz_why_text(int why) { return rz_why_text(why); }
uint64_t rp_rz_bound(int count, const zada_rezip_entry *ent, uint64_t comment_len) { return rz_bound(count, ent, comment_len); }
int rp_rz_groups(const zada_rezip_entry *ent, int count, uint64_t limit, int *ends, int cap) {
  std::vector<int> e;
  rz_groups(ent, count, limit, e);
  for (size_t i = 0; i < e.size() && (int)i < cap; i++) ends[i] = e[i];
  return (int)e.size();
}
// The archive of made-up winners (payloads as lengths only): the kept entries' local headers one behind the other, then the central directory, the
// end records and the comment, into out (up to cap bytes); offsets [k] of the kept entries; *archive_len.  Returns the bytes the headers take.
uint64_t rp_rz_archive(const zada_rezip_entry *ent, int count, const uint64_t *csize, const uint16_t *zip_type, const uint8_t *eos, uint64_t base,
                       const uint8_t *comment, uint32_t comment_len, uint8_t *out, uint64_t cap, uint64_t *offsets, uint64_t *archive_len) {
  RzArchive A;
  A.base = base;
  std::vector<uint8_t> blob;
  int k = 0;
  for (int i = 0; i < count; i++) {
    if (rz_dropped(ent[i])) continue;
    offsets[k++] = A.base + A.pos;
    rz_add(A, ent[i], csize[i], zip_type[i], eos[i] != 0, blob);
  }
  rz_finish(A, comment, comment_len, blob);
  *archive_len = A.pos;
  for (size_t j = 0; j < blob.size() && j < cap; j++) out[j] = blob[j];
  return blob.size();
}

}

#ifdef REZIP_PLAN_MAIN
// input, by the first character of a line:
//   "c allowed s0 .. s11"            a choice (18446744073709551615: not tried)                         -> the choice
//   "m approaches formats p2 p1"     the methods to run                                                 -> the methods
//   "e count src_len d_src d_archive cap limit comment_len" + count lines "name in_off n_in usize method flags"
//                                    an entry table: check, bound, groups                               -> "rc bad why | bound | groups: ends ..."
//   "a count base comment" + count lines "name usize flags version time crc csize zip_type eos"
//                                    an archive of made-up winners (payloads as lengths)               -> "archive_len header_bytes fnv1a64 | offsets ..."
//   "v la lb d"                      a verdict                                                          -> "verdict position compared"
//   "g count len_a len_b have_keys limit" + count lines "in_off n_in cap method flags | in_off n_in cap method flags"
//                                    a list of pairs                                                    -> "rc bad side why | groups: ends ..."
// Names and the comment are hexadecimal, "-" for none; every name is an exact-size heap block of its own (an empty one: a null pointer).
static uint8_t *hex_block(const char *h, uint32_t *len) {
  if (h[0] == '-') { *len = 0; return nullptr; }
  const size_t n = strlen(h) / 2;
  uint8_t *p = (uint8_t *)malloc(n ? n : 1);
  for (size_t i = 0; i < n; i++) { unsigned v; sscanf(h + 2 * i, "%2x", &v); p[i] = (uint8_t)v; }
  *len = (uint32_t)n;
  if (!n) { free(p); return nullptr; }
  return p;
}
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'c') {
      int allowed;
      uint64_t *size = (uint64_t *)malloc(RZ_NA * sizeof(uint64_t));
      if (fscanf(f, "%d", &allowed) != 1) return 2;
      for (int a = 0; a < RZ_NA; a++) { unsigned long long v; if (fscanf(f, "%llu", &v) != 1) return 2; size[a] = v; }
      printf("%d\n", rz_choose(size, allowed != 0));
      free(size);
      continue;
    }
    if (kind == 'm') {
      unsigned approaches, formats;
      int p2, p1;
      if (fscanf(f, "%u %u %d %d", &approaches, &formats, &p2, &p1) != 4) return 2;
      std::vector<int> m;
      rz_methods(rz_considered(approaches, formats), p2, p1, m);
      for (int x : m) printf("%d ", x);
      printf("\n");
      continue;
    }
    if (kind == 'e' || kind == 'a') {
      int count;
      unsigned long long q[6] = {0, 0, 0, 0, 0, 0};
      static char word[140000];
      if (fscanf(f, "%d", &count) != 1) return 2;
      uint8_t *comment = nullptr;
      uint32_t comment_len = 0;
      if (kind == 'e') { for (int j = 0; j < 6; j++) if (fscanf(f, "%llu", &q[j]) != 1) return 2; }
      else { if (fscanf(f, "%llu %139999s", &q[0], word) != 2) return 2; comment = hex_block(word, &comment_len); }
      zada_rezip_entry *ent = (zada_rezip_entry *)malloc(count ? (size_t)count * sizeof(zada_rezip_entry) : 1);
      uint64_t *csize = (uint64_t *)malloc(count ? (size_t)count * 8 : 1);
      uint16_t *zt = (uint16_t *)malloc(count ? (size_t)count * 2 : 1);
      uint8_t *eos = (uint8_t *)malloc(count ? (size_t)count : 1);
      for (int i = 0; i < count; i++) {
        unsigned long long a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (fscanf(f, "%139999s", word) != 1) return 2;
        for (int j = 0; j < (kind == 'e' ? 5 : 8); j++) if (fscanf(f, "%llu", &a[j]) != 1) return 2;
        uint32_t nl = 0;
        uint8_t *nm = hex_block(word, &nl);
        if (kind == 'e') ent[i] = zada_rezip_entry{a[0], a[1], a[2], 0, 0, (uint16_t)a[3], (uint16_t)a[4], 20, 0, nl, nm};
        else { ent[i] = zada_rezip_entry{0, 0, a[0], (uint32_t)a[4], (uint32_t)a[3], 0, (uint16_t)a[1], (uint16_t)a[2], 0, nl, nm}; csize[i] = a[5]; zt[i] = (uint16_t)a[6]; eos[i] = (uint8_t)a[7]; }
      }
      if (kind == 'e') {
        int bad, why;
        const int rc = rz_check(ent, count, q[1], q[0], q[2], q[3], &bad, &why);
        printf("%d %d %d | %llu | groups:", rc, bad, why, (unsigned long long)rz_bound(count, ent, q[5]));
        std::vector<int> ends;
        rz_groups(ent, count, q[4], ends);
        for (int e : ends) printf(" %d", e);
        printf("\n");
      } else {
        RzArchive A;
        A.base = q[0];
        std::vector<uint8_t> blob;
        std::vector<uint64_t> offs;
        for (int i = 0; i < count; i++) {
          if (rz_dropped(ent[i])) continue;
          offs.push_back(A.base + A.pos);
          rz_add(A, ent[i], csize[i], zt[i], eos[i] != 0, blob);
        }
        rz_finish(A, comment, comment_len, blob);
        uint64_t h = 1469598103934665603ull;
        for (uint8_t b : blob) h = (h ^ b) * 1099511628211ull;
        printf("%llu %llu %llu |", (unsigned long long)A.pos, (unsigned long long)blob.size(), (unsigned long long)h);
        for (uint64_t o : offs) printf(" %llu", (unsigned long long)o);
        printf("\n");
      }
      for (int i = 0; i < count; i++) free((void *)ent[i].name);
      free(ent); free(csize); free(zt); free(eos); free(comment);
      continue;
    }
    if (kind == 'v') {
      unsigned long long la, lb, d;
      if (fscanf(f, "%llu %llu %llu", &la, &lb, &d) != 3) return 2;
      uint64_t pos = 0, cmp = 0;
      const int v = cz_verdict(la, lb, d, &pos, &cmp);
      printf("%d %llu %llu\n", v, (unsigned long long)pos, (unsigned long long)cmp);
      continue;
    }
    int count, have_keys;
    unsigned long long len_a, len_b, limit;
    if (kind != 'g' || fscanf(f, "%d %llu %llu %d %llu", &count, &len_a, &len_b, &have_keys, &limit) != 5) return 2;
    // exact-size heap blocks: a read or a write beyond a table is the sanitizer's to see
    zada_unzip_entry *a = (zada_unzip_entry *)malloc(count ? (size_t)count * sizeof(zada_unzip_entry) : 1);
    zada_unzip_entry *b = (zada_unzip_entry *)malloc(count ? (size_t)count * sizeof(zada_unzip_entry) : 1);
    for (int i = 0; i < count; i++) {
      unsigned long long x[3], y[3];
      unsigned mx, fx, my, fy;
      if (fscanf(f, "%llu %llu %llu %u %u | %llu %llu %llu %u %u", &x[0], &x[1], &x[2], &mx, &fx, &y[0], &y[1], &y[2], &my, &fy) != 10) return 2;
      a[i] = zada_unzip_entry{x[0], x[1], 0, x[2], (uint16_t)mx, (uint8_t)fx, 0, 0};
      b[i] = zada_unzip_entry{y[0], y[1], 0, y[2], (uint16_t)my, (uint8_t)fy, 0, 0};
    }
    int bad, side, why;
    const int rc = cz_check(a, b, count, len_a, len_b, have_keys, &bad, &side, &why);
    printf("%d %d %d %d | groups:", rc, bad, side, why);
    std::vector<int> ends;
    cz_groups(a, b, count, limit, ends);
    for (int e : ends) printf(" %d", e);
    printf("\n");
    free(a); free(b);
  }
  fclose(f);
  printf("plan ok\n");
  return 0;
}
#endif
