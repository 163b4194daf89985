// zip_plan_ex_host.cpp -- the host plan of zada_zip_device_ex (zip-ada_amd/csrc/zada_zip_plan.h: a method per entry, the groups with several methods,
// the flag bits, encryption headers) for the CPU tests: a C interface for ctypes (tests/test_zip_plan_ex.py), and -- with -DZIP_PLAN_MAIN -- a program
// of its own that reads entry lists from a text file and prints what the plan makes of them, which the test builds with -fsanitize=address,undefined
// and runs as a child process.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_zip_plan.h"

using namespace zada;

// The whole plan of one call as zada_zip_device_ex walks it: the groups in order (store: method Store for all), every group placed from its verdicts
// -- bytes [i] of stream at device address src [i], the running register reg [i], the zip type zt [i] of entry i's method --, hdr12: null, or twelve
// bytes per entry.  Returns the archive's length.
static uint64_t plan_archive_ex(const zada_zip_entry *ent, int count, int store, const int *m, const uint64_t *lit, uint64_t base, uint64_t limit, uint64_t bz_limit,
                                uint64_t lit_limit, const uint64_t *src, const uint64_t *bytes, const uint32_t *reg, const uint16_t *zt, const uint8_t *hdr12,
                                std::vector<ZwGroup> &groups, std::vector<uint8_t> &locals, std::vector<uint8_t> &tail, std::vector<ZwJob> &jobs, zada_zip_result *res) {
  ZwArchive A;
  A.base = base;
  if (store) zw_groups(ent, count, 0, 0, groups);
  else zw_groups_ex(ent, count, m, lit, limit, bz_limit, lit_limit, groups);
  for (const ZwGroup &g : groups) {
    std::vector<ZwVerdict> v;
    for (int i = g.g0; i < g.g1; i++) v.push_back(ZwVerdict{src[i], bytes[i], reg[i], zt[i], 0});
    zw_group_place_ex(A, ent, g.g0, g.g1, v.data(), hdr12 ? hdr12 + 12 * (size_t)g.g0 : nullptr, locals, jobs, res);
  }
  zw_finish(A, tail);
  return A.pos;
}

extern "C" {

int zpx_method_ok(int m) { return zw_method_ok_ex(m) ? 1 : 0; }
int zpx_zip_type(int m) { return zw_zip_type(m); }
uint64_t zpx_one_block(int m) { return zw_bz_one_block(m); }
int zpx_check(const zada_zip_entry *ent, int count, uint64_t d_archive, uint64_t cap, int encrypted, int *bad, int *why) { return zw_check_ex(ent, count, d_archive, cap, encrypted != 0, bad, why); }
const char *zpx_why_text(int why) { return zw_why_text(why); }
// the groups alone: up to cap (g1, kind) pairs; returns how many there are
int zpx_groups(const zada_zip_entry *ent, int count, const int *m, const uint64_t *lit, uint64_t limit, uint64_t bz_limit, uint64_t lit_limit, int *groups, int cap) {
  std::vector<ZwGroup> g;
  zw_groups_ex(ent, count, m, lit, limit, bz_limit, lit_limit, g);
  for (size_t k = 0; k < g.size() && (int)k < cap; k++) { groups[2 * k] = g[k].g1; groups[2 * k + 1] = g[k].kind; }
  return (int)g.size();
}
uint64_t zpx_bound(int count, const zada_zip_entry *ent, uint64_t base, int encrypted) { return zw_bound_ex(count, ent, base, encrypted != 0); }
// the whole plan from verdicts (plan_archive_ex): the groups as (g1, kind) pairs, up to jobs_cap jobs as five values each (kind, entry, src, dst, len),
// the results, the local headers (in job order, each with its encryption header) and the tail.  Returns the archive's length; a buffer that is too
// small gets nothing (*_need say what it takes).
uint64_t zpx_archive(const zada_zip_entry *ent, int count, int store, const int *m, const uint64_t *lit, uint64_t base, uint64_t limit, uint64_t bz_limit, uint64_t lit_limit,
                     const uint64_t *src, const uint64_t *bytes, const uint32_t *reg, const uint16_t *zt, const uint8_t *hdr12, int *groups, int groups_cap, int *ngroups,
                     uint64_t *jobs, uint64_t jobs_cap, uint64_t *njobs, zada_zip_result *res, uint8_t *locals, uint64_t locals_cap, uint64_t *locals_need, uint8_t *tail,
                     uint64_t tail_cap, uint64_t *tail_need) {
  std::vector<uint8_t> l, t;
  std::vector<ZwJob> j;
  std::vector<ZwGroup> g;
  const uint64_t len = plan_archive_ex(ent, count, store, m, lit, base, limit, bz_limit, lit_limit, src, bytes, reg, zt, hdr12, g, l, t, j, res);
  *ngroups = (int)g.size(); *njobs = j.size(); *locals_need = l.size(); *tail_need = t.size();
  for (size_t k = 0; k < g.size() && (int)k < groups_cap; k++) { groups[2 * k] = g[k].g1; groups[2 * k + 1] = g[k].kind; }
  for (size_t k = 0; k < j.size() && k < jobs_cap; k++) { uint64_t *r = jobs + 5 * k; r[0] = j[k].kind; r[1] = j[k].entry; r[2] = j[k].src; r[3] = j[k].dst; r[4] = j[k].len; }
  if (l.size() <= locals_cap && !l.empty()) memcpy(locals, l.data(), l.size());
  if (t.size() <= tail_cap) memcpy(tail, t.data(), t.size());
  return len;
}

}

#ifdef ZIP_PLAN_MAIN
// sum of (k + 1) * byte k over the bytes of a then b, mod 2 ** 64
static uint64_t wsum(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b) {
  uint64_t h = 0, k = 0;
  for (uint8_t x : a) h += ++k * x;
  for (uint8_t x : b) h += ++k * x;
  return h;
}
// input: per list a line "count store encrypted base limit bz_limit lit_limit", then count lines "d_data n name_len time flags method lit src bytes reg zt";
// byte j of entry i's name is 'a' + (7 * i + j) % 26, byte j of its encryption header (3 * i + 5 * j) % 256.
// output: per list a line "bound | groups: g1/kind ... | archive_len | sum of (k + 1) * byte k over the local headers, then the tail | jobs: count, sum of
// (kind + 3 * entry + 5 * src + 7 * dst + 11 * len) mod 2 ** 64 | results: sum of (zip_type + 3 * crc + 5 * csize + 7 * offset)"
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int count, store, enc;
  unsigned long long base, limit, bz_limit, lit_limit;
  while (fscanf(f, "%d %d %d %llu %llu %llu %llu", &count, &store, &enc, &base, &limit, &bz_limit, &lit_limit) == 7) {
    // exact-size heap blocks: a read or a write beyond a table or a name is the sanitizer's to see
    const size_t c1 = count ? (size_t)count : 1;
    zada_zip_entry *ent = (zada_zip_entry *)malloc(c1 * sizeof(zada_zip_entry));
    int *m = (int *)malloc(c1 * sizeof(int));
    uint64_t *lit = (uint64_t *)malloc(c1 * 8), *src = (uint64_t *)malloc(c1 * 8), *bytes = (uint64_t *)malloc(c1 * 8);
    uint32_t *reg = (uint32_t *)malloc(c1 * 4);
    uint16_t *zt = (uint16_t *)malloc(c1 * 2);
    uint8_t *hdr12 = (uint8_t *)malloc(c1 * 12);
    zada_zip_result *res = (zada_zip_result *)malloc(c1 * sizeof(zada_zip_result));
    std::vector<uint8_t *> names;
    for (int i = 0; i < count; i++) {
      unsigned long long a, n, lt, sr, by;
      unsigned nl, tm, fl, rg, z;
      int me;
      if (fscanf(f, "%llu %llu %u %u %u %d %llu %llu %llu %u %u", &a, &n, &nl, &tm, &fl, &me, &lt, &sr, &by, &rg, &z) != 11) return 2;
      uint8_t *nm = (uint8_t *)malloc(nl ? nl : 1);
      for (unsigned j = 0; j < nl; j++) nm[j] = (uint8_t)('a' + (7u * (unsigned)i + j) % 26u);
      names.push_back(nm);
      ent[i] = zada_zip_entry{(const void *)(uintptr_t)a, n, nm, nl, tm, fl};
      m[i] = me; lit[i] = lt; src[i] = sr; bytes[i] = by; reg[i] = rg; zt[i] = (uint16_t)z;
      for (unsigned j = 0; j < 12; j++) hdr12[12 * (size_t)i + j] = (uint8_t)(3u * (unsigned)i + 5u * j);
    }
    printf("%llu | groups:", (unsigned long long)zw_bound_ex(count, ent, base, enc != 0));
    std::vector<ZwGroup> groups;
    std::vector<uint8_t> l, t;
    std::vector<ZwJob> j;
    const uint64_t len = plan_archive_ex(ent, count, store, m, lit, base, limit, bz_limit, lit_limit, src, bytes, reg, zt, enc ? hdr12 : nullptr, groups, l, t, j, res);
    for (const ZwGroup &g : groups) printf(" %d/%d", g.g1, g.kind);
    uint64_t sum = 0, rsum = 0;
    for (const ZwJob &J : j) sum += J.kind + 3ull * J.entry + 5ull * J.src + 7ull * J.dst + 11ull * J.len;
    for (int i = 0; i < count; i++) rsum += res[i].zip_type + 3ull * res[i].crc + 5ull * res[i].csize + 7ull * res[i].offset;
    printf(" | %llu | %llu | jobs: %llu %llu | results: %llu\n", (unsigned long long)len, (unsigned long long)wsum(l, t), (unsigned long long)j.size(), (unsigned long long)sum,
           (unsigned long long)rsum);
    for (uint8_t *nm : names) free(nm);
    free(ent); free(m); free(lit); free(src); free(bytes); free(reg); free(zt); free(hdr12); free(res);
  }
  fclose(f);
  printf("plan ok\n");
  return 0;
}
#endif
