// zip_plan_host.cpp -- the host plan of zada_zip_device (zip-ada_amd/csrc/zada_zip_plan.h) for the CPU tests: a C interface for ctypes
// (tests/test_zip_plan.py), and -- with -DZIP_PLAN_MAIN -- a program of its own that reads entry lists from a text file and prints what the plan
// makes of them, which the test builds with -fsanitize=address,undefined and runs as a child process.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_zip_plan.h"

using namespace zada;

// The whole plan of one call as zada_zip_device walks it: the groups in order, every group placed from its verdicts (bytes [i] of Deflate stream --
// 64 bits here; a batch's are below 2 ** 32 -- at base [i] of the workspace, the running register reg [i]).  Returns the archive's length.
static uint64_t plan_archive(const zada_zip_entry *ent, int count, int method, uint64_t base, uint64_t limit, const uint64_t *bytes, const uint32_t *wbase,
                             const uint32_t *reg, std::vector<uint8_t> &locals, std::vector<uint8_t> &tail, std::vector<ZwJob> &jobs, zada_zip_result *res) {
  ZwArchive A;
  A.base = base;
  std::vector<ZwGroup> groups;
  zw_groups(ent, count, method, limit, groups);
  for (const ZwGroup &g : groups) {
    if (g.kind == ZW_G_SINGLE) zw_single_place(A, ent, g.g0, bytes[g.g0] >= ent[g.g0].n, bytes[g.g0], reg[g.g0], locals, jobs, res);
    else {
      std::vector<uint32_t> b32;
      for (int i = g.g0; i < g.g1; i++) b32.push_back((uint32_t)bytes[i]);
      zw_group_place(A, ent, g.g0, g.g1, g.kind == ZW_G_STORE ? nullptr : b32.data(), wbase + g.g0, reg + g.g0, locals, jobs, res);
    }
  }
  zw_finish(A, tail);
  return A.pos;
}

extern "C" {

int zp_method_ok(int m) { return zw_method_ok(m) ? 1 : 0; }
const char *zp_method_name(int m) { return zw_method_name(m); }
int zp_check(const zada_zip_entry *ent, int count, uint64_t d_archive, uint64_t cap, int *bad, int *why) { return zw_check(ent, count, d_archive, cap, bad, why); }
const char *zp_why_text(int why) { return zw_why_text(why); }
uint64_t zp_bound(int count, const zada_zip_entry *ent, uint64_t base) { return zw_bound(count, ent, base); }
// the groups: up to cap of them into g1 / kind; returns how many there are
int zp_groups(const zada_zip_entry *ent, int count, int method, uint64_t limit, int *g1, int *kind, int cap) {
  std::vector<ZwGroup> g;
  zw_groups(ent, count, method, limit, g);
  for (size_t i = 0; i < g.size() && (int)i < cap; i++) { g1[i] = g[i].g1; kind[i] = g[i].kind; }
  return (int)g.size();
}
// add_compressed entry after entry and finish, from given (crc, csize, zip_type); ent [i].n is the uncompressed size.  The local headers go one behind
// the other into locals (local_at [count + 1]: where each begins), the directory and the end records into tail; offset [i]: the header's place in
// the archive.  Returns the archive's length; a buffer that is too small gets nothing (*_need say what it takes).
uint64_t zp_headers(const zada_zip_entry *ent, int count, uint64_t base, const uint32_t *crc, const uint64_t *csize, const uint16_t *zt, uint8_t *locals, uint64_t locals_cap,
                    uint64_t *locals_need, uint64_t *local_at, uint64_t *offset, uint8_t *tail, uint64_t tail_cap, uint64_t *tail_need) {
  ZwArchive A;
  A.base = base;
  std::vector<uint8_t> l, t;
  for (int i = 0; i < count; i++) {
    local_at[i] = l.size(); offset[i] = A.base + A.pos;
    zw_add(A, ent[i], crc[i], csize[i], ent[i].n, zt[i], l);
  }
  local_at[count] = l.size();
  zw_finish(A, t);
  *locals_need = l.size(); *tail_need = t.size();
  if (l.size() <= locals_cap && !l.empty()) memcpy(locals, l.data(), l.size());
  if (t.size() <= tail_cap) memcpy(tail, t.data(), t.size());
  return A.pos;
}
// the whole plan from verdicts (plan_archive): up to jobs_cap jobs as five values each (kind, entry, src, dst, len) into jobs, *njobs of them; the
// results into res; the local headers (in job order) and the tail as zp_headers gives them.  Returns the archive's length.
uint64_t zp_archive(const zada_zip_entry *ent, int count, int method, uint64_t base, uint64_t limit, const uint64_t *bytes, const uint32_t *wbase, const uint32_t *reg,
                    uint64_t *jobs, uint64_t jobs_cap, uint64_t *njobs, zada_zip_result *res, uint8_t *locals, uint64_t locals_cap, uint64_t *locals_need, uint8_t *tail,
                    uint64_t tail_cap, uint64_t *tail_need) {
  std::vector<uint8_t> l, t;
  std::vector<ZwJob> j;
  const uint64_t len = plan_archive(ent, count, method, base, limit, bytes, wbase, reg, l, t, j, res);
  *njobs = j.size(); *locals_need = l.size(); *tail_need = t.size();
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
// input: per list a line "count method base limit d_archive cap", then count lines "d_data n name_len time flags bytes wbase reg"; byte j of entry i's
// name is 'a' + (7 * i + j) % 26.
// output: per list a line "rc bad why | bound | groups: g1/kind ... | archive_len | sum of (k + 1) * byte k over the local headers, then the tail | jobs: count, sum of
// (kind + 3 * entry + 5 * src + 7 * dst + 11 * len) mod 2 ** 64"
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int count, method;
  unsigned long long base, limit, d_archive, cap;
  while (fscanf(f, "%d %d %llu %llu %llu %llu", &count, &method, &base, &limit, &d_archive, &cap) == 6) {
    // exact-size heap blocks: a read or a write beyond a table or a name is the sanitizer's to see
    zada_zip_entry *ent = (zada_zip_entry *)malloc(count ? (size_t)count * sizeof(zada_zip_entry) : 1);
    uint64_t *bytes = (uint64_t *)malloc(count ? (size_t)count * 8 : 1);
    uint32_t *wbase = (uint32_t *)malloc(count ? (size_t)count * 4 : 1), *reg = (uint32_t *)malloc(count ? (size_t)count * 4 : 1);
    zada_zip_result *res = (zada_zip_result *)malloc(count ? (size_t)count * sizeof(zada_zip_result) : 1);
    std::vector<uint8_t *> names;
    for (int i = 0; i < count; i++) {
      unsigned long long a, n, by;
      unsigned nl, tm, fl, wb, rg;
      if (fscanf(f, "%llu %llu %u %u %u %llu %u %u", &a, &n, &nl, &tm, &fl, &by, &wb, &rg) != 8) return 2;
      const unsigned keep = nl <= 65535u ? nl : 0;                              // (a name that is refused is never read)
      uint8_t *nm = (uint8_t *)malloc(keep ? keep : 1);
      for (unsigned j = 0; j < keep; j++) nm[j] = (uint8_t)('a' + (7u * (unsigned)i + j) % 26u);
      names.push_back(nm);
      ent[i] = zada_zip_entry{(const void *)(uintptr_t)a, n, nm, nl, tm, fl};
      bytes[i] = by; wbase[i] = wb; reg[i] = rg;
    }
    int bad, why;
    const int rc = zw_check(ent, count, d_archive, cap, &bad, &why);
    printf("%d %d %d | %llu | groups:", rc, bad, why, (unsigned long long)zw_bound(count, ent, base));
    std::vector<ZwGroup> groups;
    zw_groups(ent, count, method, limit, groups);
    for (const ZwGroup &g : groups) printf(" %d/%d", g.g1, g.kind);
    if (rc == 0) {
      std::vector<uint8_t> l, t;
      std::vector<ZwJob> j;
      const uint64_t len = plan_archive(ent, count, method, base, limit, bytes, wbase, reg, l, t, j, res);
      uint64_t sum = 0;
      for (const ZwJob &J : j) sum += J.kind + 3ull * J.entry + 5ull * J.src + 7ull * J.dst + 11ull * J.len;
      printf(" | %llu | %llu | jobs: %llu %llu", (unsigned long long)len, (unsigned long long)wsum(l, t), (unsigned long long)j.size(), (unsigned long long)sum);
    }
    printf("\n");
    for (uint8_t *nm : names) free(nm);
    free(ent); free(bytes); free(wbase); free(reg); free(res);
  }
  fclose(f);
  printf("plan ok\n");
  return 0;
}
#endif
