// The group plan of the readers' batch calls (zip-ada_amd/csrc/zada_reader_plan.h) for the CPU: a C ABI for tests/test_reader_plan.py, and with
// -DREADER_PLAN_MAIN a program of its own that reads lists of entries from a file and prints their plans (built with -fsanitize=address,undefined
// by the same test).
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_reader_plan.h"

using namespace zada;

// one line per list: the groups, each as "g0 g1 in_bytes out_bytes hi io... oo..." behind a bar; wrote [i]: the bytes entry i wrote (0: it failed)
static void plan_line(FILE *f, int count, const uint64_t *n_in, const uint64_t *cap, const uint64_t *wrote, uint64_t limit) {
  for (int g0 = 0; g0 < count;) {
    const ReaderGroup G = reader_plan_group(g0, count, n_in, cap, limit);
    const int E = G.g1 - G.g0;
    std::vector<uint64_t> io(E), oo(E);
    reader_plan_offsets(G, n_in, cap, io.data(), oo.data());
    const uint64_t hi = reader_plan_extent(G, oo.data(), [&](int k) { return wrote[g0 + k]; });
    fprintf(f, "| %d %d %llu %llu %llu", G.g0, G.g1, (unsigned long long)G.in_bytes, (unsigned long long)G.out_bytes, (unsigned long long)hi);
    for (int k = 0; k < E; k++) fprintf(f, " %llu", (unsigned long long)io[k]);
    for (int k = 0; k < E; k++) fprintf(f, " %llu", (unsigned long long)oo[k]);
    g0 = G.g1;
  }
  fprintf(f, "\n");
}

extern "C" {

// rows: g0, g1, in_bytes, out_bytes per group, up to max_groups of them -> the number of groups
int rp_groups(int count, const uint64_t *n_in, const uint64_t *cap, uint64_t limit, uint64_t *rows, int max_groups) {
  int n = 0;
  for (int g0 = 0; g0 < count; n++) {
    const ReaderGroup G = reader_plan_group(g0, count, n_in, cap, limit);
    if (n < max_groups) { rows[4 * n] = (uint64_t)G.g0; rows[4 * n + 1] = (uint64_t)G.g1; rows[4 * n + 2] = G.in_bytes; rows[4 * n + 3] = G.out_bytes; }
    g0 = G.g1;
  }
  return n;
}

// the offsets of the group that begins at g0, and how much of its outputs comes back -> hi
uint64_t rp_layout(int g0, int count, const uint64_t *n_in, const uint64_t *cap, const uint64_t *wrote, uint64_t limit, uint64_t *io, uint64_t *oo) {
  const ReaderGroup G = reader_plan_group(g0, count, n_in, cap, limit);
  reader_plan_offsets(G, n_in, cap, io, oo);
  return reader_plan_extent(G, oo, [&](int k) { return wrote[g0 + k]; });
}

uint64_t rp_pad16(uint64_t x) { return reader_pad16(x); }

}  // extern "C"

#ifdef READER_PLAN_MAIN
// each line of the file: limit count, then count times "n_in cap wrote"
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  unsigned long long limit;
  int count;
  while (fscanf(f, "%llu %d", &limit, &count) == 2) {
    std::vector<uint64_t> n_in(count), cap(count), wrote(count);
    for (int i = 0; i < count; i++) {
      unsigned long long a, b, w;
      if (fscanf(f, "%llu %llu %llu", &a, &b, &w) != 3) return 3;
      n_in[i] = a; cap[i] = b; wrote[i] = w;
    }
    plan_line(stdout, count, n_in.data(), cap.data(), wrote.data(), limit);
  }
  fclose(f);
  printf("plan ok\n");
  return 0;
}
#endif
