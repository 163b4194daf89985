// Stand-alone check of zip-ada_amd/csrc/zada_descr_bound.h (tests/test_descr_bound.py builds it with -fsanitize=address,undefined and runs it
// as a child process).  Reads a file of cases written by the test:
//   header   uint32 count
//   case     uint8 ref [320], uint8 win [320]   code lengths of the reference descriptor and of the window's (the oracle's coder)
//            uint32 U [10], uint32 D [10]       what the scan would know about the window: may use / does use (D in U, U covers the window)
// For every case: descr_bound (ref, U, D) >= L1_tweaked (ref, win), and so is the plain bound (kraft = false).  Prints one line:
//   cases <n> violations <v> plain_violations <p> decided <d> plain_decided <q> max_slack_ratio_x1000 <r>
// and, for the cases 0 and 1 (the directed ones, see the test), "directed <k> true <t> bound <b> plain <p>".
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_descr_bound.h"

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) { fprintf(stderr, "short file\n"); return 2; }
  std::vector<uint8_t> ref(320), win(320);
  std::vector<uint32_t> U(zada::DB_WORDS), D(zada::DB_WORDS);
  uint64_t viol = 0, pviol = 0, decided = 0, pdecided = 0, bad_sets = 0;
  for (uint32_t k = 0; k < count; k++) {
    if (fread(ref.data(), 1, 320, f) != 320 || fread(win.data(), 1, 320, f) != 320 || fread(U.data(), 4, zada::DB_WORDS, f) != (size_t)zada::DB_WORDS ||
        fread(D.data(), 4, zada::DB_WORDS, f) != (size_t)zada::DB_WORDS) { fprintf(stderr, "short case %u\n", k); return 2; }
    // the premises: every symbol the window codes is in U, every symbol of D is coded, no length above 15
    for (int s = 0; s < 320; s++) {
      if (ref[s] > 15 || win[s] > 15) bad_sets++;
      if (win[s] && !zada::db_has(U.data(), s)) bad_sets++;
      if (zada::db_has(D.data(), s) && (!win[s] || !zada::db_has(U.data(), s))) bad_sets++;
    }
    const uint32_t t = zada::descr_l1_tweaked(ref.data(), win.data());
    const uint32_t b = zada::descr_bound(ref.data(), U.data(), D.data()), p = zada::descr_bound(ref.data(), U.data(), D.data(), false);
    if (b < t) { if (!viol) fprintf(stderr, "case %u: bound %u < true %u\n", k, b, t); viol++; }
    if (p < t) { if (!pviol) fprintf(stderr, "case %u: plain bound %u < true %u\n", k, p, t); pviol++; }
    if (b < zada::DB_L3_CUT) decided++;
    if (p < zada::DB_L3_CUT) pdecided++;
    if (k < 2) printf("directed %u true %u bound %u plain %u\n", k, t, b, p);
  }
  fclose(f);
  printf("cases %u violations %llu plain_violations %llu decided %llu plain_decided %llu bad_sets %llu\n", count, (unsigned long long)viol,
         (unsigned long long)pviol, (unsigned long long)decided, (unsigned long long)pdecided, (unsigned long long)bad_sets);
  return viol || pviol || bad_sets ? 1 : 0;
}
