/* Stand-alone check of the Shrink and Reduce CPU models, meant to be built with -fsanitize=address,undefined (tests/test_legacy_model.py):
 *   legacy_check COUNT [-mMETHODS | FILE] ...
 * runs the seeded self-tests over COUNT small inputs each, then every FILE through both forms and the decoder of each method in the METHODS
 * given last (digits: 1 Shrink_1, 2 .. 5 Reduce_1 .. _4; at first all five).
 * Exit status 0 when nothing fails. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "shrink_model.c"
#define lcg lcg_reduce
#include "reduce_model.c"

int main(int argc, char **argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 200;
  const char *methods = "12345";
  int bad = shrink_selftest(1, count, NULL) + reduce_selftest(1, count, NULL);
  for (int a = 2; a < argc; a++) {
    if (argv[a][0] == '-' && argv[a][1] == 'm') { methods = argv[a] + 2; continue; }
    FILE *f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *d = (uint8_t *)malloc((size_t)n + 1);
    if (fread(d, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
    fclose(f);
    for (const char *m = methods; *m; m++) {
      if (*m == '1') bad += shrink_check_one(d, (uint64_t)n, NULL);
      else if (*m >= '2' && *m <= '5') bad += reduce_check_one(*m - '1', d, (uint64_t)n, NULL);
    }
    free(d);
  }
  printf("legacy_check: %d failures\n", bad);
  return bad ? 1 : 0;
}
