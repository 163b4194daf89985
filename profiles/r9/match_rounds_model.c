/* match_rounds_model.c -- how many rounds of its lane a position of k_match costs, on the CPU.
 *
 *   gcc -O2 profiles/r9/match_rounds_model.c zip-ada_amd/csrc/silesia_mix.c -lm -o match_rounds_model && ./match_rounds_model
 *
 * One stream of 8 MiB of silesia_mix_v2 (at offsets 0 and 512 MiB), Deflate_3's row (nice_match 258).  Chains are the kernel's: positions
 * with the same hashL_of (v, 5), window MAX_DIST.  A search starts at best = 4 (the nearest four-byte match) where one exists and the
 * chain's head lies in the window ("walked").  A round of a lane = up to 12 fast steps (follow the link, two-byte filter at best-1, best;
 * stop at a candidate that passes, or whose successor lies beyond the window) and a slow phase with two eight-byte compare turns; a longer
 * compare goes on in the following rounds.  A search is cut after `budget` rounds that end walking (a guess).
 * Not modelled: segments, chain-length limits (heavy buckets), quarter limits, the queue, the refill's own cost.
 *
 * Variants: the first K candidates settled before the walk, in the fetch, with the compare bounded there at T turns (a first candidate
 * whose compare does not end within the bound leaves the position on today's path; with K > 1 the later ones stop there).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void zada_silesia_mix_v2(uint64_t seed, unsigned class_mask, uint64_t offset, uint64_t len, uint8_t *dst);

enum { MAX_DIST = 32506, FAST = 12, TURNS = 2, NICE = 258 };
#define N (8u << 20)

static uint8_t *in;
static int32_t *prev5, *d4;

static uint32_t hash5(const uint8_t *p) {
  uint32_t x; memcpy(&x, p, 4);
  return (x * 2654435761u + (uint32_t)p[4] * 0x9E3779B1u) >> 16;
}
static uint32_t hash4(const uint8_t *p) { uint32_t x; memcpy(&x, p, 4); return (x * 2654435761u) >> 16; }

static int match_len(uint32_t a, uint32_t b, int la) { int l = 0; while (l < la && in[a + l] == in[b + l]) l++; return l; }

struct Tot { double walked, rounds, steps, rounds_with_steps, guesses, first_pass, in_fetch_seen, in_fetch_done; };

/* one position; K candidates examined in the fetch (0 = today), compare bound T turns there, budget rounds */
static void search(uint32_t p, int K, int T, int budget, struct Tot *t) {
  const int la = N - p < 258 ? (int)(N - p) : 258;
  if (la < 5 || d4[p] == 0 || prev5[p] < 0 || p - (uint32_t)prev5[p] > MAX_DIST - 1) return;
  t->walked++;
  int best = 4;
  int32_t cur = prev5[p];
  int first = 1;
  /* ---- in the fetch ---- */
  for (int k = 0; k < K; k++) {
    const int pass = in[cur + best - 1] == in[p + best - 1] && in[cur + best] == in[p + best];
    if (k == 0 && pass) t->first_pass++;
    if (pass) {
      const int len = match_len((uint32_t)cur, p, la);
      const int ended = len < 8 * T || la <= 8 * T;         /* a mismatch within the bound, or the end of the data */
      if (!ended) break;                                    /* on the walker's path from this candidate on */
      if (len > best) best = len;
    }
    first = 0;
    t->in_fetch_seen += k == 0;
    const int32_t nx = prev5[cur];
    if (best >= NICE || best >= la || nx < 0 || p - (uint32_t)nx > MAX_DIST - 1) { t->in_fetch_done++; return; }
    cur = nx;
  }
  /* ---- the walker ---- */
  int age = 0;
  for (;;) {
    /* fast phase */
    int steps = 0, stopped = 0, pass = 0;
    int32_t nx = -1;
    while (steps < FAST) {
      steps++;
      pass = in[cur + best - 1] == in[p + best - 1] && in[cur + best] == in[p + best];
      nx = prev5[cur];
      const int beyond = nx < 0 || p - (uint32_t)nx > MAX_DIST - 1;
      if (pass || beyond) { stopped = 1; break; }
      cur = nx;
    }
    t->rounds++; t->rounds_with_steps++; t->steps += steps;
    if (first && pass && steps == 1 && K == 0) t->first_pass++;
    first = 0;
    if (stopped) {
      int fin = 0;
      if (pass) {
        const int len = match_len((uint32_t)cur, p, la);
        /* two turns in the round that found it; every further pair of turns is a round of its own */
        int done_bytes = 8 * TURNS;
        while (len >= done_bytes && done_bytes < la) { t->rounds++; done_bytes += 8 * TURNS; }
        if (len > best) { best = len; if (len >= NICE || len >= la) fin = 1; }
      }
      if (nx < 0 || p - (uint32_t)nx > MAX_DIST - 1) fin = 1;
      if (fin) return;
      cur = nx;
    }
    if (++age >= budget) { t->guesses++; return; }
  }
}

static void run(const char *name, int K, int T, int budget, double base) {
  struct Tot t; memset(&t, 0, sizeof t);
  for (uint32_t p = 0; p + 8 < N; p++) search(p, K, T, budget, &t);
  const double r = t.rounds / t.walked;
  printf("%-52s walked %5.1f %%  first passes %5.1f %%  rounds/walked %.3f", name, 100.0 * t.walked / N, 100.0 * t.first_pass / t.walked, r);
  if (base > 0) printf(" (%+5.1f %%)", 100.0 * (r / base - 1.0));
  printf("  fast steps/round %4.1f  in fetch: seen %5.1f %% done %5.1f %% of walked  guesses %5.1f %% of walked\n", t.steps / t.rounds_with_steps,
         100.0 * t.in_fetch_seen / t.walked, 100.0 * t.in_fetch_done / t.walked, 100.0 * t.guesses / t.walked);
}

int main(void) {
  in = malloc(N + 64); prev5 = malloc(4ull * N); d4 = malloc(4ull * N);
  static int32_t head[65536];
  for (int pass = 0; pass < 2; pass++) {
    const uint64_t off = pass ? 512ull << 20 : 0;
    memset(in, 0, N + 64);
    zada_silesia_mix_v2(0x5A1E51A, 0x1F, off, N, in);
    /* chains of the five-byte hash, and the nearest four-byte match (through chains of a four-byte hash) */
    for (int i = 0; i < 65536; i++) head[i] = -1;
    for (uint32_t p = 0; p < N; p++) { const uint32_t h = hash5(in + p); prev5[p] = head[h]; head[h] = (int32_t)p; }
    for (int i = 0; i < 65536; i++) head[i] = -1;
    int32_t *prev4 = malloc(4ull * N);
    for (uint32_t p = 0; p < N; p++) {
      const uint32_t h = hash4(in + p);
      prev4[p] = head[h]; head[h] = (int32_t)p;
      d4[p] = 0;
      for (int32_t q = prev4[p]; q >= 0 && p - (uint32_t)q <= MAX_DIST - 1; q = prev4[q])
        if (!memcmp(in + q, in + p, 4)) { d4[p] = (int32_t)(p - (uint32_t)q); break; }
    }
    free(prev4);
    printf("== silesia_mix_v2, 8 MiB at offset %llu MiB ==\n", (unsigned long long)(off >> 20));
    struct Tot t; memset(&t, 0, sizeof t);
    for (uint32_t p = 0; p + 8 < N; p++) search(p, 0, 0, 6, &t);
    const double base = t.rounds / t.walked;
    run("today, budget 6", 0, 0, 6, 0);
    run("first candidate in fetch (2 turns), budget 6", 1, 2, 6, base);
    run("first candidate in fetch (2 turns), budget 5", 1, 2, 5, base);
    run("first candidate in fetch (1 turn), budget 6", 1, 1, 6, base);
    run("first candidate in fetch (4 turns), budget 6", 1, 4, 6, base);
    run("first two candidates in fetch (2 turns), budget 6", 2, 2, 6, base);
    run("first three candidates in fetch (2 turns), budget 6", 3, 2, 6, base);
  }
  return 0;
}
