// zada_descr_bound.h -- an upper bound on the Taillaule splitter's similarity distance (L1_tweaked,
// zip-compress-deflate.adb:379-433, 457-490) between the reference descriptor and a sliding window's descriptor,
// taken from the reference's code lengths and from WHICH symbols the window uses -- without building the window's
// descriptor.  Host + device, like zada_logic.h; the host compiles it only in tests (tests/hostcheck).
//
// What is known about window symbol s, per alphabet (literal/length 0..287, distance 288..319: two separate codes):
//   s not in U          the window does not use s: its length is 0, its tweak 1600; the term is exactly 1600 - t_ref
//   s in U, not in D    the window may use s (U is a superset): length 0 or 1..15, tweak in [100, 1600]
//   s in D  (D in U)    the window does use s: length 1..15 (a used symbol of a length-limited code has a code of at
//                       most 15 bits), tweak in [100, 1513]
// So a term is at most long_s = 1600 - t_ref (1513 - t_ref, at least 0, for s in D) when the window's code of s is not
// shorter than the reference's, and t_ref - tweak (l) when it is l bits and shorter.  Kraft's inequality lets at most
// 2^L symbols of one code have L bits or fewer, so the i-th shortest code of ANY prefix code has at least lambda_i =
// 1, 1, 2, 2, 3, 3, 3, 3, 4 ... bits.  With A_s = t_ref - long_s, the symbols that are shorter in the window add
//   sum (A_s - tweak (l_s))  <=  sum over ranks r of max (0, A_(r) - tweak (lambda_r))        (A_(r): descending)
// to the sum of all long_s: the left side takes some set of symbols, whose A are at most the largest ones, and their
// lengths, sorted, are at least lambda.  A_s depends only on the reference's length of s (16 values) and on s in D (2):
// 32 bins per alphabet, counted, then ranked bin by bin.
//
// The distance statistics go through Patch_statistics_for_buggy_decoders (:340-365) before they are coded, which makes
// symbols 288 and 289 used when fewer than two distance symbols are: db_patch_dist adds them to U unless D already
// proves two.  The end-of-block symbol 256 is counted once in every window (:946): the caller puts it into D.
#pragma once
#include "zada_logic.h"

namespace zada {

constexpr uint32_t DB_L3_CUT = 2050u * 100u;   // step level 3 cuts at L1_tweaked >= 2050 * 100 (:1304-1308, :480-488)
constexpr int DB_WORDS = 10;                    // 320 presence bits: symbol s is bit s & 31 of word s >> 5
constexpr int DB_BINS = 32;                     // per alphabet: the reference's length of the symbol (0 .. 15) * 2 + (s in D)

ZADA_HD bool db_has(const uint32_t *m, int s) { return ((m[s >> 5] >> (s & 31)) & 1u) != 0; }
ZADA_HD int db_popc(uint32_t x) { int n = 0; while (x) { x &= x - 1; n++; } return n; }
ZADA_HD void db_patch_dist(uint32_t *U, const uint32_t *D) { if (db_popc(D[9]) < 2) U[9] |= 3u; }

ZADA_HD int db_long(int t_ref, bool definite) { const int m = (definite ? 1513 : 1600) - t_ref; return m > 0 ? m : 0; }
ZADA_HD int db_bin_value(int b) { const int t = tweak_value(b >> 1); return t - db_long(t, (b & 1) != 0); }   // A of the bin

// the part of symbol s that does not depend on the other symbols; bin: where it is counted (-1: not in U)
ZADA_HD uint32_t db_sym(int ref_bl, bool in_u, bool in_d, int &bin) {
  const int t = tweak_value(ref_bl);
  if (!in_u) { bin = -1; return (uint32_t)(1600 - t); }
  bin = ref_bl * 2 + (in_d ? 1 : 0);
  return (uint32_t)db_long(t, in_d);
}

// what the symbols of bin b can add by being shorter in the window, given the counts of all bins of its alphabet
ZADA_HD uint32_t db_bin_extra(const uint32_t *cnt, int b) {
  const uint32_t n = cnt[b];
  if (!n) return 0;
  const int v = db_bin_value(b);
  uint32_t r0 = 0;                                   // ranks [r0, r0 + n) in the descending order of A
  for (int o = 0; o < DB_BINS; o++) { const int vo = db_bin_value(o); if (vo > v || (vo == v && o < b)) r0 += cnt[o]; }
  uint32_t ex = 0;
  for (int L = 1; L <= 15; L++) {                    // ranks [2^(L-1), 2^L) have lambda = L (rank 0 as well: L = 1)
    const int g = v - tweak_value(L);
    if (g <= 0) break;
    const uint32_t lo = L == 1 ? 0u : 1u << (L - 1), hi = 1u << L;
    const uint32_t a = r0 > lo ? r0 : lo, e = r0 + n < hi ? r0 + n : hi;
    if (e > a) ex += (e - a) * (uint32_t)g;
    if (hi >= r0 + n) break;
  }
  return ex;
}

// The bound, serially (the scan kernel spreads the same functions over a wave: five symbols and one bin per lane).
// ref_bl: the reference descriptor's 320 code lengths, 0 = unused (their tweak_value is what the metric compares).
// kraft = false: the plain bound max (1600 - t_ref, t_ref - 100) for every symbol of U, D ignored.
ZADA_HD uint32_t descr_bound(const uint8_t *ref_bl, const uint32_t *U, const uint32_t *D, bool kraft = true) {
  uint32_t cnt[2][DB_BINS];
  for (int a = 0; a < 2; a++) for (int b = 0; b < DB_BINS; b++) cnt[a][b] = 0;
  uint32_t sum = 0;
  for (int s = 0; s < 320; s++) {
    const bool in_u = db_has(U, s);
    if (!kraft) {
      const int t = tweak_value(ref_bl[s]), up = 1600 - t, down = t - 100;
      sum += (uint32_t)(!in_u || up > down ? up : down);
      continue;
    }
    int bin;
    sum += db_sym(ref_bl[s], in_u, in_u && db_has(D, s), bin);
    if (bin >= 0) cnt[s >= 288][bin]++;
  }
  if (kraft) for (int a = 0; a < 2; a++) for (int b = 0; b < DB_BINS; b++) sum += db_bin_extra(cnt[a], b);
  return sum;
}

// the metric itself, for the tests
ZADA_HD uint32_t descr_l1_tweaked(const uint8_t *a, const uint8_t *b) {
  uint32_t d = 0;
  for (int s = 0; s < 320; s++) { const int x = tweak_value(a[s]) - tweak_value(b[s]); d += (uint32_t)(x < 0 ? -x : x); }
  return d;
}

}  // namespace zada
