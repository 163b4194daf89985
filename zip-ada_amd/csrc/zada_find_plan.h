// zada_find_plan.h -- the host plan and the lane arithmetic of Find_Zip on the device (zada_find.hip; tools/find_zip.adb): the Latin-1
// upper and lower tables of Ada.Characters.Handling, the check of the string's length, the string as the kernel takes it, upper-casing four and
// sixteen bytes at once, the mask of the bytes equal to the string's last character, the filter on the string's last four bytes, the comparison of
// one lane of the wave-wide confirmation, the groups -- and a CPU model of k_fz_search put together from exactly these pieces, word by word and lane
// by lane as the kernel walks a piece.  Plain C++ plus __host__ __device__ helpers: tests/find/find_plan_host.cpp exposes it to the CPU tests
// (tests/test_find_plan.py).
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/zada.h"
#include "zada_unzip_plan.h"

#ifdef __HIPCC__
#define FZ_HD __host__ __device__ __forceinline__
#else
#define FZ_HD inline
#endif

namespace zada {

constexpr uint32_t FZ_MAX = 1024;                      // find_zip.adb:21, max: the longest string, and the ring's size
constexpr uint32_t FZ_PIECE_LOG = 14;                  // log2 of the bytes one wave of k_fz_search takes (a piece of the table)
constexpr uint64_t FZ_PIECE = 1ull << FZ_PIECE_LOG;
constexpr uint32_t FZ_WAVES = 4;                       // waves (pieces) per workgroup
constexpr uint32_t FZ_SPACES = 0x20202020u;

// Ada.Characters.Handling.To_Upper / To_Lower on Latin-1: a .. z, a-grave .. o-diaeresis and o-stroke .. thorn lose 0x20 (0xF7, the division sign,
// 0xDF, sharp s, and 0xFF, y-diaeresis, have no upper-case form there); A .. Z, 0xC0 .. 0xD6 and 0xD8 .. 0xDE gain it (0xD7 is the multiplication sign).
constexpr uint8_t fz_upper_byte(uint8_t c) { return (c >= 0x61 && c <= 0x7A) || (c >= 0xE0 && c <= 0xF6) || (c >= 0xF8 && c <= 0xFE) ? (uint8_t)(c - 0x20) : c; }
constexpr uint8_t fz_lower_byte(uint8_t c) { return (c >= 0x41 && c <= 0x5A) || (c >= 0xC0 && c <= 0xD6) || (c >= 0xD8 && c <= 0xDE) ? (uint8_t)(c + 0x20) : c; }
struct FzTable { uint8_t v[256]; };
constexpr FzTable fz_make_table(bool upper) {
  FzTable t{};
  for (int c = 0; c < 256; c++) t.v[c] = upper ? fz_upper_byte((uint8_t)c) : fz_lower_byte((uint8_t)c);
  return t;
}
constexpr FzTable FZ_UPPER = fz_make_table(true), FZ_LOWER = fz_make_table(false);

// Prepare_Search_String (find_zip.adb:186-199): more than max characters raise Constraint_Error; an empty string fails on str (stl)
inline int fz_check_len(uint64_t text_len) { return text_len >= 1 && text_len <= FZ_MAX ? ZADA_OK : ZADA_E_INVALID; }

// To_Upper on the four bytes of x at once.  Every sum stays inside its byte: l holds the low seven bits of each byte, and the largest addend is 0x7F.
// Bit 7 of l + (0x80 - v) says "l >= v"; a letter is l in 0x61 .. 0x7A with bit 7 of x clear, or l in 0x60 .. 0x7E other than 0x77 with it set.
FZ_HD uint32_t fz_upper4(uint32_t x) {
  const uint32_t l = x & 0x7F7F7F7Fu;
  const uint32_t ascii = (l + 0x1F1F1F1Fu) & ~(l + 0x05050505u) & ~x;
  const uint32_t latin = (l + 0x20202020u) & ~(l + 0x01010101u) & ((l ^ 0x77777777u) + 0x7F7F7F7Fu) & x;
  return x & ~(((ascii | latin) & 0x80808080u) >> 2);
}
FZ_HD void fz_upper16(uint32_t w[4]) { w[0] = fz_upper4(w[0]); w[1] = fz_upper4(w[1]); w[2] = fz_upper4(w[2]); w[3] = fz_upper4(w[3]); }
// 0x80 in every byte of x that equals the byte c4 repeats four times, 0 in the others (exact: no carry leaves a byte)
FZ_HD uint32_t fz_eq_mask4(uint32_t x, uint32_t c4) {
  const uint32_t y = x ^ c4;
  return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
}
// the dword that begins r bytes (0 .. 3) into lo, hi (what v_alignbyte gives)
FZ_HD uint32_t fz_align(uint32_t hi, uint32_t lo, uint32_t r) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * r)); }
// the sixteen bytes that begin s = 0 .. 15 bytes into the aligned words lo, hi
FZ_HD void fz_funnel(const uint32_t lo[4], const uint32_t hi[4], uint32_t s, uint32_t o[4]) {
  uint32_t x0 = lo[0], x1 = lo[1], x2 = lo[2], x3 = lo[3], x4 = hi[0], x5 = hi[1], x6 = hi[2], x7 = hi[3];
  const uint32_t q = s >> 2, r = s & 3u;
  if (q & 2u) { x0 = x2; x1 = x3; x2 = x4; x3 = x5; x4 = x6; x5 = x7; }
  if (q & 1u) { x0 = x1; x1 = x2; x2 = x3; x3 = x4; x4 = x5; }
  o[0] = fz_align(x1, x0, r); o[1] = fz_align(x2, x1, r); o[2] = fz_align(x3, x2, r); o[3] = fz_align(x4, x3, r);
}
// the first c = 1 .. 15 bytes of the word become spaces: the ring is all spaces when the entry starts (find_zip.adb:38)
FZ_HD void fz_spaces_front(uint32_t w[4], uint32_t c) {
  for (uint32_t d = 0; d < 4; d++) {
    const uint32_t k = c > 4u * d ? c - 4u * d : 0u;
    if (k >= 4u) w[d] = FZ_SPACES;
    else if (k) { const uint32_t m = (1u << (8u * k)) - 1u; w[d] = (w[d] & ~m) | (FZ_SPACES & m); }
  }
}
// bits lo .. hi - 1 of sixteen: the bytes of the word at address a that lie in [a0, a1) (the word holds one at least)
FZ_HD uint32_t fz_range_mask(uint64_t a, uint64_t a0, uint64_t a1) {
  const uint32_t lo = a0 > a ? (uint32_t)(a0 - a) : 0u, hi = a1 - a < 16u ? (uint32_t)(a1 - a) : 16u;
  return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// The string as the kernel takes it: upper-cased when asked, right-aligned in a buffer of max bytes (zeros in front), so that lane L of the
// confirmation owns the buffer's 16-byte word 63 - L.  For the filter: its last four bytes as a dword (pat) under the mask of those that exist
// (pmask: the string's last min (stl, 4) bytes are the dword's high ones), the four in front of them likewise (pat2, pmask2: none for stl <= 4), and
// its last character four times (last4).
struct FzPat { uint32_t len, pat, pmask, pat2, pmask2, last4, fold; };
struct FzNeedle { uint8_t buf[FZ_MAX]; FzPat p; };
inline int fz_needle(const uint8_t *text, uint64_t text_len, uint32_t flags, FzNeedle &N) {
  if (fz_check_len(text_len) != ZADA_OK || !text) return ZADA_E_INVALID;
  memset(&N, 0, sizeof N);
  FzPat &P = N.p;
  P.len = (uint32_t)text_len;
  P.fold = (flags & ZADA_FZ_IGNORE_CASE) ? 1u : 0u;
  uint8_t *s = N.buf + (FZ_MAX - P.len);
  for (uint32_t i = 0; i < P.len; i++) s[i] = P.fold ? FZ_UPPER.v[text[i]] : text[i];
  memcpy(&P.pat, N.buf + FZ_MAX - 4, 4);
  memcpy(&P.pat2, N.buf + FZ_MAX - 8, 4);
  P.pmask = P.len >= 4 ? ~0u : ~0u << (8u * (4u - P.len));
  P.pmask2 = P.len >= 8 ? ~0u : P.len > 4 ? ~0u << (8u * (8u - P.len)) : 0u;
  P.pat &= P.pmask;
  P.pat2 &= P.pmask2;
  P.last4 = (uint32_t)N.buf[FZ_MAX - 1] * 0x01010101u;
  return ZADA_OK;
}

// The filter.  Bit i of the result: the eight bytes that end at byte i of the word w -- prev2 and prev are the two dwords in front of it -- are,
// upper-cased when fold is set, the string's last eight (under pmask2 and pmask: its last min (stl, 8)).  The dwords are the text as it lies in
// memory: To_Upper only ever clears bit 5 of a byte, so with fold a byte can only become the string's last character if it equals it in the other
// seven bits (find_zip.adb:69 on seven bits), and a window of four can only become the string's last four if it equals them there.  A dword without
// such a byte is left at once; the four windows of the others are formed without a branch; the few that pass are upper-cased and compared exactly,
// and then the four bytes in front of them.
FZ_HD uint32_t fz_filter16(const uint32_t w[4], uint32_t prev2, uint32_t prev, const FzPat &P) {
  const uint32_t cm = P.fold ? 0xDFDFDFDFu : ~0u, l4 = P.last4 & cm, pm = P.pmask & cm;
  uint32_t m = 0, lo2 = prev2, lo = prev;
  for (uint32_t d = 0; d < 4; d++) {
    const uint32_t cur = w[d];
    if (fz_eq_mask4(cur & cm, l4)) {
      uint32_t c = ((fz_align(cur, lo, 1) ^ P.pat) & pm ? 0u : 1u) | ((fz_align(cur, lo, 2) ^ P.pat) & pm ? 0u : 2u) |
                   ((fz_align(cur, lo, 3) ^ P.pat) & pm ? 0u : 4u) | ((cur ^ P.pat) & pm ? 0u : 8u);
      for (; c; c &= c - 1) {
        const uint32_t i = (uint32_t)__builtin_ctz(c);
        uint32_t x = i == 3u ? cur : fz_align(cur, lo, i + 1u), y = i == 3u ? lo : fz_align(lo, lo2, i + 1u);
        if (P.fold) { x = fz_upper4(x); y = fz_upper4(y); }
        if (!((x ^ P.pat) & P.pmask) && !((y ^ P.pat2) & P.pmask2)) m |= 1u << (4u * d + i);
      }
    }
    lo2 = lo; lo = cur;
  }
  return m;
}
// The confirmation of an end position e, lane L of 64: the lane owns the string's bytes [stl - 16 (L + 1), stl - 16 L) -- word 63 - L of the buffer --
// of which the last nv exist, and compares them with the text's bytes [e + 1 - 16 (L + 1), e + 1 - 16 L).
FZ_HD uint32_t fz_lane_bytes(uint32_t stl, uint32_t L) { return stl > 16u * L ? (stl - 16u * L < 16u ? stl - 16u * L : 16u) : 0u; }
// t against s in their last nv = 1 .. 16 bytes
FZ_HD bool fz_same_tail(const uint32_t t[4], const uint32_t s[4], uint32_t nv) {
  const uint32_t skip = 16u - nv;
  uint32_t diff = 0;
  for (uint32_t d = 0; d < 4; d++) {
    const uint32_t k = skip > 4u * d ? skip - 4u * d : 0u;
    if (k < 4u) diff |= (t[d] ^ s[d]) & (~0u << (8u * k));
  }
  return diff == 0;
}

// One aligned 16-byte word of the text as the search sees it: word k covers addresses [16 k, 16 k + 16); the entry is [base, end).  A word in front
// of the entry is all spaces and a word behind it all zeros, and NEITHER IS LOADED: ld (address, w) is only called for a word that holds a byte of
// the entry.  Upper-cased when asked; the bytes in front of the entry's first are spaces; the bytes behind its last are whatever lies there -- no
// occurrence that ends inside the entry reaches them.
template <class Load>
FZ_HD void fz_word(const Load &ld, uint64_t k, uint64_t base, uint64_t end, uint32_t fold, uint32_t w[4]) {
  const uint64_t a = k << 4;
  if (a + 16u <= base) { w[0] = w[1] = w[2] = w[3] = FZ_SPACES; return; }
  if (a >= end) { w[0] = w[1] = w[2] = w[3] = 0; return; }
  ld(a, w);
  if (fold) fz_upper16(w);
  if (a < base) fz_spaces_front(w, (uint32_t)(base - a));
}
// the text's sixteen bytes that lane L compares for the end position e (see fz_lane_bytes)
template <class Load>
FZ_HD void fz_lane_text(const Load &ld, uint64_t e, uint32_t L, uint64_t base, uint64_t end, uint32_t fold, uint32_t t[4]) {
  const uint64_t ta = e + 1u - 16u * (uint64_t)(L + 1u);
  uint32_t lo[4], hi[4] = {0, 0, 0, 0};
  fz_word(ld, ta >> 4, base, end, fold, lo);
  if (ta & 15u) fz_word(ld, (ta >> 4) + 1u, base, end, fold, hi);
  fz_funnel(lo, hi, (uint32_t)(ta & 15u), t);
}

// Groups of consecutive rows of zada_findzip_device: the extracted bytes (uz_slot of every cap) within `limit`, or a single row
inline void fz_groups(const zada_unzip_entry *ent, int count, uint64_t limit, std::vector<int> &ends) { uz_groups(ent, count, limit, ends); }
// the argument checks of zada_findzip_device: uz_check's without the output ranges, row by row
inline int fz_check(const zada_unzip_entry *ent, int count, uint64_t archive_len, int have_keys, int *bad, int *why, int legacy = 0) {
  *bad = -1; *why = UZ_W_NONE;
  for (int i = 0; i < count; i++) {
    zada_unzip_entry e = ent[i];
    e.flags &= 3u;
    int k = -1, w = 0;
    const int rc = uz_check(&e, 1, archive_len, 0, 0, have_keys, &k, &w, legacy);
    if (rc) { *bad = i; *why = w; return rc; }
  }
  return ZADA_OK;
}
inline uint64_t fz_piece_count(uint64_t n) { return (n + FZ_PIECE - 1) >> FZ_PIECE_LOG; }

// ---- the CPU model of k_fz_search ----
// mem [0 .. mem_len) stands for device memory, the entry is mem [base, base + n); a load of a word outside mem, or of one that holds no byte of the
// entry, sets *bad.  The pieces of the entry one after the other, each as a wave walks it: the words of the piece, the filter, and for a string of
// more than eight bytes the confirmation by sixty-four lanes.  occurrences and first as zada_find_device gives them.
struct FzModelLoad {
  const uint8_t *mem; uint64_t mem_len, base, end; int *bad;
  void operator()(uint64_t a, uint32_t w[4]) const {
    if (a + 16u > mem_len || a + 16u <= base || a >= end) { *bad = 1; w[0] = w[1] = w[2] = w[3] = 0; return; }
    memcpy(w, mem + a, 16);
  }
};
inline void fz_model(const uint8_t *mem, uint64_t mem_len, uint64_t base, uint64_t n, const FzNeedle &N, uint64_t *occurrences, uint64_t *first, int *bad) {
  *occurrences = 0; *first = n; *bad = 0;
  const uint64_t end = base + n;
  const FzModelLoad ld{mem, mem_len, base, end, bad};
  for (uint64_t off = 0; off < n; off += FZ_PIECE) {
    const uint64_t a0 = base + off, a1 = a0 + (n - off < FZ_PIECE ? n - off : FZ_PIECE);
    for (uint64_t k = a0 >> 4; k <= (a1 - 1) >> 4; k++) {
      uint32_t w[4], p[4];
      fz_word(ld, k, base, end, 0, w);                              // (as it lies in memory: the filter folds what it has to)
      fz_word(ld, k - 1, base, end, 0, p);
      uint32_t m = fz_filter16(w, p[2], p[3], N.p) & fz_range_mask(k << 4, a0, a1);
      for (; m; m &= m - 1) {
        const uint64_t e = (k << 4) + (uint32_t)__builtin_ctz(m);
        bool hit = true;
        for (uint32_t L = 0; N.p.len > 8 && L < 64; L++) {
          const uint32_t nv = fz_lane_bytes(N.p.len, L);
          if (!nv) continue;
          uint32_t t[4], s[4];
          fz_lane_text(ld, e, L, base, end, N.p.fold, t);
          memcpy(s, N.buf + 16u * (63u - L), 16);
          hit = hit && fz_same_tail(t, s, nv);
        }
        if (hit) { ++*occurrences; if (e - base < *first) *first = e - base; }
      }
    }
  }
}

}  // namespace zada
