// zada_rezip_plan.h -- the host plan of the tools built on the archive reader and writer (zada_rezip.hip).  ReZip (tools/rezip_lib.adb):
// the approaches and format sets, the choice as a closed form, the methods to run, ReZip's headers, argument checks, bound and groups.
// Comp_Zip (tools/comp_zip_prc.adb): the verdict on one pair of entries as a closed form, the argument checks of zada_compzip_device, its groups and
// the geometry of the compare kernel's pieces.  Plain C++ without HIP: tests/rezip/rezip_plan_host.cpp exposes it to the CPU tests
// (tests/test_rezip_plan.py).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/zada.h"
#include "zada_unzip_plan.h"
#include "zada_zip_plan.h"

namespace zada {

constexpr uint32_t CZ_PIECE_LOG = 14;                  // log2 of the bytes one wave of k_cz_compare takes (a piece of the table)
constexpr uint64_t CZ_PIECE = 1ull << CZ_PIECE_LOG;
constexpr uint32_t CZ_WAVES = 4;                       // waves (pieces) per workgroup

// Compare_1_file (comp_zip_prc.adb:102-143) as a closed form.  The loop reads one character of each stream at a time, p counting from 1:
//   while not End_Of_File (f1):  End_Of_File (f2) -> "Shorter in 2 at position p";  c1 /= c2 -> "Difference at position p";  p := p + 1
//   then: not End_Of_File (f2) -> "Longer in 2";  else OK, p - 1 bytes compared.
// With la, lb the two lengths, m = min (la, lb) and d the first offset below m at which the bytes differ (d = m: none), the loop meets a difference
// at p = d + 1 before it can meet the end of either stream (d < m); without one it runs m times and then stands at p = m + 1, where la > lb is
// "shorter" (the test comes first in the next turn), la < lb "longer" (the loop has ended) and la = lb is OK with la bytes.
// *compared: the equal bytes in front of the verdict (what total_bytes receives on OK).
inline int cz_verdict(uint64_t la, uint64_t lb, uint64_t d, uint64_t *position, uint64_t *compared) {
  const uint64_t m = la < lb ? la : lb;
  if (d < m) { *position = d + 1; *compared = d; return ZADA_CZ_DIFFERENT; }
  *compared = m;
  if (la > lb) { *position = m + 1; return ZADA_CZ_SHORTER; }
  *position = 0;
  return la < lb ? ZADA_CZ_LONGER : ZADA_CZ_OK;
}

inline bool cz_absent(const zada_unzip_entry &e) { return (e.flags & ZADA_CZ_ABSENT) != 0; }

// The argument checks of zada_compzip_device: uz_check's on every row of archive 1, then on every present row of archive 2 (no output ranges: the
// outputs are workspace).  *side: 1 or 2.  Returns ZADA_OK, ZADA_E_INVALID or ZADA_E_TOO_LARGE.
inline int cz_check(const zada_unzip_entry *a, const zada_unzip_entry *b, int count, uint64_t len_a, uint64_t len_b, int have_keys, int *bad, int *side, int *why,
                    int legacy = 0) {
  *bad = -1; *side = 0; *why = UZ_W_NONE;
  for (int s = 1; s <= 2; s++)
    for (int i = 0; i < count; i++) {
      if (s == 2 && cz_absent(b[i])) continue;
      zada_unzip_entry e = s == 1 ? a[i] : b[i];
      e.flags &= 3u;
      int k = -1, w = 0;
      const int rc = uz_check(&e, 1, s == 1 ? len_a : len_b, 0, 0, have_keys, &k, &w, legacy);
      if (rc) { *bad = i; *side = s; *why = w; return rc; }
    }
  return ZADA_OK;
}

// A pair's slot in each of the two arenas: the same offset in both, so that the two copies of an entry lie at the same 16-byte phase.
inline uint64_t cz_slot(const zada_unzip_entry &a, const zada_unzip_entry &b) { return uz_slot(cz_absent(b) || a.cap > b.cap ? a.cap : b.cap); }
// Groups of consecutive pairs: both arenas of a group within `limit` bytes together -- or a single pair.  A pair whose second row is absent takes no
// room: nothing of it is extracted.  ends receives the index behind every group's last pair.
inline void cz_groups(const zada_unzip_entry *a, const zada_unzip_entry *b, int count, uint64_t limit, std::vector<int> &ends) {
  ends.clear();
  for (int g0 = 0; g0 < count;) {
    uint64_t bytes = 0;
    int g1 = g0, live = 0;
    while (g1 < count) {
      const uint64_t s = cz_absent(b[g1]) ? 0 : 2 * cz_slot(a[g1], b[g1]);
      if (live && s && bytes + s > limit) break;
      bytes += s; live += s != 0; g1++;
    }
    ends.push_back(g1);
    g0 = g1;
  }
}

// The pieces of one pair of n bytes when no table is given (zada_compare_device): piece k covers [k << CZ_PIECE_LOG, ...), the last one shorter.
inline uint64_t cz_piece_count(uint64_t n) { return (n + CZ_PIECE - 1) >> CZ_PIECE_LOG; }

// ---- ReZip (tools/rezip_lib.adb) ----
// The approaches in the reference's order (rezip_lib.adb:79-91); the rank is the bit in the mask.  Method 0: original.  Shrink_1 and Reduce_4 are
// taken only with the knob "zip_legacy" (RZ_UNBUILT: the approaches a call without it refuses).
constexpr int RZ_NA = 12, RZ_ORIGINAL = 0, RZ_PRESEL_2 = 1, RZ_PRESEL_1 = 2, RZ_SHRINK = 3, RZ_REDUCE_4 = 4, RZ_LZMA_3 = 10;
constexpr int RZ_METHOD[RZ_NA] = {0, ZADA_PRESELECTION_2, ZADA_PRESELECTION_1, ZADA_SHRINK_1, ZADA_REDUCE_4, ZADA_DEFLATE_3, ZADA_DEFLATE_R, ZADA_BZIP2_3, ZADA_BZIP2_2, ZADA_BZIP2_1,
                                  ZADA_LZMA_3, ZADA_LZMA_2};
constexpr uint32_t RZ_BUILT = 0x0FE7, RZ_UNBUILT = (1u << RZ_SHRINK) | (1u << RZ_REDUCE_4);
constexpr uint64_t RZ_SHRINK_MAX = 6000, RZ_REDUCE_4_MAX = 9000;      // the largest entries these two are tried on (rezip_lib.adb:819-832)
constexpr uint64_t RZ_NOT_TRIED = ~0ull;
constexpr uint32_t RZ_MAX_ENTRIES = 65534;
// the bit of a zip type in a format set (Zip.PKZip_Format: store, deflate, deflate_64, bzip2_fmt, lzma_fmt); -1: not one ReZip writes or reads here
inline int rz_format_bit(uint16_t zt) { return zt == 0 ? 0 : zt == 8 ? 1 : zt == 9 ? 2 : zt == 12 ? 3 : zt == 14 ? 4 : -1; }
inline bool rz_format_in(uint32_t formats, uint16_t zt) { const int b = rz_format_bit(zt); return b >= 0 && ((formats >> b) & 1u); }
// consider_a_priori (rezip_lib.adb:1072-1089) over the built approaches of the mask: original always; a single method when its format is in the set;
// the Preselections only with all formats.  legacy (the knob "zip_legacy"): shrink and reduce_4 are single methods whose formats the five-bit mask
// cannot name; such a format counts as in the set exactly when the set is all formats, which is so for every named set of the reference
// (all_formats, deflate_or_store, fast_decompression).  Without it the two are never considered.
inline bool rz_all_formats(uint32_t formats) { return (formats & ZADA_RZ_ALL_FORMATS) == ZADA_RZ_ALL_FORMATS; }
inline uint32_t rz_considered(uint32_t approaches, uint32_t formats, int legacy = 0) {
  uint32_t c = 1u;
  for (int a = 1; a < RZ_NA; a++) {
    if (!((approaches >> a) & 1u)) continue;
    if ((RZ_UNBUILT >> a) & 1u) { if (legacy && rz_all_formats(formats)) c |= 1u << a; continue; }
    const bool multi = a == RZ_PRESEL_1 || a == RZ_PRESEL_2;
    if (multi ? (formats & ZADA_RZ_ALL_FORMATS) == ZADA_RZ_ALL_FORMATS : rz_format_in(formats, zw_zip_type(RZ_METHOD[a]))) c |= 1u << a;
  }
  return c;
}
// The choice (rezip_lib.adb:835-889) as a closed form.  The loop starts at original and walks the considered approaches in rank order; it takes an
// approach that is strictly smaller than the choice, and, while the choice is still original and original's format is not allowed, whatever comes.
// If original's format is allowed (or nothing else is considered), the choice only ever moves to a strictly smaller size, so the loop ends at the
// first approach in rank order that has the smallest size: the minimum of (size, rank) over all of them, original included -- a tie with original
// stays at original, rank 0.  If it is not allowed, the first other considered approach is taken whatever its size, and from there on the rule is
// "strictly smaller" among the others: the minimum of (size, rank) without original.  size [a] = RZ_NOT_TRIED: not considered for this entry.
inline int rz_choose(const uint64_t size[RZ_NA], bool original_allowed) {
  int best = -1;
  for (int a = 1; a < RZ_NA; a++) if (size[a] != RZ_NOT_TRIED && (best < 0 || size[a] < size[best])) best = a;
  if (best < 0) return RZ_ORIGINAL;
  return original_allowed && size[RZ_ORIGINAL] <= size[best] ? RZ_ORIGINAL : best;
}
// The considered approaches of one entry of usize bytes: shrink only up to 6 000 bytes, reduce_4 only up to 9 000 (rezip_lib.adb:819-832); the
// entry's size row says RZ_NOT_TRIED for the others.
inline uint32_t rz_considered_entry(uint32_t considered, uint64_t usize) {
  if (usize > RZ_SHRINK_MAX) considered &= ~(1u << RZ_SHRINK);
  if (usize > RZ_REDUCE_4_MAX) considered &= ~(1u << RZ_REDUCE_4);
  return considered;
}
// original's format is allowed (rezip_lib.adb:880-886): the source's zip type is in the format set; a Shrink, Reduce or Implode source (1 .. 6)
// by the rule of rz_considered, only with all formats.
inline bool rz_original_allowed(uint32_t formats, uint16_t method) { return method >= 1 && method <= 6 ? rz_all_formats(formats) : rz_format_in(formats, method); }
// The method approach a runs on an entry: its single method, or what zada_preselect gave for the entry (p2, p1).
inline int rz_method_of(int a, int p2, int p1) { return a == RZ_PRESEL_2 ? p2 : a == RZ_PRESEL_1 ? p1 : RZ_METHOD[a]; }
// The distinct methods of an entry over its considered approaches, ascending; an (entry, method) pair that serves several approaches is run once.
// usize: the entry's size, for the limits of shrink and reduce_4.
inline void rz_methods(uint32_t considered, int p2, int p1, std::vector<int> &out, uint64_t usize = 0) {
  out.clear();
  considered = rz_considered_entry(considered, usize);
  for (int a = 1; a < RZ_NA; a++) if ((considered >> a) & 1u) out.push_back(rz_method_of(a, p2, p1));
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
}
// An entry ReZip drops: an empty name, or one that ends in '/' or '\' (rezip_lib.adb:752-758)
inline bool rz_dropped(const zada_rezip_entry &e) { return e.name_len == 0 || e.name[e.name_len - 1] == '/' || e.name[e.name_len - 1] == '\\'; }

enum RzWhy { RZ_W_NONE = 0, RZ_W_RANGE, RZ_W_METHOD, RZ_W_ENCRYPTED, RZ_W_DUPLICATE, RZ_W_TOO_LARGE, RZ_W_NAME, RZ_W_OVERLAP, RZ_W_COUNT };
// legacy: the knob "unzip_legacy" is set, so that source methods 1 .. 6 are known (the reader's text then)
inline const char *rz_why_text(int why, int legacy = 0) {
  if (legacy && why == RZ_W_METHOD) return uz_why_text(UZ_W_METHOD, 1);
  switch (why) {
    case RZ_W_RANGE: return "its data lie beyond the source archive";
    case RZ_W_METHOD: return "unknown source method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)";
    case RZ_W_ENCRYPTED: return "encrypted (ReZip reads without a password)";
    case RZ_W_DUPLICATE: return "the same name as an earlier entry";
    case RZ_W_TOO_LARGE: return "a stream or an entry of 1 TiB or more";
    case RZ_W_NAME: return "a name longer than 65 535 bytes (or a null name)";
    case RZ_W_OVERLAP: return "the archive buffer overlaps the source archive";
    case RZ_W_COUNT: return "more than 65 534 entries are kept (the end record holds the count in 16 bits)";
    default: return "";
  }
}
// The argument checks, entry after entry; then the count of kept entries; the overlap of [d_archive, d_archive + cap) with the source is *bad = -1.
inline int rz_check(const zada_rezip_entry *ent, int count, uint64_t d_src, uint64_t src_len, uint64_t d_archive, uint64_t cap, int *bad, int *why,
                    int legacy = 0) {
  *bad = -1; *why = RZ_W_NONE;
  if (src_len && cap && d_src < d_archive + cap && d_archive < d_src + src_len) { *why = RZ_W_OVERLAP; return ZADA_E_INVALID; }
  std::vector<int> order;
  uint32_t kept = 0;
  for (int i = 0; i < count; i++) {
    const zada_rezip_entry &e = ent[i];
    int w = RZ_W_NONE;
    if (e.name_len > 65535u || (e.name_len && !e.name)) w = RZ_W_NAME;
    else if (!uz_method_known(e.method, legacy)) w = RZ_W_METHOD;
    else if (e.flags & 1u) w = RZ_W_ENCRYPTED;
    else if (e.n_in >= UZ_MAX_BYTES || e.usize >= UZ_MAX_BYTES) w = RZ_W_TOO_LARGE;
    else if (e.in_off > src_len || e.n_in > src_len - e.in_off) w = RZ_W_RANGE;
    if (w) { *bad = i; *why = w; return w == RZ_W_TOO_LARGE ? ZADA_E_TOO_LARGE : ZADA_E_INVALID; }
    order.push_back(i);
    if (!rz_dropped(e)) kept++;
  }
  auto less = [&](int a, int b) {
    const uint32_t la = ent[a].name_len, lb = ent[b].name_len;
    const uint32_t lm = la < lb ? la : lb;
    const int c = lm ? memcmp(ent[a].name, ent[b].name, lm) : 0;              // (an empty name may be a null pointer)
    return c ? c < 0 : la != lb ? la < lb : a < b;
  };
  std::sort(order.begin(), order.end(), less);
  int dup = -1;
  for (size_t k = 1; k < order.size(); k++) {
    const int a = order[k - 1], b = order[k];
    if (ent[a].name_len == ent[b].name_len && (!ent[a].name_len || !memcmp(ent[a].name, ent[b].name, ent[a].name_len)) && (dup < 0 || b < dup)) dup = b;
  }
  if (dup >= 0) { *bad = dup; *why = RZ_W_DUPLICATE; return ZADA_E_INVALID; }
  if (kept > RZ_MAX_ENTRIES) { *why = RZ_W_COUNT; return ZADA_E_TOO_LARGE; }
  return ZADA_OK;
}
// An upper bound on the archive: per kept entry both headers with their Zip64 extensions and max (n_in, usize) bytes of payload -- a forced format
// can only lose up to the Store fallback --, the three end records and the comment.
inline uint64_t rz_bound(int count, const zada_rezip_entry *ent, uint64_t comment_len) {
  uint64_t b = 56 + 20 + 22 + comment_len;
  for (int i = 0; i < count; i++) if (!rz_dropped(ent[i])) b += 30 + 20 + 46 + 28 + 2ull * ent[i].name_len + (ent[i].n_in > ent[i].usize ? ent[i].n_in : ent[i].usize);
  return b;
}
// Groups of consecutive entries: their extracted bytes (uz_slot) within `limit`; an entry above ZW_ENTRY_MAX runs alone; dropped entries take no room.
inline void rz_groups(const zada_rezip_entry *ent, int count, uint64_t limit, std::vector<int> &ends) {
  ends.clear();
  uint64_t bytes = 0;
  int g0 = 0;
  auto flush = [&](int g1) { if (g1 > g0) ends.push_back(g1); g0 = g1; bytes = 0; };
  for (int i = 0; i < count; i++) {
    if (rz_dropped(ent[i])) continue;
    if (ent[i].usize > ZW_ENTRY_MAX) { flush(i); flush(i + 1); continue; }
    if (bytes && bytes + uz_slot(ent[i].usize) > limit) flush(i);
    bytes += uz_slot(ent[i].usize);
  }
  flush(count);
}
// The archive as ReZip writes it (rezip_lib.adb:776-800, 1000-1032, 1184-1260; zip-headers.adb:168-276, 336-355).
struct RzDirEnt { uint64_t csize, usize, offset; uint32_t crc, time; uint16_t version, flag, zip_type; const uint8_t *name; uint32_t name_len; };
struct RzArchive { uint64_t base = 0, pos = 0; std::vector<RzDirEnt> dir; };
// The winner's local header appended to blob, the entry added to the directory; returns the header's length.  Kept from the source's local header:
// version needed, time, and the bit flag and 0xFFF5 (no data descriptor, no EOS; rezip_lib.adb:1002-1003), bit 1 set again when the winner ends on a
// marker.  kept_original: the winner is the source's own stream.  For a kept Implode stream (method 6) bits 1 and 2 say how it is read -- an 8 KiB
// dictionary, three trees -- and the mask would drop bit 1, so that the reference's own output no longer decodes: here the two bits of the source
// stay.  A departure from the reference, on purpose.  A Shrink or Reduce winner has no flag bits of its own.
inline uint32_t rz_add(RzArchive &A, const zada_rezip_entry &e, uint64_t csize, uint16_t zip_type, bool eos, std::vector<uint8_t> &blob, bool kept_original = false) {
  const uint32_t implode = kept_original && e.method == 6 ? e.flags & 6u : 0u;
  RzDirEnt d{csize, e.usize, A.base + A.pos, e.crc, e.time, e.version, (uint16_t)((e.flags & 0xFFF5u) | (eos ? 2u : 0u) | implode), zip_type, e.name, e.name_len};
  const bool z64 = zw_needs_zip64(csize, e.usize, d.offset);
  const size_t at = blob.size();
  zw_put(blob, 0x04034B50u, 4); zw_put(blob, d.version, 2); zw_put(blob, d.flag, 2); zw_put(blob, zip_type, 2); zw_put(blob, d.time, 4); zw_put(blob, d.crc, 4);
  zw_put(blob, z64 ? ZW_M32 : csize, 4); zw_put(blob, z64 ? ZW_M32 : e.usize, 4); zw_put(blob, e.name_len, 2); zw_put(blob, z64 ? 20 : 0, 2);
  blob.insert(blob.end(), e.name, e.name + e.name_len);
  if (z64) { zw_put(blob, 1, 2); zw_put(blob, 16, 2); zw_put(blob, e.usize, 8); zw_put(blob, csize, 8); }
  const uint32_t len = (uint32_t)(blob.size() - at);
  A.pos += len + csize;
  A.dir.push_back(d);
  return len;
}
// The central directory, the end records -- the Zip64 ones only when an entry needed the extension -- and the comment.
inline void rz_finish(RzArchive &A, const uint8_t *comment, uint32_t comment_len, std::vector<uint8_t> &out) {
  const size_t at = out.size();
  const uint64_t cd_off = A.base + A.pos, n = A.dir.size();
  uint64_t cd_size = 0;
  bool needs_64 = false;
  for (const RzDirEnt &d : A.dir) {
    const bool z64 = zw_needs_zip64(d.csize, d.usize, d.offset);
    needs_64 = needs_64 || z64;
    zw_put(out, 0x02014B50u, 4); zw_put(out, 20, 2); zw_put(out, d.version, 2); zw_put(out, d.flag, 2); zw_put(out, d.zip_type, 2); zw_put(out, d.time, 4); zw_put(out, d.crc, 4);
    zw_put(out, z64 ? ZW_M32 : d.csize, 4); zw_put(out, z64 ? ZW_M32 : d.usize, 4); zw_put(out, d.name_len, 2); zw_put(out, z64 ? 28 : 0, 2);
    zw_put(out, 0, 2); zw_put(out, 0, 2); zw_put(out, 0, 2); zw_put(out, 0, 4); zw_put(out, z64 ? ZW_M32 : d.offset, 4);
    out.insert(out.end(), d.name, d.name + d.name_len);
    if (z64) { zw_put(out, 1, 2); zw_put(out, 24, 2); zw_put(out, d.usize, 8); zw_put(out, d.csize, 8); zw_put(out, d.offset, 8); }
    cd_size += 46 + (uint64_t)d.name_len + (z64 ? 28 : 0);
  }
  if (needs_64) {
    zw_put(out, 0x06064B50u, 4); zw_put(out, 44, 8); zw_put(out, 0x2D, 2); zw_put(out, 0x2D, 2); zw_put(out, 0, 4); zw_put(out, 0, 4);
    zw_put(out, n, 8); zw_put(out, n, 8); zw_put(out, cd_size, 8); zw_put(out, cd_off, 8);
    zw_put(out, 0x07064B50u, 4); zw_put(out, 0, 4); zw_put(out, cd_off + cd_size, 8); zw_put(out, 1, 4);
    zw_put(out, 0x06054B50u, 4); zw_put(out, 0, 2); zw_put(out, 0, 2); zw_put(out, 0xFFFF, 2); zw_put(out, 0xFFFF, 2); zw_put(out, ZW_M32, 4); zw_put(out, ZW_M32, 4);
  } else {
    zw_put(out, 0x06054B50u, 4); zw_put(out, 0, 2); zw_put(out, 0, 2); zw_put(out, n, 2); zw_put(out, n, 2); zw_put(out, cd_size, 4); zw_put(out, cd_off, 4);
  }
  zw_put(out, comment_len, 2);
  if (comment_len) out.insert(out.end(), comment, comment + comment_len);
  A.pos += out.size() - at;
}

}  // namespace zada
