// zada_zip_plan.h -- the host plan of zada_zip_device (zada_zip.hip): argument checks, the groups, every header byte of the archive (Zip.Create's
// Add_Stream and Finish as ZipCreate.add_compressed / finish restate them: zip-create.adb:161-179, 194-297, 645-756; zip-headers.adb:168-210, 244-276,
// 336-355, 494-579) and the table of copy jobs.  Plain C++ without HIP: tests/zip/zip_plan_host.cpp exposes it to the CPU tests (tests/test_zip_plan.py).
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/zada.h"
#include "zada_legacy_plan.h"

namespace zada {

constexpr uint64_t ZW_MAX_BYTES = 1ull << 40;          // an entry of 1 TiB and more is beyond any device
constexpr uint64_t ZW_ENTRY_MAX = 4ull << 20;          // larger entries fill the GPU by themselves (BATCH_ENTRY_MAX, zada_api.hip)
constexpr uint32_t ZW_PIECE = 16384;                   // bytes one wave of k_zw_pack / k_zw_place moves
constexpr uint64_t ZW_STORE_PIECES = 1ull << 22;       // method Store: pieces of 16 KiB one launch of k_uz_store takes (a single entry may have more)
constexpr uint64_t ZW_MARGIN = 22 + 56 + 20 + 65536 + 10;   // Check_Size, zip-create.adb:165-169
constexpr uint64_t ZW_M32 = 0xFFFFFFFFull;

inline bool zw_method_ok(int m) { return m == 0 || (m >= ZADA_DEFLATE_FIXED && m <= ZADA_DEFLATE_R); }
inline const char *zw_method_name(int m) {
  static const char *const names[] = {"Store", "Shrink_1", "Reduce_1", "Reduce_2", "Reduce_3", "Reduce_4", "Deflate_Fixed", "Deflate_0", "Deflate_1", "Deflate_2", "Deflate_3",
                                      "Deflate_R", "BZip2_1", "BZip2_2", "BZip2_3", "LZMA_0", "LZMA_1", "LZMA_2", "LZMA_3", "LZMA_2_for_Zip_in_Zip", "LZMA_3_for_Zip_in_Zip",
                                      "LZMA_2_for_Source", "LZMA_3_for_Source", "LZMA_for_JPEG", "LZMA_for_ARW", "LZMA_for_ORF", "LZMA_for_MP3", "LZMA_for_MP4", "LZMA_for_PGM",
                                      "LZMA_for_PPM", "LZMA_for_PNG", "LZMA_for_GIF", "LZMA_for_WAV", "LZMA_for_AU", "Preselection_1", "Preselection_2"};
  if (m >= 0 && m <= ZADA_PRESELECTION_2) return names[m];
  return "unknown";
}

// what zw_check found wrong with entry *bad
enum ZwWhy { ZW_W_NONE = 0, ZW_W_NULL_DATA, ZW_W_NAME, ZW_W_TOO_LARGE, ZW_W_OVERLAP, ZW_W_CRYPT_SIZE };
inline const char *zw_why_text(int why) {
  switch (why) {
    case ZW_W_NULL_DATA: return "null d_data with n > 0";
    case ZW_W_NAME: return "a name longer than 65 535 bytes (or a null name)";
    case ZW_W_TOO_LARGE: return "an entry of 1 TiB or more";
    case ZW_W_OVERLAP: return "its input overlaps the archive buffer";
    case ZW_W_CRYPT_SIZE: return "an encrypted entry of 4 GiB - 11 .. 4 GiB - 1 bytes (with the 12 header bytes its compressed size has no place in a local header without Zip64 extension)";
    default: return "";
  }
}
// The argument checks, entry after entry in the order of the table.  Returns ZADA_OK, ZADA_E_INVALID or ZADA_E_TOO_LARGE.
inline int zw_check(const zada_zip_entry *ent, int count, uint64_t d_archive, uint64_t cap, int *bad, int *why) {
  *bad = -1; *why = ZW_W_NONE;
  for (int i = 0; i < count; i++) {
    const zada_zip_entry &e = ent[i];
    const uint64_t a = (uint64_t)(uintptr_t)e.d_data;
    int w = ZW_W_NONE;
    if (e.n && !e.d_data) w = ZW_W_NULL_DATA;
    else if (e.name_len > 65535u || (e.name_len && !e.name)) w = ZW_W_NAME;
    else if (e.n >= ZW_MAX_BYTES) w = ZW_W_TOO_LARGE;
    else if (e.n && cap && a < d_archive + cap && d_archive < a + e.n) w = ZW_W_OVERLAP;      // (addresses are below 2 ** 63: no wrap)
    if (w) { *bad = i; *why = w; return w == ZW_W_TOO_LARGE ? ZADA_E_TOO_LARGE : ZADA_E_INVALID; }
  }
  return ZADA_OK;
}

inline bool zw_needs_zip64(uint64_t csize, uint64_t usize, uint64_t offset) { return csize >= ZW_M32 || usize >= ZW_M32 || offset >= ZW_M32; }   // zip-headers.adb:197-210

// An upper bound on the archive's length: every local and central header with the Zip64 extension where the entry's size or the largest offset it can
// have asks for it, n bytes of payload per entry (a payload is never longer: Compress_Data's Store fallback), and all three end records.
inline uint64_t zw_bound(int count, const zada_zip_entry *ent, uint64_t archive_base) {
  uint64_t local = 0, central = 0;
  for (int i = 0; i < count; i++) {
    const bool z64 = zw_needs_zip64(ent[i].n, ent[i].n, archive_base + local);
    local += 30 + (uint64_t)ent[i].name_len + (z64 ? 20 : 0) + ent[i].n;
    central += 46 + (uint64_t)ent[i].name_len + (z64 ? 28 : 0);
  }
  return local + central + 56 + 20 + 22;
}

// ---- the groups: consecutive entries that go through one launch sequence ----
enum { ZW_G_BATCH = 0, ZW_G_SINGLE = 1, ZW_G_STORE = 2 };     // batch_core's launches; the single-stream path; method Store: k_uz_store / k_uz_fold
struct ZwGroup { int g0, g1, kind; };
inline uint64_t zw_slot(uint64_t n) { return ((n ? n : 1) + 32767) & ~32767ull; }               // an entry's share of the LZ buffer: whole 32 KiB segments
inline uint64_t zw_piece_count(uint64_t n) { return (n + ZW_PIECE - 1) / ZW_PIECE; }
// Deflate: entries of up to ZW_ENTRY_MAX are collected as long as their slots stay within `limit` bytes; a larger entry ends the group before it and
// runs alone; a group of one entry takes the single-stream path.  Store: as many entries as have ZW_STORE_PIECES pieces, or one.
inline void zw_groups(const zada_zip_entry *ent, int count, int method, uint64_t limit, std::vector<ZwGroup> &out) {
  out.clear();
  int g0 = 0;
  uint64_t bytes = 0;
  auto flush = [&](int g1) {
    if (g1 > g0) out.push_back(ZwGroup{g0, g1, method == 0 ? ZW_G_STORE : g1 - g0 == 1 ? ZW_G_SINGLE : ZW_G_BATCH});
    g0 = g1; bytes = 0;
  };
  for (int i = 0; i < count; i++) {
    if (method == 0) {
      const uint64_t p = zw_piece_count(ent[i].n) + 1;
      if (bytes + p > ZW_STORE_PIECES) flush(i);
      bytes += p;
    } else if (ent[i].n > ZW_ENTRY_MAX) {
      flush(i); flush(i + 1);
    } else {
      if (bytes + zw_slot(ent[i].n) > limit) flush(i);
      bytes += zw_slot(ent[i].n);
    }
  }
  flush(count);
}

// ---- the archive as it grows: add_compressed and finish ----
struct ZwDirEnt { uint64_t csize, usize, offset; uint32_t crc, time; uint16_t flag, zip_type; const uint8_t *name; uint32_t name_len; };
struct ZwArchive {
  uint64_t base = 0, pos = 0;            // bytes in front of the buffer; bytes laid out so far
  bool zip64 = false;
  std::vector<ZwDirEnt> dir;
};
inline void zw_put(std::vector<uint8_t> &b, uint64_t v, int bytes) { for (int i = 0; i < bytes; i++) b.push_back((uint8_t)(v >> (8 * i))); }
inline void zw_check_size(ZwArchive &A, uint64_t v) { if (!A.zip64 && v >= (1ull << 32) - ZW_MARGIN) A.zip64 = true; }
inline uint32_t zw_local_len(const zada_zip_entry &e, uint64_t offset) { return 30 + e.name_len + (zw_needs_zip64(e.n, e.n, offset) ? 20u : 0u); }
// The entry's local header appended to `blob`, the entry added to the directory; returns the header's length.  The header's form is decided on the
// provisional sizes -- the uncompressed size for both (zip-create.adb:231-241) --, its extension carries the final ones.
// more_flags: LZMA_EOS_Flag_Bit 0x0002 (zip type 14) and Encryption_Flag_Bit 0x0001 (zip-create.adb:221-223, 266-278), as add_compressed sets them.
inline uint32_t zw_add(ZwArchive &A, const zada_zip_entry &e, uint32_t crc, uint64_t csize, uint64_t usize, uint16_t zip_type, std::vector<uint8_t> &blob,
                       uint16_t more_flags = 0) {
  ZwDirEnt d{csize, usize, A.base + A.pos, crc, e.time, (uint16_t)(((e.flags & 1u) ? 0x0800 : 0) | more_flags), zip_type, e.name, e.name_len};
  zw_check_size(A, usize);
  const bool z64 = zw_needs_zip64(usize, usize, d.offset);
  const size_t at = blob.size();
  zw_put(blob, 0x04034B50u, 4); zw_put(blob, 10, 2); zw_put(blob, d.flag, 2); zw_put(blob, zip_type, 2); zw_put(blob, d.time, 4); zw_put(blob, crc, 4);
  zw_put(blob, z64 ? ZW_M32 : csize, 4); zw_put(blob, z64 ? ZW_M32 : usize, 4); zw_put(blob, e.name_len, 2); zw_put(blob, z64 ? 20 : 0, 2);
  if (e.name_len) blob.insert(blob.end(), e.name, e.name + e.name_len);
  if (z64) { zw_put(blob, 1, 2); zw_put(blob, 16, 2); zw_put(blob, usize, 8); zw_put(blob, csize, 8); }
  const uint32_t len = (uint32_t)(blob.size() - at);
  A.pos += len + csize;
  A.dir.push_back(d);
  return len;
}
// The central directory and the end records appended to `out`: what follows the last entry's payload.
inline void zw_finish(ZwArchive &A, std::vector<uint8_t> &out) {
  const size_t at = out.size();
  const uint64_t cd_off = A.base + A.pos, n = A.dir.size();
  if (!A.zip64 && n >= 0xFFFF) A.zip64 = true;
  uint64_t cd_size = 0;
  for (const ZwDirEnt &d : A.dir) {
    const bool z64 = zw_needs_zip64(d.csize, d.usize, d.offset);
    if (z64) A.zip64 = true;
    zw_put(out, 0x02014B50u, 4); zw_put(out, 23, 2); zw_put(out, 10, 2); zw_put(out, d.flag, 2); zw_put(out, d.zip_type, 2); zw_put(out, d.time, 4); zw_put(out, d.crc, 4);
    zw_put(out, z64 ? ZW_M32 : d.csize, 4); zw_put(out, z64 ? ZW_M32 : d.usize, 4); zw_put(out, d.name_len, 2); zw_put(out, z64 ? 28 : 0, 2);
    zw_put(out, 0, 2); zw_put(out, 0, 2); zw_put(out, 0, 2); zw_put(out, 0, 4); zw_put(out, z64 ? ZW_M32 : d.offset, 4);
    if (d.name_len) out.insert(out.end(), d.name, d.name + d.name_len);
    if (z64) { zw_put(out, 1, 2); zw_put(out, 24, 2); zw_put(out, d.usize, 8); zw_put(out, d.csize, 8); zw_put(out, d.offset, 8); }
    cd_size += 46 + (uint64_t)d.name_len + (z64 ? 28 : 0);
  }
  if (n) zw_check_size(A, cd_off + cd_size + 1);
  if (A.zip64) {
    const uint64_t e64_off = cd_off + cd_size;
    zw_put(out, 0x06064B50u, 4); zw_put(out, 44, 8); zw_put(out, 0x2D, 2); zw_put(out, 0x2D, 2); zw_put(out, 0, 4); zw_put(out, 0, 4);
    zw_put(out, n, 8); zw_put(out, n, 8); zw_put(out, cd_size, 8); zw_put(out, cd_off, 8);
    zw_put(out, 0x07064B50u, 4); zw_put(out, 0, 4); zw_put(out, e64_off, 8); zw_put(out, 1, 4);
    zw_put(out, 0x06054B50u, 4); zw_put(out, 0, 2); zw_put(out, 0, 2); zw_put(out, 0xFFFF, 2); zw_put(out, 0xFFFF, 2); zw_put(out, ZW_M32, 4); zw_put(out, ZW_M32, 4); zw_put(out, 0, 2);
  } else {
    zw_put(out, 0x06054B50u, 4); zw_put(out, 0, 2); zw_put(out, 0, 2); zw_put(out, n, 2); zw_put(out, n, 2); zw_put(out, cd_size, 4); zw_put(out, cd_off, 4); zw_put(out, 0, 2);
  }
  A.pos += out.size() - at;
}

// ---- the copy jobs of a group, from its verdicts ----
// A job moves `len` bytes to offset `dst` of the archive buffer from one of three sources: the blob of local headers the host uploads (src: offset in
// it), the group's Deflate streams in the workspace (src: offset in it, ent_base) or the entry's own bytes (src: offset in them, 0) for a stored entry.
enum { ZW_SRC_BLOB = 0, ZW_SRC_STREAM = 1, ZW_SRC_DATA = 2 };
struct ZwJob { uint64_t src, dst, len; uint32_t kind, entry; };
// Entries [g0, g1) with their verdicts -- bytes [k] of Deflate stream at base [k] of the workspace and the running CRC register reg [k], k counted from
// g0; bytes = nullptr: method Store -- are added to the archive: Compress_Data's fallback (zip-compress.adb:224-237: a stream that is not shorter than
// the input is dropped and the entry stored), the local headers into `blob`, the jobs appended to `jobs`, the entries' results into res.
inline void zw_group_place(ZwArchive &A, const zada_zip_entry *ent, int g0, int g1, const uint32_t *bytes, const uint32_t *base, const uint32_t *reg,
                           std::vector<uint8_t> &blob, std::vector<ZwJob> &jobs, zada_zip_result *res) {
  for (int i = g0; i < g1; i++) {
    const zada_zip_entry &e = ent[i];
    const int k = i - g0;
    const bool stored = !bytes || bytes[k] >= e.n;
    const uint64_t csize = stored ? e.n : bytes[k], dst = A.pos, at = blob.size();
    const uint32_t crc = reg[k] ^ 0xFFFFFFFFu;
    const uint16_t zt = stored ? 0 : 8;
    const uint32_t hl = zw_add(A, e, crc, csize, e.n, zt, blob);
    jobs.push_back(ZwJob{at, dst, hl, ZW_SRC_BLOB, (uint32_t)i});
    if (csize) jobs.push_back(ZwJob{stored ? 0 : base[k], dst + hl, csize, stored ? (uint32_t)ZW_SRC_DATA : (uint32_t)ZW_SRC_STREAM, (uint32_t)i});
    if (res) res[i] = zada_zip_result{ZADA_OK, zt, 0, crc, csize, A.base + dst};
  }
}

// One entry that ran alone (a large one, or a group of one): its Deflate stream of stream_len bytes was written straight to its place behind the local
// header -- the job of kind ZW_SRC_STREAM says where it lies, there is nothing to move --, or the entry is stored (`stored`: Compress_Data's fallback).
inline void zw_single_place(ZwArchive &A, const zada_zip_entry *ent, int i, bool stored, uint64_t stream_len, uint32_t reg, std::vector<uint8_t> &blob,
                            std::vector<ZwJob> &jobs, zada_zip_result *res) {
  const zada_zip_entry &e = ent[i];
  const uint64_t csize = stored ? e.n : stream_len, dst = A.pos, at = blob.size();
  const uint32_t crc = reg ^ 0xFFFFFFFFu;
  const uint16_t zt = stored ? 0 : 8;
  const uint32_t hl = zw_add(A, e, crc, csize, e.n, zt, blob);
  jobs.push_back(ZwJob{at, dst, hl, ZW_SRC_BLOB, (uint32_t)i});
  if (csize) jobs.push_back(ZwJob{0, dst + hl, csize, stored ? (uint32_t)ZW_SRC_DATA : (uint32_t)ZW_SRC_STREAM, (uint32_t)i});
  if (res) res[i] = zada_zip_result{ZADA_OK, zt, 0, crc, csize, A.base + dst};
}

// ---- zada_zip_device_ex: every method, a method per entry (Preselection), passwords.  legacy: the knob "zip_legacy" is set, so that Shrink_1 and
//      Reduce_1 .. _4 are taken too ----
inline bool zw_is_legacy(int m) { return m >= ZADA_SHRINK_1 && m <= ZADA_REDUCE_4; }
inline bool zw_method_ok_ex(int m, int legacy = 0) { return m == 0 || (m >= ZADA_DEFLATE_FIXED && m <= ZADA_PRESELECTION_2) || (legacy && zw_is_legacy(m)); }
inline bool zw_is_bzip2(int m) { return m >= ZADA_BZIP2_1 && m <= ZADA_BZIP2_3; }
inline bool zw_is_lzma(int m) { return m >= ZADA_LZMA_0 && m <= ZADA_LZMA_FOR_AU; }
// of a single method (Shrink_1: 1; Reduce_1 .. _4: 2 .. 5)
inline uint16_t zw_zip_type(int m) { return m == 0 ? 0 : zw_is_legacy(m) ? (uint16_t)(m - ZADA_SHRINK_1 + 1) : m <= ZADA_DEFLATE_R ? 8 : zw_is_bzip2(m) ? 12 : 14; }
// the longest entry that is one block whatever it holds (zada_bzip2_batch's rule)
inline uint64_t zw_bz_one_block(int m) { return ((m == ZADA_BZIP2_1 ? 100000ull : m == ZADA_BZIP2_2 ? 400000ull : 900000ull) - 16) * 4 / 5; }
// zw_check for zada_zip_device_ex: with a password an entry of 4 GiB - 11 .. 4 GiB - 1 bytes is refused as well.  The form of its local header is decided
// on the uncompressed size, below 0xFFFFFFFF, so it has no Zip64 extension, and the compressed size with the 12 header bytes -- of the stored entry at
// the least -- does not fit the header's four bytes (ZipCreate.add_compressed cannot pack it either).  The first bad entry in table order is reported.
inline int zw_check_ex(const zada_zip_entry *ent, int count, uint64_t d_archive, uint64_t cap, bool encrypted, int *bad, int *why) {
  const int rc = zw_check(ent, count, d_archive, cap, bad, why);
  const int upto = rc ? *bad : count;
  if (encrypted)
    for (int i = 0; i < upto; i++)
      if (ent[i].n > ZW_M32 - 12 && ent[i].n < ZW_M32) { *bad = i; *why = ZW_W_CRYPT_SIZE; return ZADA_E_INVALID; }
  return rc;
}
// zw_bound with the 12 bytes of an encryption header per entry.  The central extension also looks at the compressed size, which may reach n + 12.
inline uint64_t zw_bound_ex(int count, const zada_zip_entry *ent, uint64_t archive_base, bool encrypted) {
  uint64_t local = 0, central = 0;
  const uint64_t x = encrypted ? 12 : 0;
  for (int i = 0; i < count; i++) {
    const bool z64 = zw_needs_zip64(ent[i].n, ent[i].n, archive_base + local);
    local += 30 + (uint64_t)ent[i].name_len + (z64 ? 20 : 0) + ent[i].n + x;
    central += 46 + (uint64_t)ent[i].name_len + (zw_needs_zip64(ent[i].n + x, ent[i].n, archive_base + local) ? 28 : 0);
  }
  return local + central + 56 + 20 + 22;
}
// The groups when every entry has its method m [i] (a single method: the same for all; never a Preselection method).  Method Store (for all): zw_groups'
// Store groups.  Otherwise an entry above ZW_ENTRY_MAX, or a BZip2 entry longer than one block, ends the group before it and runs alone; the others
// are collected while their slots stay within `limit` bytes, the BZip2 entries' within bz_limit and the HBM literal tables (lit [i] bytes, 0: none)
// within lit_limit; a group of one takes the single-stream path.
inline void zw_groups_ex(const zada_zip_entry *ent, int count, const int *m, const uint64_t *lit, uint64_t limit, uint64_t bz_limit, uint64_t lit_limit,
                         std::vector<ZwGroup> &out) {
  out.clear();
  int g0 = 0;
  uint64_t bytes = 0, bz = 0, lt = 0;
  auto flush = [&](int g1) {
    if (g1 > g0) out.push_back(ZwGroup{g0, g1, g1 - g0 == 1 ? ZW_G_SINGLE : ZW_G_BATCH});
    g0 = g1; bytes = bz = lt = 0;
  };
  for (int i = 0; i < count; i++) {
    const uint64_t slot = zw_slot(ent[i].n), b = zw_is_bzip2(m[i]) ? slot : 0, l = lit ? lit[i] : 0;
    if (ent[i].n > ZW_ENTRY_MAX || (b && ent[i].n > zw_bz_one_block(m[i]))) { flush(i); flush(i + 1); continue; }
    if (bytes + slot > limit || bz + b > bz_limit || lt + l > lit_limit) flush(i);
    bytes += slot; bz += b; lt += l;
  }
  flush(count);
}
// The first entry that Shrink and Reduce do not take (LEGACY_ENTRY_MAX bytes and more), or -1.
inline int zw_legacy_too_large(const zada_zip_entry *ent, int count) {
  for (int i = 0; i < count; i++) if (ent[i].n >= LEGACY_ENTRY_MAX) return i;
  return -1;
}
// The groups of Shrink_1 or Reduce_1 .. _4 (the same method for all), by the rules of zada_shrink_batch / zada_reduce_batch: an entry takes
// 2 * legacy_slot (n) bytes, its slots in the input and in the output arena, and a group's slots stay within `limit` bytes -- at most 1 GiB, so that
// both arenas together stay below 2 ** 32 (LegacyJob's offsets have 32 bits) --; for Reduce the work arrays of a group, reduce_footprint (n) per
// entry, stay within work_limit.  An entry above ZW_ENTRY_MAX ends the group before it and runs alone; a group of one takes the single-stream path.
inline void zw_groups_legacy(const zada_zip_entry *ent, int count, int method, uint64_t limit, uint64_t work_limit, std::vector<ZwGroup> &out) {
  out.clear();
  if (limit > (1ull << 30)) limit = 1ull << 30;
  const bool reduce = method != ZADA_SHRINK_1;
  int g0 = 0;
  uint64_t bytes = 0, work = 0;
  auto flush = [&](int g1) {
    if (g1 > g0) out.push_back(ZwGroup{g0, g1, g1 - g0 == 1 ? ZW_G_SINGLE : ZW_G_BATCH});
    g0 = g1; bytes = work = 0;
  };
  for (int i = 0; i < count; i++) {
    if (ent[i].n > ZW_ENTRY_MAX) { flush(i); flush(i + 1); continue; }
    const uint64_t slot = 2 * legacy_slot(ent[i].n), w = reduce ? reduce_footprint(ent[i].n) : 0;
    if (bytes + slot > limit || work + w > work_limit) flush(i);
    bytes += slot; work += w;
  }
  flush(count);
}
// What the launches of entry i's method left: a stream of `bytes` bytes at device address src (bytes >= n, or zip_type 0: none that counts), the running
// CRC register, the zip type of its method.
struct ZwVerdict { uint64_t src, bytes; uint32_t reg; uint16_t zip_type, pad; };
// zw_group_place for verdicts of any method.  hdr12: null, or 12 bytes per entry (k counted from g0), the encoded encryption header that goes behind
// the local header; the payload's job then starts 12 bytes further on and csize counts them.  A job of kind ZW_SRC_STREAM carries the stream's device
// address in src.
inline void zw_group_place_ex(ZwArchive &A, const zada_zip_entry *ent, int g0, int g1, const ZwVerdict *v, const uint8_t *hdr12, std::vector<uint8_t> &blob,
                              std::vector<ZwJob> &jobs, zada_zip_result *res) {
  for (int i = g0; i < g1; i++) {
    const zada_zip_entry &e = ent[i];
    const ZwVerdict &V = v[i - g0];
    const bool stored = V.zip_type == 0 || V.bytes >= e.n;
    const uint64_t payload = stored ? e.n : V.bytes, csize = payload + (hdr12 ? 12 : 0), dst = A.pos, at = blob.size();
    const uint32_t crc = V.reg ^ 0xFFFFFFFFu;
    const uint16_t zt = stored ? 0 : V.zip_type;
    uint32_t hl = zw_add(A, e, crc, csize, e.n, zt, blob, (uint16_t)((zt == 14 ? 0x0002 : 0) | (hdr12 ? 0x0001 : 0)));
    if (hdr12) { blob.insert(blob.end(), hdr12 + 12 * (size_t)(i - g0), hdr12 + 12 * (size_t)(i - g0) + 12); hl += 12; }
    jobs.push_back(ZwJob{at, dst, hl, ZW_SRC_BLOB, (uint32_t)i});
    if (payload) jobs.push_back(ZwJob{stored ? 0 : V.src, dst + hl, payload, stored ? (uint32_t)ZW_SRC_DATA : (uint32_t)ZW_SRC_STREAM, (uint32_t)i});
    if (res) res[i] = zada_zip_result{ZADA_OK, zt, 0, crc, csize, A.base + dst};
  }
}

// A job cut into the pieces one wave moves: at most ZW_PIECE bytes each.
struct ZwPiece { uint64_t src, dst; uint32_t len, pad; };       // addresses
inline void zw_cut(uint64_t src, uint64_t dst, uint64_t len, std::vector<ZwPiece> &pieces) {
  for (uint64_t o = 0; o < len; o += ZW_PIECE) pieces.push_back(ZwPiece{src + o, dst + o, (uint32_t)(len - o < ZW_PIECE ? len - o : ZW_PIECE), 0});
}

}  // namespace zada
