// zada_unzip_plan.h -- the host plan of zada_unzip_device (zada_unzip.hip): argument checks, the overlap test, the piece table of the stored entries and
// the grouping of the test-only form.  Plain C++ without HIP: tests/unzip/unzip_plan_host.cpp exposes it to the CPU tests (tests/test_unzip_plan.py).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/zada.h"

namespace zada {

constexpr uint64_t UZ_MAX_BYTES = 1ull << 40;          // (as Inflate: a stream or an output of 1 TiB and more is beyond any device)
constexpr uint32_t UZ_PIECE_MIN = 8, UZ_PIECE_MAX = 14, UZ_PIECE_DEFAULT = 14;   // log2 of the bytes of one piece of a stored entry ("unzip_piece")
constexpr uint64_t UZ_OUT_ALIGN = 256;                 // test-only form: every entry's output at a multiple of this in the context's workspace

// what uz_check found wrong with entry *bad
enum UzWhy { UZ_W_NONE = 0, UZ_W_METHOD, UZ_W_TOO_LARGE, UZ_W_IN_RANGE, UZ_W_OUT_RANGE, UZ_W_NO_KEYS, UZ_W_OVERLAP };
// legacy: the knob "unzip_legacy" is set, so that methods 1 .. 6 (Shrink, Reduce_1 .. _4, Implode) are known too
inline const char *uz_why_text(int why, int legacy = 0) {
  switch (why) {
    case UZ_W_METHOD: return legacy ? "unknown method (0 Store, 1 Shrink, 2 .. 5 Reduce, 6 Implode, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)"
                                    : "unknown method (0 Store, 8 Deflate, 9 Deflate64, 12 BZip2, 14 LZMA)";
    case UZ_W_TOO_LARGE: return "a stream or an output of 1 TiB or more";
    case UZ_W_IN_RANGE: return "its data lie beyond the archive";
    case UZ_W_OUT_RANGE: return "its output range lies beyond the output buffer";
    case UZ_W_NO_KEYS: return "encrypted, and no keys were given";
    case UZ_W_OVERLAP: return "its output range overlaps another entry's";
    default: return "";
  }
}
inline bool uz_method_legacy(uint16_t m) { return m >= 1 && m <= 6; }
inline bool uz_method_known(uint16_t m, int legacy = 0) { return m == 0 || m == 8 || m == 9 || m == 12 || m == 14 || (legacy && uz_method_legacy(m)); }
inline bool uz_encrypted(const zada_unzip_entry &e) { return (e.flags & 1u) != 0; }
// bytes of the entry's data behind the encryption header (an encrypted entry shorter than its header: 0, and ZADA_E_DATA)
inline uint64_t uz_payload(const zada_unzip_entry &e) { return uz_encrypted(e) ? (e.n_in < 12 ? 0 : e.n_in - 12) : e.n_in; }

// The argument checks, entry after entry in the order of the table: method, 1 TiB, input range, output range (have_out), keys; then the overlap of the
// output ranges with cap > 0 (have_out), found by sorting them by their start: the entry whose range begins before the end of an earlier one is *bad.
// Returns ZADA_OK, ZADA_E_INVALID or ZADA_E_TOO_LARGE.  legacy: methods 1 .. 6 are known (the knob "unzip_legacy").
inline int uz_check(const zada_unzip_entry *ent, int count, uint64_t archive_len, uint64_t out_bytes, int have_out, int have_keys, int *bad, int *why,
                    int legacy = 0) {
  *bad = -1; *why = UZ_W_NONE;
  for (int i = 0; i < count; i++) {
    const zada_unzip_entry &e = ent[i];
    int w = UZ_W_NONE;
    if (!uz_method_known(e.method, legacy)) w = UZ_W_METHOD;
    else if (e.n_in >= UZ_MAX_BYTES || e.cap >= UZ_MAX_BYTES) w = UZ_W_TOO_LARGE;
    else if (e.in_off > archive_len || e.n_in > archive_len - e.in_off) w = UZ_W_IN_RANGE;
    else if (have_out && (e.out_off > out_bytes || e.cap > out_bytes - e.out_off)) w = UZ_W_OUT_RANGE;
    else if (uz_encrypted(e) && !have_keys) w = UZ_W_NO_KEYS;
    if (w) { *bad = i; *why = w; return w == UZ_W_TOO_LARGE ? ZADA_E_TOO_LARGE : ZADA_E_INVALID; }
  }
  if (!have_out) return ZADA_OK;
  std::vector<int> order;
  for (int i = 0; i < count; i++) if (ent[i].cap) order.push_back(i);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return ent[a].out_off != ent[b].out_off ? ent[a].out_off < ent[b].out_off : a < b; });
  uint64_t end = 0;
  for (int i : order) {
    if (ent[i].out_off < end) { *bad = i; *why = UZ_W_OVERLAP; return ZADA_E_INVALID; }
    end = ent[i].out_off + ent[i].cap;             // (below 2 ** 41: no wrap)
  }
  return ZADA_OK;
}

// The piece table of the stored entries: entry `id [k]` of `len [k]` bytes is cut into pieces of 1 << plog bytes, the last one shorter; an empty
// entry has none.  first [k] receives the index of the entry's first piece, first [n] the total.
struct UzPiece { uint64_t off; uint32_t entry, len; };
inline uint64_t uz_piece_count(uint64_t len, uint32_t plog) { return (len + ((1ull << plog) - 1)) >> plog; }
inline void uz_pieces(const uint64_t *len, const uint32_t *id, uint32_t n, uint32_t plog, std::vector<UzPiece> &pieces, std::vector<uint64_t> &first) {
  pieces.clear(); first.assign((size_t)n + 1, 0);
  const uint64_t P = 1ull << plog;
  for (uint32_t k = 0; k < n; k++) {
    first[k] = pieces.size();
    for (uint64_t o = 0; o < len[k]; o += P) pieces.push_back(UzPiece{o, id[k], (uint32_t)(len[k] - o < P ? len[k] - o : P)});
  }
  first[n] = pieces.size();
}

// Groups of the test-only form: entries in order, every output at a multiple of UZ_OUT_ALIGN, a group as long as it stays within `limit` bytes -- or
// holds a single entry.  ends receives the index behind every group's last entry.
inline uint64_t uz_slot(uint64_t cap) { return (cap + UZ_OUT_ALIGN - 1) & ~(UZ_OUT_ALIGN - 1); }
inline void uz_groups(const zada_unzip_entry *ent, int count, uint64_t limit, std::vector<int> &ends) {
  ends.clear();
  for (int g0 = 0; g0 < count;) {
    uint64_t bytes = 0;
    int g1 = g0;
    while (g1 < count && (g1 == g0 || bytes + uz_slot(ent[g1].cap) <= limit)) bytes += uz_slot(ent[g1++].cap);
    ends.push_back(g1);
    g0 = g1;
  }
}

}  // namespace zada
