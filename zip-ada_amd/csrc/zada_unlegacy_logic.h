// zada_unlegacy_logic.h -- the decoders of the three oldest Zip formats: Unshrink (method 1), Unreduce (methods 2 .. 5) and Explode (method 6), as
// UnZip.Decompress states them (unzip-decompress.adb:590-819, :823-964, :973-1418), written once as host+device inline code with no HIP calls.
// The kernels of zada_unlegacy.hip run it with one wave per entry (every decision wave-uniform, the tables in LDS, the window = the entry's own
// output); tests/unlegacy/unlegacy_host.cpp compiles the same text into a CPU model with one "lane", so that every validity rule is tested --
// also under ASan + UBSan -- on a machine without a GPU before a device sees a damaged stream.
//
// What is valid is what the reference accepts, with two departures that hold for all three methods:
//   - a code, a table byte or an extra field that needs a byte beyond n_in is ULG_R_INPUT_END (the reference reads on in whatever its buffer
//     holds and leaves the verdict to the CRC);
//   - a string or a copy that would pass cap is ULG_R_OUTPUT_FULL (the reference's unsigned count of bytes left wraps).
// The stream ends when cap bytes are out; bytes behind that are no error; in_used counts through the byte that held the last bit consumed.
// Nothing is read beyond n_in, nothing is written beyond cap, and a failed entry delivers nothing.
//
// Unshrink keeps the reference's free list in a closed form.  The list is read from its front only and is ascending whenever it is built
// (at the start: 257, 258, ..; in Clear_Leaf_Nodes: every node up to Actual_Max_Code that was free or is a leaf, in index order, then
// Actual_Max_Code + 1, behind which lie the nodes never used with their first links), so it always holds exactly the free nodes in ascending
// order: one "free" bit per node says what Previous_Code (i) < 0 says ("orphan" = that bit), and the next free node is the next set bit.
// tests/unlegacy/unlegacy_model.c keeps the list itself, with the negative Previous_Code, and the tests hold the two equal.
//
// An IO type gives the surroundings: byte () -- the next input byte; beyond the input it gives 0 and counts on --, ip (bytes taken, those
// beyond the input included), n (the input's length), lane () / lanes () / sync () / uni (v) (0 / 1 / nothing / v for one CPU "lane"),
// put (b) -- a literal --, copyz (pos, dist, len) -- a copy whose source reads 0 in front of the entry's first byte --, flush (), and the
// tables of each method (see at the decoders).  Table accessors give what the calling lane reads; the chain makes them uniform with uni ().
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ULG_HD __host__ __device__ __forceinline__
#else
#define ULG_HD inline
#endif

namespace zada {

// the rule a stream broke (zada_last_error names it with the input byte); every one is ZADA_E_DATA
enum UlgRule {
  ULG_OK = 0,
  ULG_R_INPUT_END = 1,       // a code, a table byte or an extra field needs a byte beyond n_in (departure 1)
  ULG_R_OUTPUT_FULL,         // a string or a copy would pass cap (departure 2)
  ULG_R_SHRINK_FIRST,        // "Wrong LZW (Shrink) 1st byte; must be a literal"
  ULG_R_SHRINK_CODE_SIZE,    // "Wrong LZW (Shrink) code size": 256, 1 with 13 bits already
  ULG_R_SHRINK_SPECIAL,      // "Wrong LZW (Shrink) special code": 256, x with x not 1 or 2
  ULG_R_SHRINK_STACK,        // "LZW (Shrink): String stack exhausted": more than 8193 bytes on the stack (this also ends a cycle)
  ULG_R_IMPLODE_RUNS,        // Get_Tree: K + J > N, or K /= N behind the last run
  ULG_R_IMPLODE_TREE,        // HufT_build: the code lengths are over-subscribed or incomplete
  ULG_NRULES
};
ULG_HD const char *ulg_rule_name(uint32_t r) {
  switch (r) {
    case ULG_OK: return "ok";
    case ULG_R_INPUT_END: return "input exhausted before the end of the stream";
    case ULG_R_OUTPUT_FULL: return "output beyond cap";
    case ULG_R_SHRINK_FIRST: return "wrong LZW (Shrink) 1st code; must be a literal";
    case ULG_R_SHRINK_CODE_SIZE: return "wrong LZW (Shrink) code size";
    case ULG_R_SHRINK_SPECIAL: return "wrong LZW (Shrink) special code";
    case ULG_R_SHRINK_STACK: return "LZW (Shrink): string stack exhausted";
    case ULG_R_IMPLODE_RUNS: return "Implode: code length runs do not fill the tree";
    case ULG_R_IMPLODE_TREE: return "Implode: incomplete or over-subscribed tree";
    default: return "?";
  }
}

// what a decoder leaves per entry
struct UlgResult {
  int32_t rc;                 // 0, or ZADA_E_DATA (-7)
  uint32_t rule;              // the UlgRule broken
  uint64_t out_len;           // bytes written (0 unless rc = 0)
  uint64_t in_used;           // bytes through the one that held the last bit consumed (0 unless rc = 0)
  uint64_t in_pos, out_pos;   // where the decoder stood when it ended or gave up (ULG_R_INPUT_END: in_pos = n_in)
  uint32_t crc, pad;          // the CRC-32 register behind the output
};
constexpr int32_t ULG_E_DATA = -7;

ULG_HD void ulg_done(UlgResult &R, uint64_t in_used, uint64_t out_len) {
  R.rc = 0; R.rule = ULG_OK; R.out_len = out_len; R.in_used = in_used; R.in_pos = in_used; R.out_pos = out_len; R.crc = 0; R.pad = 0;
}
ULG_HD void ulg_fail(UlgResult &R, uint32_t rule, uint64_t in_pos, uint64_t out_pos) {
  R.rc = ULG_E_DATA; R.rule = rule; R.out_len = 0; R.in_used = 0; R.in_pos = in_pos; R.out_pos = out_pos; R.crc = 0; R.pad = 0;
}

// ---- Bit_buffer (unzip-decompress.adb:266-329): least significant bit first ----
struct UlgBits { uint32_t b = 0, k = 0; };
template <class IO> ULG_HD uint32_t ulg_peek(IO &io, UlgBits &B, uint32_t n) {          // n <= 16
  while (B.k < n) { B.b |= io.byte() << B.k; B.k += 8; }
  return B.b & ((1u << n) - 1u);
}
ULG_HD void ulg_dump(UlgBits &B, uint32_t n) { B.b >>= n; B.k -= n; }
template <class IO> ULG_HD uint32_t ulg_get(IO &io, UlgBits &B, uint32_t n) {
  const uint32_t v = ulg_peek(io, B, n);
  ulg_dump(B, n);
  return v;
}
// bits consumed lie beyond the input (what was only looked at does not count)
template <class IO> ULG_HD bool ulg_over(const IO &io, const UlgBits &B) { return io.ip * 8 - B.k > io.n * 8; }
template <class IO> ULG_HD uint64_t ulg_used(const IO &io, const UlgBits &B) { return (io.ip * 8 - B.k + 7) / 8; }
template <class IO> ULG_HD void ulg_fail_at(const IO &io, const UlgBits &B, UlgResult &R, uint32_t rule, uint64_t out_pos) {
  ulg_fail(R, rule, rule == ULG_R_INPUT_END ? io.n : ulg_used(io, B), out_pos);
}

// ---- Unshrink ----
// IO: sh_par / sh_set_par (u16 [ULG_SH_NODES]), sh_lit / sh_set_lit (u8 [ULG_SH_NODES]), sh_free / sh_set_free and sh_child / sh_set_child /
// sh_child_or (u32 [ULG_SH_WORDS], one bit per node), sh_stack / sh_set_stack (u8 [ULG_SH_STACK], filled from its end), put_stack (from, len).
constexpr uint32_t ULG_SH_FIRST = 257, ULG_SH_MAX_CODE = 8192;               // Shrink.first_entry, Max_Code
constexpr uint32_t ULG_SH_NODES = ULG_SH_MAX_CODE + 2;                       // (even)
constexpr uint32_t ULG_SH_WORDS = (ULG_SH_MAX_CODE + 32) / 32;               // bits 0 .. 8223; no bit beyond 8192 is ever set
constexpr uint32_t ULG_SH_MAX_PUSH = ULG_SH_MAX_CODE + 1;                    // Stack (0 .. Max_Stack): 8193 bytes, and the string's first byte
constexpr uint32_t ULG_SH_STACK = 8196;

// the first free node at or behind start, 8193 where there is none
template <class IO> ULG_HD uint32_t ulg_sh_next_free(IO &io, uint32_t start) {
  uint32_t w = start >> 5;
  if (w >= ULG_SH_WORDS) return ULG_SH_MAX_CODE + 1;
  uint32_t v = io.uni(io.sh_free(w)) & (~0u << (start & 31u));
  while (!v && ++w < ULG_SH_WORDS) v = io.uni(io.sh_free(w));
  return v ? w * 32u + (uint32_t)__builtin_ctz(v) : ULG_SH_MAX_CODE + 1;
}
// Clear_Leaf_Nodes: every node of 257 .. actual_max that no allocated node names as its parent becomes free (the free ones stay so)
template <class IO> ULG_HD uint32_t ulg_sh_clear(IO &io, uint32_t actual_max) {
  const uint32_t lane = io.lane(), lanes = io.lanes();
  io.sync();
  for (uint32_t w = lane; w < ULG_SH_WORDS; w += lanes) io.sh_set_child(w, 0u);
  io.sync();
  for (uint32_t i = ULG_SH_FIRST + lane; i <= actual_max; i += lanes) {
    if ((io.sh_free(i >> 5) >> (i & 31u)) & 1u) continue;
    const uint32_t p = io.sh_par(i);
    if (p > 256u) io.sh_child_or(p >> 5, 1u << (p & 31u));
  }
  io.sync();
  for (uint32_t w = lane; w < ULG_SH_WORDS; w += lanes) {
    const uint32_t lo = w * 32u, hi = lo + 31u;             // the nodes of this word that lie in 257 .. actual_max
    if (hi < ULG_SH_FIRST || lo > actual_max) continue;
    uint32_t m = ~0u;
    if (lo < ULG_SH_FIRST) m &= ~0u << (ULG_SH_FIRST - lo);
    if (hi > actual_max) m &= ~0u >> (hi - actual_max);
    io.sh_set_free(w, io.sh_free(w) | (~io.sh_child(w) & m));
  }
  io.sync();
  return ulg_sh_next_free(io, ULG_SH_FIRST);
}

template <class IO> ULG_HD void ulg_unshrink(IO &io, uint64_t cap, UlgResult &R) {
  UlgBits B;
  if (cap == 0) { ulg_done(R, 0, 0); return; }             // "compression of a 0-file with Shrink.pas": nothing is read
  {
    const uint32_t lane = io.lane(), lanes = io.lanes();
    for (uint32_t w = lane; w < ULG_SH_WORDS; w += lanes) {
      const uint32_t lo = w * 32u;
      uint32_t m = 0u;
      if (lo + 31u >= ULG_SH_FIRST && lo <= ULG_SH_MAX_CODE) {
        m = ~0u;
        if (lo < ULG_SH_FIRST) m &= ~0u << (ULG_SH_FIRST - lo);
        if (lo + 31u > ULG_SH_MAX_CODE) m &= ~0u >> (lo + 31u - ULG_SH_MAX_CODE);
      }
      io.sh_set_free(w, m);
    }
    io.sync();
  }
  uint32_t next_free = ULG_SH_FIRST, actual_max = ULG_SH_FIRST - 1, size = 9;
  uint32_t code = ulg_get(io, B, size);
  if (ulg_over(io, B)) { ulg_fail_at(io, B, R, ULG_R_INPUT_END, 0); return; }
  if (code > 255u) { ulg_fail_at(io, B, R, ULG_R_SHRINK_FIRST, 0); return; }
  uint32_t last_in = code, last_out = code;
  io.put(code);
  uint64_t pos = 1;
  while (pos < cap) {
    code = ulg_get(io, B, size);
    if (ulg_over(io, B)) { ulg_fail_at(io, B, R, ULG_R_INPUT_END, pos); return; }
    if (code == 256u) {
      const uint32_t x = ulg_get(io, B, size);
      if (ulg_over(io, B)) { ulg_fail_at(io, B, R, ULG_R_INPUT_END, pos); return; }
      if (x == 1u) {
        if (++size > 13u) { ulg_fail_at(io, B, R, ULG_R_SHRINK_CODE_SIZE, pos); return; }
      } else if (x == 2u) next_free = ulg_sh_clear(io, actual_max);
      else { ulg_fail_at(io, B, R, ULG_R_SHRINK_SPECIAL, pos); return; }
      continue;
    }
    const uint32_t new_code = code;
    if (code < 256u) {
      last_out = code;
      io.put(code);
      pos++;
    } else {
      uint32_t pushed = 0;                                  // the stack fills from its end: byte k of it lies at ULG_SH_STACK - 1 - k
      if ((io.uni(io.sh_free(code >> 5)) >> (code & 31u)) & 1u) {       // "Node from stream is orphan"
        io.sh_set_stack(ULG_SH_STACK - 1u - pushed++, last_out);
        code = last_in;
      }
      while (code > 256u) {
        if (pushed >= ULG_SH_MAX_PUSH) { ulg_fail_at(io, B, R, ULG_R_SHRINK_STACK, pos); return; }
        if ((io.uni(io.sh_free(code >> 5)) >> (code & 31u)) & 1u) {     // "Linked node is orphan"
          io.sh_set_stack(ULG_SH_STACK - 1u - pushed++, last_out);
          code = last_in;
        } else {
          io.sh_set_stack(ULG_SH_STACK - 1u - pushed++, io.uni(io.sh_lit(code)));
          code = io.uni(io.sh_par(code));
        }
      }
      last_out = code;
      io.sh_set_stack(ULG_SH_STACK - 1u - pushed++, code);
      if ((uint64_t)pushed > cap - pos) { ulg_fail_at(io, B, R, ULG_R_OUTPUT_FULL, pos); return; }
      io.put_stack(ULG_SH_STACK - pushed, pushed);
      pos += pushed;
    }
    if (next_free <= ULG_SH_MAX_CODE) {                     // Attempt_Table_Increase; a full table adds nothing
      const uint32_t cand = next_free;
      io.sh_set_free(cand >> 5, io.uni(io.sh_free(cand >> 5)) & ~(1u << (cand & 31u)));
      io.sh_set_par(cand, last_in);
      io.sh_set_lit(cand, last_out);
      next_free = ulg_sh_next_free(io, cand + 1u);
      if (next_free - 1u > actual_max) actual_max = next_free - 1u;
    }
    last_in = new_code;
  }
  io.flush();
  ulg_done(R, ulg_used(io, B), pos);
}

// ---- Unreduce ----
// IO: rd_slen / rd_set_slen (u8 [256]), rd_fol / rd_set_fol (u8 [256 * 64]), rd_zero () -- every follower 0, by all lanes.
constexpr uint32_t ULG_RD_DLE = 144;
template <class IO> ULG_HD void ulg_unreduce(IO &io, uint32_t factor, uint64_t cap, UlgResult &R) {
  UlgBits B;
  io.rd_zero();
  for (int32_t x = 255; x >= 0; x--) {                      // LoadFollowers; read even when cap = 0
    const uint32_t s = ulg_get(io, B, 6);
    io.rd_set_slen((uint32_t)x, s);
    for (uint32_t i = 0; i < s; i++) io.rd_set_fol((uint32_t)x * 64u + i, ulg_get(io, B, 8));
    if (ulg_over(io, B)) { ulg_fail_at(io, B, R, ULG_R_INPUT_END, 0); return; }
  }
  const uint32_t mask = (1u << (8u - factor)) - 1u;         // maximum_AND_mask
  uint32_t last = 0, state = 0, V = 0, len = 0;
  uint64_t pos = 0;
  while (pos < cap) {
    const uint32_t sl = io.uni(io.rd_slen(last));
    uint32_t c;
    if (sl == 0u) c = ulg_get(io, B, 8);
    else if (ulg_get(io, B, 1) == 0u) {
      uint32_t nb = 1;                                      // B_Table (sl)
      while ((1u << nb) < sl) nb++;
      c = io.uni(io.rd_fol(last * 64u + ulg_get(io, B, nb)));
    } else c = ulg_get(io, B, 8);
    if (ulg_over(io, B)) { ulg_fail_at(io, B, R, ULG_R_INPUT_END, pos); return; }
    switch (state) {
      case 0:                                               // normal
        if (c == ULG_RD_DLE) state = 1;
        else { io.put(c); pos++; }
        break;
      case 1:                                               // length_a
        if (c == 0u) { io.put(ULG_RD_DLE); pos++; state = 0; }
        else { V = c; len = V & mask; state = len == mask ? 2u : 3u; }
        break;
      case 2:                                               // length_b
        len += c; state = 3;
        break;
      default: {                                            // distance
        len += 3u;
        if ((uint64_t)len > cap - pos) { ulg_fail_at(io, B, R, ULG_R_OUTPUT_FULL, pos); return; }
        io.copyz(pos, (uint64_t)c + 1u + (uint64_t)((V >> (8u - factor)) << 8), len);
        pos += len; state = 0;
      }
    }
    last = c;
  }
  io.flush();
  ulg_done(R, ulg_used(io, B), pos);
}

// ---- Explode ----
// A tree t (0: literals, 1: lengths, 2: distances) is its canonical form: ex_cnt (t, l) codes of l bits, l = 1 .. 16, and ex_sym (t, i) the symbols
// in the order of (length, symbol).  HufT_build gives the codes out in that order, shortest first, and Read_inverted reads them with every bit
// inverted; a complete tree has no other entries, so the tables' width (Bb, Bl, Bd) changes no result.
// IO: ex_cnt / ex_set_cnt (u16 [3 * 17]), ex_sym / ex_set_sym (u8 [3 * 256]), ex_len / ex_set_len (u8 [256]) and ex_off / ex_set_off
// (u16 [17]): the lengths and the offsets while a tree is built.
constexpr uint32_t ULG_EX_LIT = 0, ULG_EX_LEN = 1, ULG_EX_DIST = 2;
// Get_Tree + HufT_build; the tree lies behind the input's bytes taken so far (no bits are pending)
template <class IO> ULG_HD uint32_t ulg_ex_tree(IO &io, uint32_t t, uint32_t N) {
  uint32_t I = io.byte() + 1u, K = 0;
  if (io.ip > io.n) return ULG_R_INPUT_END;
  for (; I; I--) {
    uint32_t J = io.byte();
    if (io.ip > io.n) return ULG_R_INPUT_END;
    const uint32_t Bl = (J & 15u) + 1u;
    J = (J >> 4) + 1u;
    if (K + J > N) return ULG_R_IMPLODE_RUNS;
    for (; J; J--) io.ex_set_len(K++, Bl);
  }
  if (K != N) return ULG_R_IMPLODE_RUNS;
  for (uint32_t l = 0; l <= 16u; l++) io.ex_set_cnt(t * 17u + l, 0u);
  for (uint32_t s = 0; s < N; s++) { const uint32_t l = io.uni(io.ex_len(s)); io.ex_set_cnt(t * 17u + l, io.uni(io.ex_cnt(t * 17u + l)) + 1u); }
  int32_t y = 1;
  for (uint32_t l = 1; l <= 16u; l++) {
    y = y * 2 - (int32_t)io.uni(io.ex_cnt(t * 17u + l));
    if (y < 0) return ULG_R_IMPLODE_TREE;
  }
  if (y != 0) return ULG_R_IMPLODE_TREE;
  uint32_t at = 0;                                          // "Make table of values in order of bit length"
  for (uint32_t l = 1; l <= 16u; l++) { io.ex_set_off(l, at); at += io.uni(io.ex_cnt(t * 17u + l)); }
  for (uint32_t s = 0; s < N; s++) {
    const uint32_t l = io.uni(io.ex_len(s)), o = io.uni(io.ex_off(l));
    io.ex_set_sym(t * 256u + o, s);
    io.ex_set_off(l, o + 1u);
  }
  return ULG_OK;
}
// one symbol of tree t; the bits looked at beyond the code are not consumed
template <class IO> ULG_HD uint32_t ulg_ex_sym(IO &io, UlgBits &B, uint32_t t) {
  const uint32_t r = ~ulg_peek(io, B, 16);
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l <= 16u; l++) {
    code |= (r >> (l - 1u)) & 1u;
    const uint32_t c = io.uni(io.ex_cnt(t * 17u + l));
    if (code - first < c) { ulg_dump(B, l); return io.uni(io.ex_sym(t * 256u + index + (code - first))); }
    index += c; first = (first + c) << 1; code <<= 1;
  }
  ulg_dump(B, 16);                                          // (not reached: the tree is complete)
  return 0;
}
// flags: the entry's general-purpose bits -- 2: 8 KiB dictionary (7 low distance bits), 4: three trees (literals coded, minimum match 3)
template <class IO> ULG_HD void ulg_explode(IO &io, uint32_t flags, uint64_t cap, UlgResult &R) {
  UlgBits B;
  const bool lit_tree = (flags & 4u) != 0;
  const uint32_t low = (flags & 2u) ? 7u : 6u, min_match = lit_tree ? 3u : 2u;
  uint32_t rule = ULG_OK;
  if (lit_tree) rule = ulg_ex_tree(io, ULG_EX_LIT, 256);
  if (!rule) rule = ulg_ex_tree(io, ULG_EX_LEN, 64);
  if (!rule) rule = ulg_ex_tree(io, ULG_EX_DIST, 64);
  if (rule) { ulg_fail_at(io, B, R, rule, 0); return; }
  io.sync();
  uint64_t pos = 0;
  while (pos < cap) {
    if (ulg_get(io, B, 1)) {
      const uint32_t c = lit_tree ? ulg_ex_sym(io, B, ULG_EX_LIT) : ulg_get(io, B, 8);
      if (ulg_over(io, B)) { ulg_fail_at(io, B, R, ULG_R_INPUT_END, pos); return; }
      io.put(c);
      pos++;
    } else {
      uint32_t d = ulg_get(io, B, low);
      d += (ulg_ex_sym(io, B, ULG_EX_DIST) << low) + 1u;
      const uint32_t ls = ulg_ex_sym(io, B, ULG_EX_LEN);
      uint32_t n = min_match + ls;
      if (ls == 63u) n += ulg_get(io, B, 8);
      if (ulg_over(io, B)) { ulg_fail_at(io, B, R, ULG_R_INPUT_END, pos); return; }
      if ((uint64_t)n > cap - pos) { ulg_fail_at(io, B, R, ULG_R_OUTPUT_FULL, pos); return; }
      io.copyz(pos, d, n);
      pos += n;
    }
  }
  io.flush();
  ulg_done(R, ulg_used(io, B), pos);
}

// method: 1 Shrink, 2 .. 5 Reduce with factor 1 .. 4, 6 Implode
template <class IO> ULG_HD void ulg_decode(IO &io, uint32_t method, uint32_t flags, uint64_t cap, UlgResult &R) {
  if (method == 1u) ulg_unshrink(io, cap, R);
  else if (method == 6u) ulg_explode(io, flags, cap, R);
  else ulg_unreduce(io, method - 1u, cap, R);
}

}  // namespace zada
