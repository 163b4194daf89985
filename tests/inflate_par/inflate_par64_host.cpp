// inflate_par64_host.cpp -- the CPU model of the parallel Inflate on Deflate64 streams (zip-ada_amd/csrc/zada_inflate_par.hip with the knob
// "inflate_par_deflate64"): inflate_par_host.cpp's pipeline -- scout (find + count), chain, repairs, symbols, window, finish -- as the format 9
// instantiation of zada_inflate_par_logic.h: d64 = true, 32-bit symbols, a window of 65 536 (InfpFmt <9>), and the one-wave decoder (inf_serial)
// where the pipeline hands the stream over.  tests/_inflate_par64.py builds it into libinflate_par64_host.so and calls it through ctypes;
// tests/inflate_par/par64_check_main.cpp links it under ASan + UBSan.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_inflate_par_logic.h"

using namespace zada;

namespace {

constexpr int FORMAT = 9;
typedef InfpFmt<FORMAT> F;
std::vector<uint64_t> last_live;          // the output bytes of the live chunks of the last stream that ran in parallel, in order

struct HostEnvBase {
  const uint8_t *in; uint64_t n_in;
  void reopen(InfHostReader &br, uint64_t at) { br.open(in, n_in, at); }
};
struct CountEnv : HostEnvBase {
  uint64_t bytes = 0;
  uint32_t stored(uint64_t, uint32_t len) { bytes += len; return INF_OK; }
  uint32_t token(uint32_t len, uint32_t, uint32_t) { bytes += len; return INF_OK; }
};
struct DecodeEnv : HostEnvBase {
  F::sym_t *sym; uint64_t base, limit, pos;
  uint32_t stored(uint64_t at, uint32_t len) {
    if (pos + len > limit) return INF_R_OUTPUT_FULL;
    for (uint32_t i = 0; i < len; i++) sym[pos + i] = in[at + i];
    pos += len;
    return INF_OK;
  }
  uint32_t token(uint32_t len, uint32_t dist, uint32_t val) {
    if (dist > pos) return INF_R_DISTANCE_TOO_FAR;
    if (pos + len > limit) return INF_R_OUTPUT_FULL;
    if (dist == 0) sym[pos] = (F::sym_t)val;
    else for (uint32_t i = 0; i < len; i++) {
      const uint64_t sp = pos - dist + i;
      sym[pos + i] = sp >= base ? sym[sp] : (F::sym_t)infp_marker<FORMAT>(base, sp);
    }
    pos += len;
    return INF_OK;
  }
};

// the 128 bits at a bit offset, zeros behind the input
void bits_at(const uint8_t *in, uint64_t n, uint64_t bit, uint64_t &lo, uint64_t &hi) {
  uint8_t w[17] = {0};
  const uint64_t b = bit >> 3;
  for (int k = 0; k < 17; k++) if (b + k < n) w[k] = in[b + k];
  uint64_t q0 = 0, q1 = 0;
  for (int k = 0; k < 8; k++) { q0 |= (uint64_t)w[k] << (8 * k); q1 |= (uint64_t)w[8 + k] << (8 * k); }
  const uint32_t sh = (uint32_t)(bit & 7u);
  lo = sh ? (q0 >> sh) | (q1 << (64u - sh)) : q0;
  hi = sh ? (q1 >> sh) | ((uint64_t)w[16] << (64u - sh)) : q1;
}

// the scout of one chunk: find (start_bit = INFP_SEARCH) and count
InfpRec scout(const uint8_t *in, uint64_t n_in, uint64_t chunk_bytes, const InfpJob &J, InfTables &T) {
  const uint64_t lo_bit = (uint64_t)J.chunk * chunk_bytes * 8, stop_bits = lo_bit + chunk_bytes * 8, hi_bit = stop_bits < n_in * 8 ? stop_bits : n_in * 8;
  CountEnv env;
  env.in = in; env.n_in = n_in;
  InfHostReader br;
  uint64_t start = J.start_bit;
  bool found = start != INFP_SEARCH;
  for (uint64_t o = lo_bit; o < hi_bit && !found; o++) {
    uint64_t lo, hi;
    {                                                   // (the three header bits first: seven offsets of eight end here)
      const uint64_t b = o >> 3;
      const uint32_t w = (uint32_t)in[b] | (b + 1 < n_in ? (uint32_t)in[b + 1] << 8 : 0u);
      if (((w >> (o & 7u)) & 7u) != 4u) continue;
    }
    bits_at(in, n_in, o, lo, hi);
    if (!infp_filter(lo, hi, F::D64)) continue;
    infp_seek(br, env, o);
    if (infp_candidate(br, T, 0, 1, F::D64)) { start = o; found = true; }
  }
  InfpRec R{found ? start : 0, 0, 0, (found ? (uint32_t)INFP_F_FOUND : 0u) | (J.start_bit != INFP_SEARCH ? (uint32_t)INFP_F_EXACT : 0u), 0};
  if (found) {
    infp_seek(br, env, start);
    uint32_t final = 0;
    R.rule = infp_blocks(br, T, n_in, stop_bits, 0, 1, env, final, F::D64);
    R.end_bit = br.used_bits(); R.bytes = env.bytes;
    if (final) R.flags |= INFP_F_FINAL;
  }
  return R;
}

uint32_t crc_bytes(uint32_t r, const uint8_t *p, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) { r ^= p[i]; for (int b = 0; b < 8; b++) r = (r & 1u) ? (r >> 1) ^ 0xEDB88320u : r >> 1; }
  return r;
}

// 0: done in parallel; 1: handed over (info [6] says why); nothing is written to out in that case
int par_try(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint64_t chunk_bytes, uint32_t repair_pct, InfTables &T, uint64_t *info8,
            uint64_t *out_len, uint64_t *in_used) {
  auto fall = [&](int reason) { info8[5] = 1; info8[6] = (uint64_t)reason; return 1; };
  const uint64_t nch64 = (n_in + chunk_bytes - 1) / chunk_bytes;
  info8[0] = nch64;
  if (nch64 < 2) return fall(INFP_SINGLE_CHUNK);
  const uint32_t nch = (uint32_t)nch64;
  std::vector<InfpRec> recs(nch);
  for (uint32_t k = 0; k < nch; k++) recs[k] = scout(in, n_in, chunk_bytes, InfpJob{k ? INFP_SEARCH : 0ull, k, 0}, T);
  info8[3] = 1;
  std::vector<uint8_t> live(nch, 0);
  std::vector<uint64_t> off(nch, 0);
  InfpWalk W;
  const uint64_t bound = infp_repair_bound(nch, repair_pct);
  for (;;) {
    const int w = infp_walk(W, recs.data(), nch, chunk_bytes * 8, live.data(), off.data());
    info8[1] = W.live; info8[2] = W.repairs;
    if (w == INFP_W_DAMAGED) return fall(INFP_DAMAGED);
    if (w == INFP_W_DONE) break;
    if (W.repairs > bound) return fall(INFP_REPAIRS);
    recs[W.cur] = scout(in, n_in, chunk_bytes, InfpJob{W.expect, W.cur, 0}, T);
    info8[3]++;
  }
  if (W.total > cap) return fall(INFP_DAMAGED);
  if (W.live < 2) return fall(INFP_SINGLE_CHUNK);
  const uint64_t total = W.total;
  F::sym_t *sym = (F::sym_t *)malloc(total ? total * sizeof(F::sym_t) : sizeof(F::sym_t));      // (exact size: a sanitizer sees a symbol too many)
  if (!sym) return fall(INFP_MEMORY);
  // symbols
  for (uint32_t k = 0; k < nch; k++) {
    if (!live[k]) continue;
    DecodeEnv env;
    env.in = in; env.n_in = n_in; env.sym = sym; env.base = env.pos = off[k]; env.limit = off[k] + recs[k].bytes;
    InfHostReader br;
    infp_seek(br, env, recs[k].start_bit);
    uint32_t final = 0;
    uint32_t rule = infp_blocks(br, T, n_in, ((uint64_t)k + 1) * chunk_bytes * 8, 0, 1, env, final, F::D64);
    if (!rule && env.pos != env.limit) rule = INF_R_OUTPUT_FULL;
    if (rule || br.used_bits() != recs[k].end_bit || (final != 0) != ((recs[k].flags & INFP_F_FINAL) != 0)) { free(sym); return fall(INFP_DAMAGED); }
  }
  // window: the live chunks in order, the last 64 Ki symbols of each
  uint64_t marks = 0;
  bool first = true;
  for (uint32_t k = 0; k < nch; k++) {
    if (!live[k]) continue;
    if (first) { first = false; continue; }
    const uint64_t base = off[k], end = base + recs[k].bytes, from = end - base > F::WINDOW ? end - F::WINDOW : base;
    for (uint64_t i = from; i < end; i++) if (sym[i] & F::MARK) { sym[i] = sym[infp_marker_source<FORMAT>(base, sym[i])]; marks++; }
  }
  // finish
  for (uint32_t k = 0; k < nch; k++) {
    if (!live[k]) continue;
    const uint64_t base = off[k], end = base + recs[k].bytes;
    for (uint64_t i = base; i < end; i++) {
      uint32_t v = sym[i];
      if (v & F::MARK) { v = sym[infp_marker_source<FORMAT>(base, v)]; marks++; }
      out[i] = (uint8_t)v;
    }
  }
  free(sym);
  last_live.clear();
  for (uint32_t k = 0; k < nch; k++) if (live[k]) last_live.push_back(recs[k].bytes);
  info8[4] = marks;
  *out_len = total; *in_used = (recs[W.last].end_bit + 7) / 8;
  return 0;
}

}  // namespace

extern "C" {

// zada_inflate_par on host memory, format 9 with the knob set (format 8 is inflate_par_host.cpp's).  Returns 0 or -7 (ZADA_E_DATA); res6 as im_inflate of tests/inflate/inflate_host.cpp: out_len, in_used, rule,
// bit position, CRC-32 register behind the output (from crc_in), 0; info8 = chunks, live chunks, repairs, scout rounds, marker bytes, fell_back,
// reason, streams.
int ipm64_inflate(int format, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint32_t crc_in, uint32_t chunk_kib, uint32_t repair_pct, uint64_t *res6,
                uint64_t *info8) {
  if (format != FORMAT) return -1;
  InfTables *T = (InfTables *)malloc(sizeof(InfTables));
  if (!T) return -2;
  memset(info8, 0, 8 * sizeof(uint64_t));
  info8[7] = 1;
  uint64_t ol = 0, iu = 0;
  const int way = par_try(in, n_in, out, cap, (uint64_t)chunk_kib << 10, repair_pct, *T, info8, &ol, &iu);
  InfResult R;
  if (way == 0) { R.rc = 0; R.rule = 0; R.out_len = ol; R.in_used = iu; R.bitpos = 0; R.crc = 0; R.pad = 0; }
  else inf_serial(format, in, n_in, out, cap, *T, R);
  free(T);
  res6[0] = R.out_len; res6[1] = R.in_used; res6[2] = R.rule; res6[3] = R.bitpos; res6[4] = crc_bytes(crc_in, out, R.out_len); res6[5] = 0;
  return R.rc;
}

// The finder's census of one valid stream at one chunk size: out8 = blocks, dynamic non-final blocks among them, chunks, chunks whose candidate is
// a true block start, chunks whose candidate is none (false positives), chunks that found nothing, 0, 0.  (What the chain makes of it -- the
// repairs -- is ipm64_inflate's to say.)
int ipm64_census(const uint8_t *in, uint64_t n_in, uint32_t chunk_kib, uint64_t *out8) {
  InfTables *T = (InfTables *)malloc(sizeof(InfTables));
  if (!T) return -2;
  memset(out8, 0, 8 * sizeof(uint64_t));
  const uint64_t chunk_bytes = (uint64_t)chunk_kib << 10;
  // every block start, by the exact walk: one block at a time (stop_bits = 0 ends after each)
  std::vector<uint64_t> starts;
  CountEnv env;
  env.in = in; env.n_in = n_in;
  InfHostReader br;
  uint64_t at = 0;
  for (;;) {
    infp_seek(br, env, at);
    br.need32();
    const uint32_t hdr = (uint32_t)br.hold & 7u;
    infp_seek(br, env, at);
    uint32_t final = 0;
    if (infp_blocks(br, *T, n_in, 0, 0, 1, env, final, F::D64)) { free(T); return -7; }
    starts.push_back(at);
    out8[0]++;
    if (hdr == 4u) out8[1]++;
    if (final) break;
    at = br.used_bits();
  }
  const uint64_t nch = (n_in + chunk_bytes - 1) / chunk_bytes;
  out8[2] = nch;
  for (uint64_t k = 1; k < nch; k++) {
    const InfpRec R = scout(in, n_in, chunk_bytes, InfpJob{INFP_SEARCH, (uint32_t)k, 0}, *T);
    if (!(R.flags & INFP_F_FOUND)) { out8[5]++; continue; }
    bool is_true = false;
    for (uint64_t s : starts) if (s == R.start_bit) is_true = true;
    out8[is_true ? 3 : 4]++;
  }
  free(T);
  return 0;
}

const char *ipm64_rule_name(unsigned rule) { return inf_rule_name(rule); }

// the output bytes of the live chunks of the last ipm64_inflate that ran in parallel: the first `max` of them into out; returns how many there are
uint64_t ipm64_last_live(uint64_t *out, uint64_t max) {
  for (uint64_t k = 0; k < last_live.size() && k < max; k++) out[k] = last_live[k];
  return last_live.size();
}

}
