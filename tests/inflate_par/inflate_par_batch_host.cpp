// inflate_par_batch_host.cpp -- the CPU model of the batched parallel Inflate (zip-ada_amd/csrc/zada_inflate_par.hip with the knob
// "inflate_par_batch"): the plan of zada_inflate_par_batch_plan.h -- passes, sub-passes, chunk numbering, the chain in rounds, the live table,
// the record -- around zada_inflate_par_logic.h with one "lane" and every kernel as a loop over its jobs, its live rows or its streams, for both
// formats (InfpFmt <8>, InfpFmt <9>); the one-wave decoder (inf_serial) for every stream the path does not select or does not take, as
// zada_unzip_device runs its one-wave batch behind the path.  inflate_par_host.cpp and inflate_par64_host.cpp, one stream each, are its reference.
// tests/_inflate_par_batch.py builds it into libinflate_par_batch_host.so; tests/inflate_par/par_batch_check_main.cpp links it under ASan + UBSan.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_inflate_par_batch_plan.h"

using namespace zada;

namespace {

struct HostEnvBase {
  const uint8_t *in; uint64_t n_in;
  void reopen(InfHostReader &br, uint64_t at) { br.open(in, n_in, at); }
};
struct CountEnv : HostEnvBase {
  uint64_t bytes = 0;
  uint32_t stored(uint64_t, uint32_t len) { bytes += len; return INF_OK; }
  uint32_t token(uint32_t len, uint32_t, uint32_t) { bytes += len; return INF_OK; }
};
template <int FORMAT> struct DecodeEnv : HostEnvBase {
  typedef typename InfpFmt<FORMAT>::sym_t sym_t;
  sym_t *sym; uint64_t base, limit, pos;
  uint32_t stored(uint64_t at, uint32_t len) {
    if (pos + len > limit) return INF_R_OUTPUT_FULL;
    for (uint32_t i = 0; i < len; i++) sym[pos + i] = in[at + i];
    pos += len;
    return INF_OK;
  }
  uint32_t token(uint32_t len, uint32_t dist, uint32_t val) {
    if (dist > pos) return INF_R_DISTANCE_TOO_FAR;
    if (pos + len > limit) return INF_R_OUTPUT_FULL;
    if (dist == 0) sym[pos] = (sym_t)val;
    else for (uint32_t i = 0; i < len; i++) {
      const uint64_t sp = pos - dist + i;
      sym[pos + i] = sp >= base ? sym[sp] : (sym_t)infp_marker<FORMAT>(base, sp);
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

// k_infpb_scout's wave: chunk `chunk` of the stream (its own index, its own bit positions); find (start_bit = INFP_SEARCH) and count
InfpRec scout(const uint8_t *in, uint64_t n_in, uint64_t chunk_bytes, uint32_t chunk, uint64_t start_bit, bool d64, InfTables &T) {
  const uint64_t lo_bit = (uint64_t)chunk * chunk_bytes * 8, stop_bits = lo_bit + chunk_bytes * 8, hi_bit = stop_bits < n_in * 8 ? stop_bits : n_in * 8;
  CountEnv env;
  env.in = in; env.n_in = n_in;
  InfHostReader br;
  uint64_t start = start_bit;
  bool found = start != INFP_SEARCH;
  for (uint64_t o = lo_bit; o < hi_bit && !found; o++) {
    uint64_t lo, hi;
    {
      const uint64_t b = o >> 3;
      const uint32_t w = (uint32_t)in[b] | (b + 1 < n_in ? (uint32_t)in[b + 1] << 8 : 0u);
      if (((w >> (o & 7u)) & 7u) != 4u) continue;
    }
    bits_at(in, n_in, o, lo, hi);
    if (!infp_filter(lo, hi, d64)) continue;
    infp_seek(br, env, o);
    if (infp_candidate(br, T, 0, 1, d64)) { start = o; found = true; }
  }
  InfpRec R{found ? start : 0, 0, 0, (found ? (uint32_t)INFP_F_FOUND : 0u) | (start_bit != INFP_SEARCH ? (uint32_t)INFP_F_EXACT : 0u), 0};
  if (found) {
    infp_seek(br, env, start);
    uint32_t final = 0;
    R.rule = infp_blocks(br, T, n_in, stop_bits, 0, 1, env, final, d64);
    R.end_bit = br.used_bits(); R.bytes = env.bytes;
    if (final) R.flags |= INFP_F_FINAL;
  }
  return R;
}

uint32_t crc_bytes(uint32_t r, const uint8_t *p, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) { r ^= p[i]; for (int b = 0; b < 8; b++) r = (r & 1u) ? (r >> 1) ^ 0xEDB88320u : r >> 1; }
  return r;
}

// one sub-pass; launches / marks: added to the record
template <int FORMAT> void sub_pass(const InfpbIn *rows, InfpbRes *res, const std::vector<uint32_t> &idx, uint64_t chunk_bytes, uint32_t pct, InfTables &T, uint64_t &launches,
                                    uint64_t &marks) {
  typedef typename InfpFmt<FORMAT>::sym_t sym_t;
  constexpr bool D64 = InfpFmt<FORMAT>::D64;
  InfpbSub B;
  std::vector<InfpbJob> jobs;
  std::vector<InfpbStream> streams;
  std::vector<InfpbLive> lives;
  if (!infpb_begin(B, rows, idx, FORMAT, chunk_bytes, pct, jobs)) { infpb_results(B, res); return; }
  auto run_scout = [&]() {
    for (const InfpbJob &J : jobs) {
      const InfpbIn &R = rows[B.st[J.stream].row];
      B.recs[J.chunk] = scout((const uint8_t *)(uintptr_t)R.in, R.n_in, chunk_bytes, J.chunk - B.st[J.stream].first, J.start_bit, D64, T);
    }
    B.launches++;
  };
  run_scout();
  for (;;) {
    infpb_round(B, rows, jobs);
    if (jobs.empty()) break;
    run_scout();
  }
  launches += B.launches;
  const uint64_t nsym = infpb_tables(B, rows, streams, lives);
  if (streams.empty()) { infpb_results(B, res); return; }
  sym_t *sym = (sym_t *)malloc(nsym ? nsym * sizeof(sym_t) : sizeof(sym_t));      // (exact size: a sanitizer sees a symbol too many)
  if (!sym) { infpb_drop(B, INFP_MEMORY); infpb_results(B, res); return; }
  // decode: every live row
  for (InfpbLive &J : lives) {
    const InfpbStream &S = streams[J.stream];
    DecodeEnv<FORMAT> env;
    env.in = (const uint8_t *)(uintptr_t)S.in; env.n_in = S.n_in; env.sym = sym + S.sym; env.base = env.pos = J.off; env.limit = J.off + J.bytes;
    InfHostReader br;
    infp_seek(br, env, J.start_bit);
    uint32_t final = 0;
    uint32_t rule = infp_blocks(br, T, S.n_in, J.stop_bits, 0, 1, env, final, D64);
    if (!rule && env.pos != env.limit) rule = INF_R_OUTPUT_FULL;
    J.end_bit = br.used_bits(); J.rule = rule; J.final = final;
  }
  infpb_compare(B, lives, streams);
  // window: every stream that stayed, its live rows in order
  for (const InfpbStream &S : streams) {
    sym_t *ss = sym + S.sym;
    for (uint32_t j = 1; j < S.n_live; j++) {
      const InfpbLive &J = lives[S.first_live + j];
      const uint64_t base = J.off, end = base + J.bytes, from = end - base > InfpFmt<FORMAT>::WINDOW ? end - InfpFmt<FORMAT>::WINDOW : base;
      for (uint64_t i = from; i < end; i++) if (ss[i] & InfpFmt<FORMAT>::MARK) { ss[i] = ss[infp_marker_source<FORMAT>(base, ss[i])]; marks++; }
    }
  }
  // finish: every live row of a stream that stayed
  for (const InfpbLive &J : lives) {
    const InfpbStream &S = streams[J.stream];
    if (!S.n_live) continue;
    const sym_t *ss = sym + S.sym;
    uint8_t *out = (uint8_t *)(uintptr_t)S.out;
    for (uint64_t i = J.off; i < J.off + J.bytes; i++) {
      uint32_t v = ss[i];
      if (v & InfpFmt<FORMAT>::MARK) { v = ss[infp_marker_source<FORMAT>(J.off, v)]; marks++; }
      out[i] = (uint8_t)v;
    }
  }
  free(sym);
  infpb_results(B, res);
}

}  // namespace

extern "C" {

// A group of zada_unzip_device with "inflate_par_batch" = 1 on host memory: n streams (format 8 or 9), the knobs as arguments.  Per stream k:
// rc [k] (0 or -7), res6 [6 k ..] = out_len, in_used, rule, CRC-32 register behind the output (from crc_in [k]), taken (1: finished on the batched
// path), reason (InfpReason; 0 where taken or not selected); info8 = chunks, live chunks, repairs, scout rounds, marker bytes, fell_back, reason,
// streams: the summed record.  pass_ends [0 .. *n_passes): the cut of the selected streams (indices among the selected ones).
int ipb_inflate(uint32_t n, const uint32_t *format, const uint8_t *const *in, const uint64_t *n_in, uint8_t *const *out, const uint64_t *cap, const uint32_t *crc_in,
                uint32_t chunk_kib, uint32_t repair_pct, uint32_t deflate64, uint32_t min_kib, uint32_t batch_mib, int32_t *rc, uint64_t *res6, uint64_t *info8,
                uint32_t *pass_ends, uint32_t *n_passes) {
  InfTables *T = (InfTables *)malloc(sizeof(InfTables));
  if (!T) return -2;
  memset(info8, 0, 8 * sizeof(uint64_t));
  const uint64_t chunk_bytes = (uint64_t)chunk_kib << 10;
  std::vector<InfpbIn> rows;
  std::vector<uint32_t> who;
  for (uint32_t k = 0; k < n; k++) {
    if (format[k] != 8 && format[k] != 9) { free(T); return -1; }
    if (min_kib == 0 || (format[k] == 9 && !deflate64) || n_in[k] < ((uint64_t)min_kib << 10)) continue;
    rows.push_back(InfpbIn{(uint64_t)(uintptr_t)in[k], n_in[k], (uint64_t)(uintptr_t)out[k], cap[k], format[k], crc_in[k]});
    who.push_back(k);
  }
  const uint32_t m = (uint32_t)rows.size();
  std::vector<InfpbRes> res(m);
  for (uint32_t k = 0; k < m; k++) res[k] = InfpbRes{0, 0, infpb_chunks(rows[k].n_in, chunk_bytes), 0, 0, rows[k].crc, 0, INFP_SINGLE_CHUNK, 0};
  std::vector<uint32_t> ends, idx;
  infpb_passes(rows.data(), m, (uint64_t)batch_mib << 20, ends);
  *n_passes = (uint32_t)ends.size();
  for (size_t p = 0; p < ends.size(); p++) pass_ends[p] = ends[p];
  uint32_t p0 = 0;
  for (uint32_t p1 : ends) {
    for (uint32_t f = 8; f <= 9; f++) {
      idx.clear();
      for (uint32_t k = p0; k < p1; k++) if (rows[k].format == f && res[k].chunks >= 2) idx.push_back(k);
      if (idx.empty()) continue;
      if (f == 8) sub_pass<8>(rows.data(), res.data(), idx, chunk_bytes, repair_pct, *T, info8[3], info8[4]);
      else sub_pass<9>(rows.data(), res.data(), idx, chunk_bytes, repair_pct, *T, info8[3], info8[4]);
    }
    p0 = p1;
  }
  uint64_t sum[6];
  infpb_sum(res.data(), m, sum);
  info8[0] = sum[0]; info8[1] = sum[1]; info8[2] = sum[2]; info8[5] = sum[3]; info8[6] = sum[4]; info8[7] = sum[5];
  // the one wave for the rest, and every stream's answer
  std::vector<int> sel(n, -1);
  for (uint32_t k = 0; k < m; k++) sel[who[k]] = (int)k;
  for (uint32_t k = 0; k < n; k++) {
    uint64_t *r = res6 + 6 * (uint64_t)k;
    const int s = sel[k];
    if (s >= 0 && res[s].taken) {
      rc[k] = 0; r[0] = res[s].out_len; r[1] = res[s].in_used; r[2] = 0; r[4] = 1; r[5] = 0;
    } else {
      InfResult R;
      inf_serial((int)format[k], in[k], n_in[k], out[k], cap[k], *T, R);
      rc[k] = R.rc; r[0] = R.out_len; r[1] = R.in_used; r[2] = R.rule; r[4] = 0; r[5] = s >= 0 ? res[s].reason : 0;
    }
    r[3] = crc_bytes(crc_in[k], out[k], r[0]);
  }
  free(T);
  return 0;
}

const char *ipb_rule_name(unsigned rule) { return inf_rule_name(rule); }

}
