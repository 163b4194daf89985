// zada_reduce.hip -- Reduce_1 .. _4 (Zip formats 2 .. 5): Zip.Compress.Reduce (zip-compress-reduce.adb) behind LZ77_using_LZHuf (lz77.adb:249-429).
//
// One stage is a chain and runs one wave per entry; the rest is parallel inside an entry:
//   k_reduce_lz         the matcher -- a 4 096-byte ring, a binary search tree over the strings that start in it, look-ahead 31 / 63 / 255 / 191 by
//                       factor, threshold 3 -- and Write_normal_byte / Write_DL_code behind it: raw bytes with the escape 144 into HBM.  The tree, the
//                       ring and Reduce's own text ring are in LDS; Insert_Node's comparison runs across the lanes, four bytes per lane.  The reference
//                       runs the matcher twice (statistics, then the stream, the second time until a 256 KiB cache of the first holds the rest); both
//                       passes write the same raw bytes (tests/legacy/reduce_model.c proves it), so the device runs it once.
//   k_reduce_markov     the 256 x 256 counts of (previous raw byte, raw byte), the first previous byte being 0
//   k_reduce_followers  one wave per row: the row's order as a stable rank (the reference's bubble sort swaps on "<" only), the first 32 symbols as
//                       followers, Slen by the smallest expected size in integers (the reference's Long_Float products are exact there)
//   k_reduce_emit       one workgroup per entry: the follower sets for X from 255 down to 0, then 8, 1 + B (Slen) or 9 bits per raw byte, placed by an
//                       exclusive scan of the bit counts tile after tile and ORed into the (cleared) slot, LSB first
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_legacy.h"

namespace zada {

constexpr uint32_t RD_N = 4096, RD_NIL = RD_N, RD_THR = 3, RD_DLE = 144, RD_STAGE = 256;

struct ReduceLds {
  uint16_t lson[RD_N + 1], dad[RD_N + 1], rson[RD_N + 257];
  uint8_t text[RD_N + 256];                              // the matcher's ring and the mirror of its first look-ahead - 1 bytes
  uint8_t ring[RD_N];                                    // Reduce's own text ring (Write_DL_code expands from it)
  uint8_t in[RD_STAGE], raw[RD_STAGE];
};
__device__ __forceinline__ uint32_t rd_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct ReduceRun {
  const uint8_t *src; uint32_t n, pos, in_base;          // the input, staged 256 bytes at a time
  uint8_t *raw; uint32_t raw_cap, raw_len, raw_queued;   // the raw bytes, queued 256 at a time
  uint32_t F, factor, R;                                 // look-ahead, factor, Reduce's ring position
  uint32_t mpos, mlen;
};

__device__ __forceinline__ uint32_t rd_read(ReduceLds &S, ReduceRun &U, int lane) {
  if (U.pos == U.in_base + RD_STAGE || U.pos == 0) {
    U.in_base = U.pos;
    __syncthreads();
    for (uint32_t i = lane; i < RD_STAGE && U.in_base + i < U.n; i += 64) S.in[i] = U.src[U.in_base + i];
    __syncthreads();
  }
  return rd_uniform(S.in[U.pos++ - U.in_base]);
}
__device__ __forceinline__ void rd_raw_flush(ReduceLds &S, ReduceRun &U, int lane) {
  __syncthreads();
  for (uint32_t i = lane; i < U.raw_queued; i += 64)
    if (U.raw_len + i < U.raw_cap) U.raw[U.raw_len + i] = S.raw[i];
  U.raw_len += U.raw_queued; U.raw_queued = 0;
  __syncthreads();
}
__device__ __forceinline__ void rd_raw(ReduceLds &S, ReduceRun &U, uint32_t b, int lane) {
  S.raw[U.raw_queued] = (uint8_t)b;
  if (++U.raw_queued == RD_STAGE) rd_raw_flush(S, U, lane);
}
__device__ __forceinline__ void rd_literal(ReduceLds &S, ReduceRun &U, uint32_t b, int lane) {      // Write_normal_byte
  rd_raw(S, U, b, lane);
  if (b == RD_DLE) rd_raw(S, U, 0, lane);
  S.ring[U.R] = (uint8_t)b; U.R = (U.R + 1) & (RD_N - 1);
}
__device__ __forceinline__ void rd_pair(ReduceLds &S, ReduceRun &U, uint32_t distance, uint32_t length, int lane) {   // Write_DL_code
  const uint32_t start = (U.R - distance) & (RD_N - 1), len = length - 3, dis = distance - 1;
  const uint32_t shift = 1u << (8 - U.factor), max1 = shift - 1;
  if (distance <= (256u << U.factor) && length >= 4 && length <= shift + 257) {
    rd_raw(S, U, RD_DLE, lane);
    const uint32_t upper = (dis >> 8) * shift;
    if (len < max1) rd_raw(S, U, len + upper, lane);
    else { rd_raw(S, U, max1 + upper, lane); rd_raw(S, U, len - max1, lane); }
    rd_raw(S, U, dis & 255, lane);
    for (uint32_t k = 0; k < length; k++) { S.ring[U.R] = S.ring[(start + k) & (RD_N - 1)]; U.R = (U.R + 1) & (RD_N - 1); }
  } else {
    for (uint32_t k = 0; k < length; k++) rd_literal(S, U, rd_uniform(S.ring[(start + k) & (RD_N - 1)]), lane);
  }
}

// Insert_Node: the walk, the tie rule and the replacement of a node matched over the whole look-ahead are the reference's
__device__ void rd_insert(ReduceLds &S, ReduceRun &U, uint32_t r, int lane) {
  const uint32_t F = U.F;
  uint32_t p = RD_N + 1 + rd_uniform(S.text[r]);
  bool geq = true;
  S.rson[r] = RD_NIL; S.lson[r] = RD_NIL;
  U.mlen = 0;
  for (;;) {
    uint16_t *son = geq ? S.rson : S.lson;
    const uint32_t nx = rd_uniform(son[p]);
    if (nx == RD_NIL) { son[p] = (uint16_t)r; S.dad[r] = (uint16_t)p; return; }
    p = nx;
    uint32_t i;
    if (rd_uniform(S.text[r + 1]) != rd_uniform(S.text[p + 1])) i = 1;       // (most walks part at once)
    else {
      // offsets 1 + 4 * lane .. 4 + 4 * lane; an offset from the look-ahead on counts as a difference, so the first difference is min (i, F)
      uint32_t first = 4;
      for (int j = 3; j >= 0; j--) {
        const uint32_t o = 1 + 4 * (uint32_t)lane + (uint32_t)j;
        if (o >= F || S.text[r + (o < F ? o : 0)] != S.text[p + (o < F ? o : 0)]) first = (uint32_t)j;
      }
      const uint64_t m = __ballot(first < 4);
      const int fl = __builtin_ctzll(m);                                       // (m != 0: 1 + 4 * 64 > F)
      i = 1 + 4 * (uint32_t)fl + rd_uniform(__shfl(first, fl));
    }
    geq = i == F || rd_uniform(S.text[r + i]) >= rd_uniform(S.text[p + i]);
    if (i > RD_THR) {
      const uint32_t c = ((r - p) & (RD_N - 1)) - 1;
      if (i > U.mlen) { U.mpos = c; U.mlen = i; if (i >= F) break; }
      else if (i == U.mlen && c < U.mpos) U.mpos = c;
    }
  }
  const uint32_t dp = S.dad[p], lp = S.lson[p], rp = S.rson[p];
  S.dad[r] = (uint16_t)dp; S.lson[r] = (uint16_t)lp; S.rson[r] = (uint16_t)rp;
  S.dad[lp] = (uint16_t)r; S.dad[rp] = (uint16_t)r;
  if (S.rson[dp] == p) S.rson[dp] = (uint16_t)r; else S.lson[dp] = (uint16_t)r;
  S.dad[p] = RD_NIL;
}
__device__ void rd_delete(ReduceLds &S, uint32_t p) {
  uint32_t q;
  const uint32_t dp = rd_uniform(S.dad[p]);
  if (dp == RD_NIL) return;
  const uint32_t lp = rd_uniform(S.lson[p]), rp = rd_uniform(S.rson[p]);
  if (rp == RD_NIL) q = lp;
  else if (lp == RD_NIL) q = rp;
  else {
    q = lp;
    if (rd_uniform(S.rson[q]) != RD_NIL) {
      do q = rd_uniform(S.rson[q]); while (rd_uniform(S.rson[q]) != RD_NIL);
      const uint32_t dq = S.dad[q], lq = S.lson[q];
      S.rson[dq] = (uint16_t)lq; S.dad[lq] = (uint16_t)dq;
      S.lson[q] = (uint16_t)lp; S.dad[lp] = (uint16_t)q;
    }
    S.rson[q] = (uint16_t)rp; S.dad[rp] = (uint16_t)q;
  }
  S.dad[q] = (uint16_t)dp;
  if (S.rson[dp] == p) S.rson[dp] = (uint16_t)q; else S.lson[dp] = (uint16_t)q;
  S.dad[p] = RD_NIL;
}

__global__ void __launch_bounds__(64) k_reduce_lz(uint32_t E, uint32_t factor, const uint8_t *__restrict__ in, const LegacyJob *__restrict__ jobs,
                                                  uint8_t *__restrict__ raw, const uint64_t *__restrict__ raw_start, uint32_t *__restrict__ raw_len) {
  __shared__ ReduceLds S;
  const int lane = threadIdx.x;
  const uint32_t e = blockIdx.x;
  if (e >= E) return;
  const LegacyJob J = jobs[e];
  if (J.n == 0) { if (lane == 0) raw_len[e] = 0; return; }
  const uint32_t F = factor == 1 ? 31 : factor == 2 ? 63 : factor == 3 ? 255 : 191;
  ReduceRun U;
  U.src = in + J.in_off; U.n = J.n; U.pos = 0; U.in_base = 0;
  U.raw = raw + raw_start[e]; U.raw_cap = 2 * J.n + 16; U.raw_len = 0; U.raw_queued = 0;
  U.F = F; U.factor = factor; U.R = RD_N - F; U.mpos = 0; U.mlen = 0;
  for (uint32_t i = RD_N + 1 + lane; i < RD_N + 257; i += 64) S.rson[i] = RD_NIL;      // Init_Tree
  for (uint32_t i = lane; i < RD_N; i += 64) S.dad[i] = RD_NIL;
  for (uint32_t i = lane; i < RD_N + 256; i += 64) S.text[i] = ' ';
  for (uint32_t i = lane; i < RD_N; i += 64) S.ring[i] = 0;
  __syncthreads();
  uint32_t s = 0, r = RD_N - F, len = 0;
  while (len < F && U.pos < U.n) { const uint32_t c = rd_read(S, U, lane); S.text[r + len++] = (uint8_t)c; }
  rd_insert(S, U, r, lane);
  do {
    if (U.mlen > len) U.mlen = len;
    if (U.mlen <= RD_THR) { U.mlen = 1; rd_literal(S, U, rd_uniform(S.text[r]), lane); }
    else rd_pair(S, U, U.mpos + 1, U.mlen, lane);
    const uint32_t last = U.mlen;
    uint32_t i = 0;
    while (i < last && U.pos < U.n) {
      i++;
      rd_delete(S, s);
      const uint32_t c = rd_read(S, U, lane);
      S.text[s] = (uint8_t)c;
      if (s < F - 1) S.text[s + RD_N] = (uint8_t)c;
      s = (s + 1) & (RD_N - 1); r = (r + 1) & (RD_N - 1);
      rd_insert(S, U, r, lane);
    }
    while (i < last) {
      i++;
      rd_delete(S, s);
      s = (s + 1) & (RD_N - 1); r = (r + 1) & (RD_N - 1);
      if (--len > 0) rd_insert(S, U, r, lane);
    }
  } while (len > 0);
  rd_raw_flush(S, U, lane);
  if (lane == 0) raw_len[e] = U.raw_len;
}

// counts [e][previous][byte] over the raw bytes of entry e (cleared by the host)
__global__ void __launch_bounds__(256) k_reduce_markov(uint32_t E, const uint8_t *__restrict__ raw, const uint64_t *__restrict__ raw_start,
                                                       const uint32_t *__restrict__ raw_len, uint32_t *__restrict__ counts) {
  const uint32_t e = blockIdx.x;
  if (e >= E) return;
  const uint8_t *p = raw + raw_start[e];
  const uint32_t n = raw_len[e];
  uint32_t *c = counts + (size_t)e * 65536;
  for (uint32_t i = threadIdx.x; i < n; i += 256) atomicAdd(&c[(i ? p[i - 1] : 0u) * 256u + p[i]], 1u);
}

__device__ __forceinline__ uint32_t rd_b_table(uint32_t slen) { return slen <= 2 ? 1 : slen <= 4 ? 2 : slen <= 8 ? 3 : slen <= 16 ? 4 : 5; }

// one wave per row: Slen, the followers, and fpos [symbol] = its place among the followers in use, 0xFF for none
__global__ void __launch_bounds__(64) k_reduce_followers(uint32_t rows, const uint32_t *__restrict__ counts, uint8_t *__restrict__ slen_out,
                                                         uint8_t *__restrict__ foll, uint8_t *__restrict__ fpos) {
  __shared__ uint32_t cnt[256], sorted[32];
  const int lane = threadIdx.x;
  const uint32_t row = blockIdx.x;
  if (row >= rows) return;
  const uint32_t *c = counts + (size_t)row * 256;
  uint32_t mine[4], sum = 0;
  for (int q = 0; q < 4; q++) { mine[q] = c[lane + 64 * q]; cnt[lane + 64 * q] = mine[q]; sum += mine[q]; }
  if (lane < 32) sorted[lane] = 0;
  for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
  const uint32_t total = rd_uniform(sum);
  __syncthreads();
  uint32_t rank[4];
  for (int q = 0; q < 4; q++) {
    const uint32_t j = (uint32_t)lane + 64u * q;
    uint32_t rk = 0;
    if (total == 0) rk = j;                                                     // an empty row keeps the symbols' own order
    else for (uint32_t i = 0; i < 256; i++) { const uint32_t v = cnt[i]; rk += v > mine[q] || (v == mine[q] && i < j); }
    rank[q] = rk;
    if (rk < 32) { sorted[rk] = mine[q]; foll[(size_t)row * 32 + rk] = (uint8_t)j; }
  }
  __syncthreads();
  // bits_min: the first of 1 .. 5 with the smallest size below total * 8
  uint64_t cum = 0, best = (uint64_t)total * 8;
  uint32_t bits_min = 0;
  for (uint32_t bits = 1, k = 0; bits <= 5; bits++) {
    for (; k < (1u << bits); k++) cum += sorted[k];
    const uint64_t size = cum * (bits + 1) + ((uint64_t)total - cum) * 9 + (uint64_t)(1u << bits) * 8;
    if (size < best) { best = size; bits_min = bits; }
  }
  const uint32_t slen = bits_min ? 1u << bits_min : 0;
  if (lane == 0) slen_out[row] = (uint8_t)slen;
  for (int q = 0; q < 4; q++) fpos[(size_t)row * 256 + lane + 64 * q] = rank[q] < slen ? (uint8_t)rank[q] : 0xFF;
}

// (nothing beyond the slot of cap_words words: a stream that long is not delivered, only counted)
__device__ __forceinline__ void rd_put_bits(uint32_t *words, uint32_t cap_words, uint64_t pos, uint32_t value, uint32_t nbits) {
  if (!nbits) return;
  const uint64_t w = pos >> 5;
  const uint32_t sh = (uint32_t)pos & 31;
  if (w < cap_words) atomicOr(&words[w], value << sh);
  if (sh + nbits > 32 && w + 1 < cap_words) atomicOr(&words[w + 1], value >> (32 - sh));
}
// exclusive scan of v over the 256 threads of the workgroup; *total = the sum
__device__ __forceinline__ uint32_t rd_block_scan(uint32_t v, uint32_t *wsum, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if (lane >= d) incl += t; }
  __syncthreads();
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; w++) before += wsum[w];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return before + incl - v;
}

// the slot of entry e is 4-byte aligned and cleared; jobs [e].cap is a multiple of 4
__global__ void __launch_bounds__(256) k_reduce_emit(uint32_t E, const LegacyJob *__restrict__ jobs, const uint8_t *__restrict__ raw, const uint64_t *__restrict__ raw_start,
                                                     const uint32_t *__restrict__ raw_len, const uint8_t *__restrict__ slen_all, const uint8_t *__restrict__ foll_all,
                                                     const uint8_t *__restrict__ fpos_all, uint8_t *__restrict__ out, uint32_t *__restrict__ bytes) {
  __shared__ uint32_t wsum[4];
  __shared__ uint8_t slen[256];
  const uint32_t e = blockIdx.x, t = threadIdx.x;
  if (e >= E) return;
  const LegacyJob J = jobs[e];
  uint32_t *words = (uint32_t *)(out + J.out_off);
  const uint32_t cap_words = J.cap / 4;
  const uint8_t *foll = foll_all + (size_t)e * 256 * 32, *fpos = fpos_all + (size_t)e * 65536, *p = raw + raw_start[e];
  const uint32_t n = raw_len[e];
  slen[t] = slen_all[(size_t)e * 256 + t];
  __syncthreads();
  // Save_Followers: X from 255 down to 0, 6 bits of Slen and 8 bits per follower
  const uint32_t x = 255 - t, sl = slen[x];
  uint32_t hdr_bits;
  uint64_t pos = rd_block_scan(6 + 8 * sl, wsum, &hdr_bits);
  rd_put_bits(words, cap_words, pos, sl, 6);
  pos += 6;
  for (uint32_t i = 0; i < sl; i++, pos += 8) rd_put_bits(words, cap_words, pos, foll[x * 32 + i], 8);
  uint64_t at = hdr_bits;
  for (uint32_t base = 0; base < n; base += 256) {
    const uint32_t i = base + t;
    uint32_t value = 0, nbits = 0;
    if (i < n) {
      const uint32_t last = i ? p[i - 1] : 0u, b = p[i], s = slen[last];
      if (s == 0) { value = b; nbits = 8; }
      else {
        const uint32_t f = fpos[last * 256 + b];
        if (f != 0xFF) { value = f << 1; nbits = 1 + rd_b_table(s); }
        else { value = b << 1 | 1; nbits = 9; }
      }
    }
    uint32_t tile_bits;
    const uint32_t off = rd_block_scan(nbits, wsum, &tile_bits);
    rd_put_bits(words, cap_words, at + off, value, nbits);
    at += tile_bits;
  }
  if (t == 0) bytes[e] = (uint32_t)((at + 7) >> 3);
}

int reduce_encode_group(Ctx *c, int factor, uint32_t E, const uint8_t *d_in, const LegacyJob *jobs, uint8_t *d_out, uint64_t out_bytes, uint64_t *bytes) {
  if (E == 0) return 0;
  LegacyState *L = legacy_state(c);
  if (!L) return ZADA_E_NOMEM;
  hipStream_t st = c->stream;
  // the work arrays: raw bytes (64-byte slots), then counts, follower positions, followers, Slen
  L->raw_start.resize(E); L->raw_len.assign(E, 0); L->E = 0;
  uint64_t raw_total = 0;
  for (uint32_t e = 0; e < E; e++) { L->raw_start[e] = raw_total; raw_total += (reduce_raw_bound(jobs[e].n) + 63) & ~63ull; }
  const uint64_t o_counts = raw_total, o_fpos = o_counts + (uint64_t)E * 262144, o_foll = o_fpos + (uint64_t)E * 65536, o_slen = o_foll + (uint64_t)E * 8192,
                 work = o_slen + (uint64_t)E * 256;
  const uint64_t t_jobs = 0, t_start = ((uint64_t)E * sizeof(LegacyJob) + 7) & ~7ull, t_len = t_start + 8ull * E, t_bytes = t_len + 4ull * E, tab = t_bytes + 4ull * E;
  int rc = legacy_grow(c, &L->work, &L->cap_work, work, "hipMalloc (Reduce work arrays)");
  if (!rc) rc = legacy_grow(c, &L->tab, &L->cap_tab, tab, "hipMalloc (Reduce tables)");
  if (rc) return rc;
  uint8_t *W = (uint8_t *)L->work, *T = (uint8_t *)L->tab;
  LegacyJob *d_jobs = (LegacyJob *)(T + t_jobs);
  uint64_t *d_start = (uint64_t *)(T + t_start);
  uint32_t *d_len = (uint32_t *)(T + t_len), *d_bytes = (uint32_t *)(T + t_bytes);
  uint32_t *d_counts = (uint32_t *)(W + o_counts);
  uint8_t *d_fpos = W + o_fpos, *d_foll = W + o_foll, *d_slen = W + o_slen;
  hipMemcpyAsync(d_jobs, jobs, (size_t)E * sizeof(LegacyJob), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(d_start, L->raw_start.data(), 8ull * E, hipMemcpyHostToDevice, st);
  hipMemsetAsync(d_counts, 0, (size_t)E * 262144, st);
  hipMemsetAsync(d_out, 0, out_bytes, st);
  c->tmark("reduce:tables");
  hipLaunchKernelGGL(k_reduce_lz, dim3(E), dim3(64), 0, st, E, (uint32_t)factor, d_in, d_jobs, W, d_start, d_len);
  c->tmark("k_reduce_lz");
  hipLaunchKernelGGL(k_reduce_markov, dim3(E), dim3(256), 0, st, E, W, d_start, d_len, d_counts);
  c->tmark("k_reduce_markov");
  hipLaunchKernelGGL(k_reduce_followers, dim3(E * 256), dim3(64), 0, st, E * 256, d_counts, d_slen, d_foll, d_fpos);
  c->tmark("k_reduce_followers");
  hipLaunchKernelGGL(k_reduce_emit, dim3(E), dim3(256), 0, st, E, d_jobs, W, d_start, d_len, d_slen, d_foll, d_fpos, d_out, d_bytes);
  c->tmark("k_reduce_emit");
  std::vector<uint32_t> b(E);
  hipMemcpyAsync(b.data(), d_bytes, 4ull * E, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(L->raw_len.data(), d_len, 4ull * E, hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipStreamSynchronize(st), "Reduce")) return ZADA_E_HIP;
  for (uint32_t e = 0; e < E; e++) bytes[e] = b[e];
  L->E = E; L->d_raw = W; L->d_foll = d_foll; L->d_slen = d_slen;
  return 0;
}

uint64_t reduce_last_record(Ctx *c, int what, uint32_t entry, uint8_t *dst, uint64_t cap) {
  LegacyState *L = (LegacyState *)c->lg;
  if (!L || entry >= L->E) return 0;
  const uint8_t *src = what == 0 ? L->d_raw + L->raw_start[entry] : what == 1 ? L->d_slen + (size_t)entry * 256 : L->d_foll + (size_t)entry * 8192;
  const uint64_t len = what == 0 ? L->raw_len[entry] : what == 1 ? 256 : 8192;
  const uint64_t k = len < cap ? len : cap;
  if (k && dst && hipMemcpy(dst, src, k, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return len;
}

}  // namespace zada
