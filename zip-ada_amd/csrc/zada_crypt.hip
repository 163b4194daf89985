// zada_crypt.hip -- CRC_Crypto.Encode (zip-crc_crypto.adb:90-128) over a device buffer, in place: ZipCrypto as three chained prefix scans.
//
// Update_keys does, per plaintext byte b:
//     key0 := CRC32_step (key0, b)                          affine over GF(2): a prefix CRC of the plaintext
//     key1 := (key1 + (key0 and 16#FF#)) * 134775813 + 1    affine over Z / 2**32 in key1, driven by key0's low byte
//     key2 := CRC32_step (key2, key1 >> 24)                 a prefix CRC again, of the bytes key1 >> 24
// and the byte is xor-ed with Crypto_code (key2 BEFORE the update).  Each line is a first-order recurrence x' = A x + c whose A depends only on
// the number of bytes consumed: for key0 / key2 the "advance over k zero bytes" matrix of the CRC (zero_advance_matrix, zada_api.hip), for key1
// the power 134775813 ** k.  One lane takes one sub-chunk of ZC_SUB = 256 bytes, one wave a tile of 64 sub-chunks.  Four rounds over the buffer,
// each staging its tile in LDS as k_crc_chunks does, with a scan over the tiles' summaries between two rounds:
//     round 0   raw CRC of every sub-chunk (register from 0)                                      -> sub0, tile summaries agg0
//     top       exclusive scan of agg0 over the tiles, seeded with key0                           -> key0 at every tile's start
//     round 1   wave scan of sub0 -> key0 at every sub-chunk's start; replay key0, collect B      -> sub0 (true key0), sub1 = B, agg1
//     top       the same scan in Z / 2**32, seeded with key1
//     round 2   wave scan of sub1 -> true key1; replay key0, key1; raw CRC of key1 >> 24          -> sub1 (true key1), sub2, agg2
//     top       the GF(2) scan again, seeded with key2
//     round 3   wave scan of sub2 -> true key2; replay all three, xor, write; the lane of the last byte leaves the keys
// All sub-chunks but the last are full, so every scan level has ONE operator per distance: the scans are Kogge-Stone with the operators for
// 256 << j bytes, j = 0 .. 15 (ZcOps).  Six table reads per byte in all (1 + 1 + 2 + 2).
// Many small buffers (k_zc_entries): one wave per entry walks the entry in strips of one tile, the four rounds inside the wave, the keys carried
// from strip to strip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"

namespace zada {

constexpr uint32_t ZC_SUB = CRC_SUB, ZC_ROW = ZC_SUB + 16, ZC_WAVE = 64, ZC_TILE = ZC_WAVE * ZC_SUB;
constexpr int ZC_NOPS = 16;                           // operators for 256 << j bytes: j 0..5 inside a wave of sub-chunks, 6..11 a wave of tiles, 12..15 the 16 waves of k_zc_top
constexpr uint32_t ZC_MUL = 134775813u;
constexpr uint64_t ZC_PIECE = 256ull << 20;           // bytes the tiled path takes at a time (the keys stay on the device in between)
constexpr uint32_t ZC_TOP = 1024;

struct ZcOps { uint32_t mat[ZC_NOPS][32]; uint32_t pw[ZC_NOPS]; };

__device__ __forceinline__ uint32_t zc_gf2(const uint32_t *m, uint32_t v) {
  uint32_t s = 0;
#pragma unroll
  for (int b = 0; b < 32; b++) s ^= (0u - ((v >> b) & 1u)) & m[b];
  return s;
}
template <bool Z> __device__ __forceinline__ uint32_t zc_adv(const uint32_t (*m)[32], const uint32_t *pw, int j, uint32_t v) { return Z ? v * pw[j] : zc_gf2(m[j], v); }
template <bool Z> __device__ __forceinline__ uint32_t zc_add(uint32_t a, uint32_t b) { return Z ? a + b : a ^ b; }

// Scan over the lanes of a wave: lane l holds the summary v of unit l ("state behind = A state before + v", A = operator 0 of m / pw; operator j
// covers 2 ** j units).  Returns the state BEFORE unit l when the state before unit 0 is `seed`; *incl = the state behind unit l.
template <bool Z> __device__ __forceinline__ uint32_t zc_wave_scan(uint32_t v, uint32_t seed, const uint32_t (*m)[32], const uint32_t *pw, int steps, uint32_t *incl) {
  const uint32_t lane = threadIdx.x & 63;
  if (lane == 0) v = zc_add<Z>(v, zc_adv<Z>(m, pw, 0, seed));
  for (int j = 0; j < steps; j++) {
    const uint32_t u = __shfl_up(v, 1u << j, 64);
    if (lane >= (1u << j)) v = zc_add<Z>(v, zc_adv<Z>(m, pw, j, u));
  }
  uint32_t e = __shfl_up(v, 1u, 64);
  if (lane == 0) e = seed;
  *incl = v;
  return e;
}

// `left` (<= ZC_TILE) bytes at src into the padded rows, and back.  al16: src is 16-byte aligned (whole 16-byte words inside the buffer only).
__device__ __forceinline__ void zc_stage_in(uint8_t *rows, const uint8_t *src, uint32_t left, bool al16) {
  const uint32_t lane = threadIdx.x;
  if (al16) {
    const uint4 *s = (const uint4 *)src;
    const uint32_t words = left / 16;
#pragma unroll
    for (uint32_t j = 0; j < ZC_SUB / 16; j++) {
      const uint32_t wq = j * ZC_WAVE + lane;
      if (wq < words) *(uint4 *)(rows + (wq >> 4) * ZC_ROW + (wq & 15) * 16) = s[wq];
    }
    if (lane < (left & 15)) { const uint32_t o = words * 16 + lane; rows[(o / ZC_SUB) * ZC_ROW + (o % ZC_SUB)] = src[o]; }
  } else {
    for (uint32_t o = lane; o < left; o += ZC_WAVE) rows[(o / ZC_SUB) * ZC_ROW + (o % ZC_SUB)] = src[o];
  }
}
__device__ __forceinline__ void zc_stage_out(const uint8_t *rows, uint8_t *dst, uint32_t left, bool al16) {
  const uint32_t lane = threadIdx.x;
  if (al16) {
    uint4 *d = (uint4 *)dst;
    const uint32_t words = left / 16;
#pragma unroll
    for (uint32_t j = 0; j < ZC_SUB / 16; j++) {
      const uint32_t wq = j * ZC_WAVE + lane;
      if (wq < words) d[wq] = *(const uint4 *)(rows + (wq >> 4) * ZC_ROW + (wq & 15) * 16);
    }
    if (lane < (left & 15)) { const uint32_t o = words * 16 + lane; dst[o] = rows[(o / ZC_SUB) * ZC_ROW + (o % ZC_SUB)]; }
  } else {
    for (uint32_t o = lane; o < left; o += ZC_WAVE) dst[o] = rows[(o / ZC_SUB) * ZC_ROW + (o % ZC_SUB)];
  }
}

// One lane over the `len` bytes of its row.  ROUND 0: k0 (from 0) = raw CRC.  1: k0 from its true start, k1 (from 0) = B.  2: k0, k1 true, k2 (from 0) = raw
// CRC of the bytes key1 >> 24.  3: all true; every byte is xor-ed with Crypto_code (:102-108) of key2 before its update (:122-126) and written back.
template <int ROUND> __device__ __forceinline__ uint8_t zc_byte(uint32_t b, const uint32_t *tab, uint32_t &k0, uint32_t &k1, uint32_t &k2) {
  uint32_t out = b;
  if (ROUND == 3) { const uint32_t t = (k2 & 0xFFFFu) | 2u; out = b ^ (((t * (t ^ 1u)) >> 8) & 0xFFu); }
  k0 = tab[(k0 ^ b) & 0xFF] ^ (k0 >> 8);                                   // Update_keys :92
  if (ROUND >= 1) k1 = (k1 + (k0 & 0xFFu)) * ZC_MUL + 1u;                   // :93-94
  if (ROUND >= 2) k2 = tab[(k2 ^ (k1 >> 24)) & 0xFF] ^ (k2 >> 8);           // :95-98
  return (uint8_t)out;
}
template <int ROUND> __device__ __forceinline__ void zc_pass(uint8_t *row, uint32_t len, const uint32_t *tab, uint32_t &k0, uint32_t &k1, uint32_t &k2) {
  uint4 *w = (uint4 *)row;
  uint32_t i = 0;
  for (; i + 16 <= len; i += 16) {
    const uint4 v = w[i >> 4];
    uint32_t xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      uint32_t x = xs[q], y = 0;
#pragma unroll
      for (int s = 0; s < 32; s += 8) y |= (uint32_t)zc_byte<ROUND>((x >> s) & 0xFFu, tab, k0, k1, k2) << s;
      xs[q] = y;
    }
    if (ROUND == 3) w[i >> 4] = make_uint4(xs[0], xs[1], xs[2], xs[3]);
  }
  for (; i < len; i++) { const uint8_t o = zc_byte<ROUND>(row[i], tab, k0, k1, k2); if (ROUND == 3) row[i] = o; }
}

__device__ __forceinline__ void zc_load_crc_table(uint32_t *tab) {
  for (uint32_t t = threadIdx.x; t < 256; t += blockDim.x) {
    uint32_t l = t;
    for (int b = 0; b < 8; b++) l = (l & 1) ? (l >> 1) ^ 0xEDB88320u : l >> 1;      // Prepare_table :31-47
    tab[t] = l;
  }
}
// operators first .. first + count - 1 of ops into LDS
__device__ __forceinline__ void zc_load_ops(uint32_t (*m)[32], uint32_t *pw, const ZcOps *ops, int first, int count) {
  for (uint32_t t = threadIdx.x; t < (uint32_t)count * 32; t += blockDim.x) m[t >> 5][t & 31] = ops->mat[first + (t >> 5)][t & 31];
  if (threadIdx.x < (uint32_t)count) pw[threadIdx.x] = ops->pw[first + threadIdx.x];
}

// Round ROUND of the tiled path: one wave per tile of 64 sub-chunks.  sub0 / sub1 / sub2: one word per sub-chunk; agg: one word per tile -- this round's
// summaries out; start: the state at every tile's start that k_zc_top made of the round before's.
template <int ROUND>
__global__ void __launch_bounds__(ZC_WAVE) k_zc_round(uint8_t *__restrict__ buf, uint64_t n, int al16, const ZcOps *__restrict__ ops, uint32_t *__restrict__ sub0,
                                                      uint32_t *__restrict__ sub1, uint32_t *__restrict__ sub2, const uint32_t *__restrict__ start,
                                                      uint32_t *__restrict__ agg, uint32_t *__restrict__ keys) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t m[6][32];
  __shared__ uint32_t pw[6];
  __shared__ __attribute__((aligned(16))) uint8_t rows[ZC_WAVE * ZC_ROW];
  zc_load_crc_table(tab);
  zc_load_ops(m, pw, ops, 0, 6);
  const uint64_t tile0 = (uint64_t)blockIdx.x * ZC_TILE;
  const uint32_t left = n - tile0 < ZC_TILE ? (uint32_t)(n - tile0) : ZC_TILE;           // (the grid has no tile beyond n)
  zc_stage_in(rows, buf + tile0, left, al16 != 0);
  __syncthreads();
  const uint32_t lane = threadIdx.x, off = lane * ZC_SUB;
  const uint32_t len = off >= left ? 0u : left - off < ZC_SUB ? left - off : ZC_SUB;
  const uint64_t k = (uint64_t)blockIdx.x * ZC_WAVE + lane;                              // the lane's sub-chunk (its words exist for every lane of a tile)
  uint8_t *row = rows + lane * ZC_ROW;
  uint32_t k0 = 0, k1 = 0, k2 = 0, incl;
  if (ROUND == 0) {
    zc_pass<0>(row, len, tab, k0, k1, k2);
    sub0[k] = k0;
    zc_wave_scan<false>(k0, 0u, m, pw, 6, &incl);
  } else if (ROUND == 1) {
    k0 = zc_wave_scan<false>(sub0[k], start[blockIdx.x], m, pw, 6, &incl);
    sub0[k] = k0;
    zc_pass<1>(row, len, tab, k0, k1, k2);
    sub1[k] = k1;
    zc_wave_scan<true>(k1, 0u, m, pw, 6, &incl);
  } else if (ROUND == 2) {
    k0 = sub0[k];
    k1 = zc_wave_scan<true>(sub1[k], start[blockIdx.x], m, pw, 6, &incl);
    sub1[k] = k1;
    zc_pass<2>(row, len, tab, k0, k1, k2);
    sub2[k] = k2;
    zc_wave_scan<false>(k2, 0u, m, pw, 6, &incl);
  } else {
    k0 = sub0[k]; k1 = sub1[k];
    k2 = zc_wave_scan<false>(sub2[k], start[blockIdx.x], m, pw, 6, &incl);
    zc_pass<3>(row, len, tab, k0, k1, k2);
    if (tile0 + off < n && tile0 + off + ZC_SUB >= n) { keys[0] = k0; keys[1] = k1; keys[2] = k2; }     // the lane of the last byte
    __syncthreads();
    zc_stage_out(rows, buf + tile0, left, al16 != 0);
  }
  if (ROUND < 3 && lane == ZC_WAVE - 1) agg[blockIdx.x] = incl;                          // (a short last tile's summary is not used)
}

// Exclusive scan of the tiles' summaries, in place, seeded with keys[which]: one workgroup of 16 waves, 1 024 tiles a strip, the state carried from strip to strip.
template <bool Z>
__global__ void __launch_bounds__(ZC_TOP) k_zc_top(uint32_t *__restrict__ agg, uint32_t ntiles, const ZcOps *__restrict__ ops, const uint32_t *__restrict__ keys, int which) {
  __shared__ uint32_t m[10][32];
  __shared__ uint32_t pw[10];
  __shared__ uint32_t wagg[16], wpre[16], carry_s;
  zc_load_ops(m, pw, ops, 6, 10);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t carry = keys[which], incl;
  for (uint32_t base = 0; base < ntiles; base += ZC_TOP) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < ntiles ? agg[i] : 0u;
    zc_wave_scan<Z>(v, 0u, m, pw, 6, &incl);
    if (lane == 63) wagg[w] = incl;
    __syncthreads();
    if (w == 0) {
      const uint32_t e = zc_wave_scan<Z>(lane < 16 ? wagg[lane] : 0u, carry, m + 6, pw + 6, 4, &incl);
      if (lane < 16) wpre[lane] = e;
      if (lane == 15) carry_s = incl;
    }
    __syncthreads();
    const uint32_t e = zc_wave_scan<Z>(v, wpre[w], m, pw, 6, &incl);
    if (i < ntiles) agg[i] = e;
    carry = carry_s;
    __syncthreads();
  }
}

// Many small buffers: one wave per entry of `list`, strip after strip of one tile, the four rounds inside the wave.  Entry e: len[e] bytes at arena + off[e]
// (16-byte aligned), its keys in and out at keys + 3 e.
__global__ void __launch_bounds__(ZC_WAVE) k_zc_entries(uint8_t *__restrict__ arena, const uint64_t *__restrict__ off, const uint64_t *__restrict__ len_of,
                                                        uint32_t *__restrict__ keys, const ZcOps *__restrict__ ops, uint32_t count) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t m[6][32];
  __shared__ uint32_t pw[6];
  __shared__ __attribute__((aligned(16))) uint8_t rows[ZC_WAVE * ZC_ROW];
  const uint32_t e = blockIdx.x;
  if (e >= count) return;
  zc_load_crc_table(tab);
  zc_load_ops(m, pw, ops, 0, 6);
  const uint64_t n = len_of[e];
  uint8_t *buf = arena + off[e];
  uint32_t key0 = keys[3 * e], key1 = keys[3 * e + 1], key2 = keys[3 * e + 2];
  const uint32_t lane = threadIdx.x, o = lane * ZC_SUB;
  uint8_t *row = rows + lane * ZC_ROW;
  for (uint64_t s0 = 0; s0 < n; s0 += ZC_TILE) {
    const uint32_t left = n - s0 < ZC_TILE ? (uint32_t)(n - s0) : ZC_TILE;
    __syncthreads();
    zc_stage_in(rows, buf + s0, left, true);
    __syncthreads();
    const uint32_t len = o >= left ? 0u : left - o < ZC_SUB ? left - o : ZC_SUB;
    uint32_t a = 0, b = 0, c = 0, incl;
    zc_pass<0>(row, len, tab, a, b, c);
    const uint32_t s_0 = zc_wave_scan<false>(a, key0, m, pw, 6, &incl);
    a = s_0; b = 0;
    zc_pass<1>(row, len, tab, a, b, c);
    const uint32_t s_1 = zc_wave_scan<true>(b, key1, m, pw, 6, &incl);
    a = s_0; b = s_1; c = 0;
    zc_pass<2>(row, len, tab, a, b, c);
    const uint32_t s_2 = zc_wave_scan<false>(c, key2, m, pw, 6, &incl);
    a = s_0; b = s_1; c = s_2;
    zc_pass<3>(row, len, tab, a, b, c);
    const int last = (int)((left - 1) / ZC_SUB);                                         // the lane of the strip's last byte
    key0 = __shfl(a, last, 64); key1 = __shfl(b, last, 64); key2 = __shfl(c, last, 64);
    __syncthreads();
    zc_stage_out(rows, buf + s0, left, true);
  }
  if (lane == 0) { keys[3 * e] = key0; keys[3 * e + 1] = key1; keys[3 * e + 2] = key2; }
}

// `left` bytes of the padded rows to dst at any alignment, touching only those bytes: head and tail byte-wise, the 16-byte words of dst in between put
// together from the rows (a word may run from one row into the next).
__device__ __forceinline__ void zc_stage_out_any(const uint8_t *rows, uint8_t *dst, uint32_t left) {
  const uint32_t lane = threadIdx.x;
  auto at = [&](uint32_t o) -> uint32_t { return rows[(o / ZC_SUB) * ZC_ROW + (o % ZC_SUB)]; };
  uint32_t hd = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
  if (hd > left) hd = left;
  if (lane < hd) dst[lane] = (uint8_t)at(lane);
  const uint32_t words = (left - hd) / 16u;
  uint4 *d = (uint4 *)(dst + hd);
  for (uint32_t w = lane; w < words; w += ZC_WAVE) {
    const uint32_t o = hd + 16u * w;
    uint32_t x[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) x[q] = at(o + 4 * q) | at(o + 4 * q + 1) << 8 | at(o + 4 * q + 2) << 16 | at(o + 4 * q + 3) << 24;
    d[w] = make_uint4(x[0], x[1], x[2], x[3]);
  }
  for (uint32_t i = hd + words * 16u + lane; i < left; i += ZC_WAVE) dst[i] = (uint8_t)at(i);
}

// Encode out of place, for the archive writer (zada_zip_device_ex): one wave per job reads the job's bytes -- a stream in the workspace, or a stored
// entry's own bytes, which are never written -- and writes their cipher text to its place in the archive, both at any alignment.  The bytes in front
// of the source's first 16-byte boundary (at most 15) are coded one after the other from the job's keys, by every lane alike; from there on the source
// is staged with aligned 16-byte loads, strip after strip of one tile through the four rounds of k_zc_entries, the keys carried from strip to strip.
__global__ void __launch_bounds__(ZC_WAVE) k_zc_place(const ZcPlaceJob *__restrict__ jobs, const ZcOps *__restrict__ ops, uint32_t count) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t m[6][32];
  __shared__ uint32_t pw[6];
  __shared__ __attribute__((aligned(16))) uint8_t rows[ZC_WAVE * ZC_ROW];
  const uint32_t e = blockIdx.x;
  if (e >= count) return;
  zc_load_crc_table(tab);
  zc_load_ops(m, pw, ops, 0, 6);
  const ZcPlaceJob J = jobs[e];
  const uint8_t *src = (const uint8_t *)J.src;
  uint8_t *dst = (uint8_t *)J.dst;
  uint64_t n = J.len;
  uint32_t key0 = J.keys[0], key1 = J.keys[1], key2 = J.keys[2];
  const uint32_t lane = threadIdx.x, o = lane * ZC_SUB;
  __syncthreads();
  uint32_t h = (16u - (uint32_t)((uintptr_t)src & 15u)) & 15u;
  if (h > n) h = (uint32_t)n;
  for (uint32_t i = 0; i < h; i++) {
    const uint8_t x = zc_byte<3>(src[i], tab, key0, key1, key2);
    if (lane == 0) dst[i] = x;
  }
  src += h; dst += h; n -= h;
  uint8_t *row = rows + lane * ZC_ROW;
  for (uint64_t s0 = 0; s0 < n; s0 += ZC_TILE) {
    const uint32_t left = n - s0 < ZC_TILE ? (uint32_t)(n - s0) : ZC_TILE;
    __syncthreads();
    zc_stage_in(rows, src + s0, left, true);
    __syncthreads();
    const uint32_t len = o >= left ? 0u : left - o < ZC_SUB ? left - o : ZC_SUB;
    uint32_t a = 0, b = 0, c = 0, incl;
    zc_pass<0>(row, len, tab, a, b, c);
    const uint32_t s_0 = zc_wave_scan<false>(a, key0, m, pw, 6, &incl);
    a = s_0; b = 0;
    zc_pass<1>(row, len, tab, a, b, c);
    const uint32_t s_1 = zc_wave_scan<true>(b, key1, m, pw, 6, &incl);
    a = s_0; b = s_1; c = 0;
    zc_pass<2>(row, len, tab, a, b, c);
    const uint32_t s_2 = zc_wave_scan<false>(c, key2, m, pw, 6, &incl);
    a = s_0; b = s_1; c = s_2;
    zc_pass<3>(row, len, tab, a, b, c);
    const int last = (int)((left - 1) / ZC_SUB);                                         // the lane of the strip's last byte
    key0 = __shfl(a, last, 64); key1 = __shfl(b, last, 64); key2 = __shfl(c, last, 64);
    __syncthreads();
    zc_stage_out_any(rows, dst + s0, left);
  }
}

// ---- host side ----
static uint32_t zc_table[256];
static ZcOps zc_ops;
static void zc_host_init() {
  static bool done = [] {
    for (uint32_t t = 0; t < 256; t++) { uint32_t l = t; for (int b = 0; b < 8; b++) l = (l & 1) ? (l >> 1) ^ 0xEDB88320u : l >> 1; zc_table[t] = l; }
    // operator j: the CRC register over 256 << j zero bytes (squaring from the one-byte operator), 134775813 ** (256 << j)
    uint32_t op[32], sq[32];
    for (int i = 0; i < 32; i++) { uint32_t r = 1u << i; r = zc_table[r & 0xFF] ^ (r >> 8); op[i] = r; }
    auto square = [&] { for (int i = 0; i < 32; i++) { uint32_t v = op[i], s = 0; for (int j = 0; v; j++, v >>= 1) if (v & 1) s ^= op[j]; sq[i] = s; } memcpy(op, sq, sizeof op); };
    for (int k = 0; k < 8; k++) square();                                                // 256 bytes
    uint32_t p = ZC_MUL;
    for (int k = 0; k < 8; k++) p *= p;
    for (int j = 0; j < ZC_NOPS; j++) { memcpy(zc_ops.mat[j], op, sizeof op); zc_ops.pw[j] = p; square(); p *= p; }
    return true;
  }();
  (void)done;
}

void crypt_update_keys(uint32_t keys[3], uint8_t by) {                                  // Update_keys :90-99
  zc_host_init();
  keys[0] = zc_table[(keys[0] ^ by) & 0xFF] ^ (keys[0] >> 8);
  keys[1] = (keys[1] + (keys[0] & 0xFFu)) * ZC_MUL + 1u;
  keys[2] = zc_table[(keys[2] ^ (keys[1] >> 24)) & 0xFF] ^ (keys[2] >> 8);
}
uint8_t crypt_code(const uint32_t keys[3]) {                                            // Crypto_code :102-108
  const uint32_t t = (keys[2] & 0xFFFFu) | 2u;
  return (uint8_t)((t * (t ^ 1u)) >> 8);
}

struct ZcState {
  ZcOps *d_ops = nullptr;
  uint32_t *d_keys = nullptr;
  uint32_t *sub[3] = {nullptr, nullptr, nullptr}, *agg[3] = {nullptr, nullptr, nullptr};
  uint64_t cap_bytes = 0;                               // bytes of one piece the sub / agg arrays serve
  uint8_t *io = nullptr; uint64_t cap_io = 0;           // zada_compress_data_pw's input and stream, a batch's arena
  uint64_t *ent = nullptr; uint32_t *ent_keys = nullptr; uint64_t cap_ent = 0;
  ZcPlaceJob *place = nullptr; uint64_t cap_place = 0;  // the jobs of k_zc_place
};
static ZcState *zc_state(Ctx *c) {
  if (c->zc) return (ZcState *)c->zc;
  zc_host_init();
  ZcState *S = new (std::nothrow) ZcState();
  if (!S) return nullptr;
  if (hipMalloc((void **)&S->d_ops, sizeof(ZcOps)) != hipSuccess || hipMalloc((void **)&S->d_keys, 64) != hipSuccess ||
      hipMemcpy(S->d_ops, &zc_ops, sizeof(ZcOps), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (S->d_ops) hipFree(S->d_ops);
    if (S->d_keys) hipFree(S->d_keys);
    delete S;
    return nullptr;
  }
  c->zc = S;
  return S;
}
void crypt_destroy(Ctx *c) {
  ZcState *S = (ZcState *)c->zc;
  if (!S) return;
  for (int i = 0; i < 3; i++) { if (S->sub[i]) hipFree(S->sub[i]); if (S->agg[i]) hipFree(S->agg[i]); }
  if (S->io) hipFree(S->io);
  if (S->ent) hipFree(S->ent);
  if (S->ent_keys) hipFree(S->ent_keys);
  if (S->place) hipFree(S->place);
  hipFree(S->d_ops); hipFree(S->d_keys);
  delete S;
  c->zc = nullptr;
}
static int zc_ensure_scan(Ctx *c, ZcState *S, uint64_t bytes) {
  if (S->cap_bytes >= bytes) return 0;
  hipStreamSynchronize(c->stream);
  for (int i = 0; i < 3; i++) { if (S->sub[i]) hipFree(S->sub[i]); if (S->agg[i]) hipFree(S->agg[i]); S->sub[i] = S->agg[i] = nullptr; }
  S->cap_bytes = 0;
  const uint64_t cap = ((bytes < (1u << 20) ? (1u << 20) : bytes) + ZC_TILE - 1) / ZC_TILE * ZC_TILE, tiles = cap / ZC_TILE;
  for (int i = 0; i < 3; i++)
    if (hipMalloc((void **)&S->sub[i], tiles * ZC_WAVE * 4) != hipSuccess || hipMalloc((void **)&S->agg[i], tiles * 4) != hipSuccess) {
      (void)hipGetLastError(); c->err = "hipMalloc (crypt scan arrays)"; return ZADA_E_NOMEM;
    }
  S->cap_bytes = cap;
  return 0;
}
// a device buffer of the crypt state, at least `bytes` long and 256-byte aligned (zada_compress_data_pw, the arena of a batch)
int crypt_io(Ctx *c, uint64_t bytes, uint8_t **p) {
  ZcState *S = zc_state(c);
  if (!S) { c->err = "crypt: no memory for the tables"; return ZADA_E_NOMEM; }
  if (S->cap_io < bytes || !S->io) {
    hipStreamSynchronize(c->stream); hipStreamSynchronize(c->stream2);
    if (S->io) hipFree(S->io);
    S->io = nullptr; S->cap_io = 0;
    const uint64_t cap = ((bytes < (1u << 20) ? (1u << 20) : bytes) + 65535) & ~65535ull;
    if (hipMalloc((void **)&S->io, cap + 256) != hipSuccess) { (void)hipGetLastError(); c->err = "hipMalloc (crypt buffer)"; return ZADA_E_NOMEM; }
    S->cap_io = cap;
  }
  *p = S->io;
  return 0;
}

// Encode (:118-128) of n bytes at d_buf (any alignment), on the context's stream; the keys are those on the device (S->d_keys)
static int zc_encode_queued(Ctx *c, ZcState *S, uint8_t *d_buf, uint64_t n) {
  int rc = zc_ensure_scan(c, S, n < ZC_PIECE ? n : ZC_PIECE);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int al16 = ((uintptr_t)d_buf & 15) == 0;
  for (uint64_t o = 0; o < n; o += ZC_PIECE) {
    const uint64_t k = n - o < ZC_PIECE ? n - o : ZC_PIECE;
    const uint32_t tiles = (uint32_t)((k + ZC_TILE - 1) / ZC_TILE);
    uint8_t *b = d_buf + o;
    hipLaunchKernelGGL(k_zc_round<0>, dim3(tiles), dim3(ZC_WAVE), 0, st, b, k, al16, S->d_ops, S->sub[0], S->sub[1], S->sub[2], (const uint32_t *)nullptr, S->agg[0], S->d_keys);
    hipLaunchKernelGGL(k_zc_top<false>, dim3(1), dim3(ZC_TOP), 0, st, S->agg[0], tiles, S->d_ops, S->d_keys, 0);
    hipLaunchKernelGGL(k_zc_round<1>, dim3(tiles), dim3(ZC_WAVE), 0, st, b, k, al16, S->d_ops, S->sub[0], S->sub[1], S->sub[2], S->agg[0], S->agg[1], S->d_keys);
    hipLaunchKernelGGL(k_zc_top<true>, dim3(1), dim3(ZC_TOP), 0, st, S->agg[1], tiles, S->d_ops, S->d_keys, 1);
    hipLaunchKernelGGL(k_zc_round<2>, dim3(tiles), dim3(ZC_WAVE), 0, st, b, k, al16, S->d_ops, S->sub[0], S->sub[1], S->sub[2], S->agg[1], S->agg[2], S->d_keys);
    hipLaunchKernelGGL(k_zc_top<false>, dim3(1), dim3(ZC_TOP), 0, st, S->agg[2], tiles, S->d_ops, S->d_keys, 2);
    hipLaunchKernelGGL(k_zc_round<3>, dim3(tiles), dim3(ZC_WAVE), 0, st, b, k, al16, S->d_ops, S->sub[0], S->sub[1], S->sub[2], S->agg[2], (uint32_t *)nullptr, S->d_keys);
  }
  return hip_check(c, hipGetLastError(), "crypt launch");
}

int crypt_encode_device(Ctx *c, uint32_t keys[3], uint8_t *d_buf, uint64_t n) {
  if (n == 0) return 0;
  ZcState *S = zc_state(c);
  if (!S) { c->err = "crypt: no memory for the tables"; return ZADA_E_NOMEM; }
  hipStream_t st = c->stream;
  if (hip_check(c, hipMemcpyAsync(S->d_keys, keys, 12, hipMemcpyHostToDevice, st), "crypt keys in")) return ZADA_E_HIP_;
  int rc = zc_encode_queued(c, S, d_buf, n);
  if (rc) return rc;
  uint32_t k[3];
  if (hip_check(c, hipMemcpyAsync(k, S->d_keys, 12, hipMemcpyDeviceToHost, st), "crypt keys out") || hip_check(c, hipStreamSynchronize(st), "crypt")) return ZADA_E_HIP_;
  memcpy(keys, k, 12);
  return 0;
}

int crypt_encode_place(Ctx *c, uint32_t E, const ZcPlaceJob *jobs) {
  if (E == 0) return 0;
  ZcState *S = zc_state(c);
  if (!S) { c->err = "crypt: no memory for the tables"; return ZADA_E_NOMEM; }
  if (S->cap_place < E) {
    hipStreamSynchronize(c->stream);
    if (S->place) hipFree(S->place);
    S->place = nullptr; S->cap_place = 0;
    const uint64_t cap = (uint64_t)E + E / 4 + 1024;
    if (hipMalloc((void **)&S->place, cap * sizeof(ZcPlaceJob)) != hipSuccess) { (void)hipGetLastError(); c->err = "hipMalloc (crypt place jobs)"; return ZADA_E_NOMEM; }
    S->cap_place = cap;
  }
  if (hip_check(c, hipMemcpy(S->place, jobs, (size_t)E * sizeof(ZcPlaceJob), hipMemcpyHostToDevice), "crypt place jobs")) return ZADA_E_HIP_;
  hipLaunchKernelGGL(k_zc_place, dim3(E), dim3(ZC_WAVE), 0, c->stream, (const ZcPlaceJob *)S->place, (const ZcOps *)S->d_ops, E);
  c->tmark("zip:k_zc_place");
  return hip_check(c, hipGetLastError(), "crypt place launch");
}

// entries idx[0 .. E) of the caller's arrays, each of at most CRYPT_WAVE_MAX bytes, through one launch: packed into an arena, one wave per entry
int crypt_encode_small(Ctx *c, const int *idx, uint32_t E, uint32_t (*keys)[3], uint8_t *const *buf, const uint64_t *n) {
  if (E == 0) return 0;
  ZcState *S = zc_state(c);
  if (!S) { c->err = "crypt: no memory for the tables"; return ZADA_E_NOMEM; }
  std::vector<uint64_t> tabs(2 * (size_t)E);                      // offsets, lengths
  std::vector<uint32_t> hk(3 * (size_t)E);
  uint64_t total = 0;
  for (uint32_t e = 0; e < E; e++) {
    tabs[e] = total; tabs[E + e] = n[idx[e]];
    total += (n[idx[e]] + 15) & ~15ull;
    memcpy(&hk[3 * (size_t)e], keys[idx[e]], 12);
  }
  if (total == 0) return 0;                                       // (empty entries: Encode of nothing leaves the keys)
  uint8_t *arena = nullptr;
  int rc = crypt_io(c, total, &arena);
  if (rc) return rc;
  if (S->cap_ent < E) {
    hipStreamSynchronize(c->stream);
    if (S->ent) hipFree(S->ent);
    if (S->ent_keys) hipFree(S->ent_keys);
    S->ent = nullptr; S->ent_keys = nullptr; S->cap_ent = 0;
    const uint64_t cap = (uint64_t)E + E / 4 + 1024;
    if (hipMalloc((void **)&S->ent, cap * 16) != hipSuccess || hipMalloc((void **)&S->ent_keys, cap * 12) != hipSuccess) {
      (void)hipGetLastError(); c->err = "hipMalloc (crypt entry tables)"; return ZADA_E_NOMEM;
    }
    S->cap_ent = cap;
  }
  std::vector<uint8_t> host(total);
  for (uint32_t e = 0; e < E; e++) if (tabs[E + e]) memcpy(host.data() + tabs[e], buf[idx[e]], tabs[E + e]);
  hipStream_t st = c->stream;
  hipMemcpyAsync(arena, host.data(), total, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(S->ent, tabs.data(), tabs.size() * 8, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(S->ent_keys, hk.data(), hk.size() * 4, hipMemcpyHostToDevice, st);
  hipLaunchKernelGGL(k_zc_entries, dim3(E), dim3(ZC_WAVE), 0, st, arena, S->ent, S->ent + E, S->ent_keys, S->d_ops, E);
  hipMemcpyAsync(host.data(), arena, total, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(hk.data(), S->ent_keys, hk.size() * 4, hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipGetLastError(), "crypt batch") || hip_check(c, hipStreamSynchronize(st), "crypt batch")) return ZADA_E_HIP_;
  for (uint32_t e = 0; e < E; e++) {
    if (tabs[E + e]) memcpy(buf[idx[e]], host.data() + tabs[e], tabs[E + e]);
    memcpy(keys[idx[e]], &hk[3 * (size_t)e], 12);
  }
  return 0;
}

}  // namespace zada
