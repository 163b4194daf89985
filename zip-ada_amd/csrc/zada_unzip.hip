// zada_unzip.hip -- zada_unzip_device: the entries of an archive that lies in device memory, extracted into device memory.
//
// The host side is a plan (zada_unzip_plan.h: argument checks, overlap test, piece table, groups) and a sequence of launches over a table of the
// entries; no entry byte crosses the host.  Deflate, Deflate64, BZip2 and LZMA entries go through the runners of their readers (inflate_run_jobs,
// bunzip2_run_jobs, unlzma_run_jobs: zada_internal.h), their jobs pointing into the archive and into the output.  What is new here:
// k_uz_decode: CRC_Crypto.Decode (zip-crc_crypto.adb:130-137) out of place, one LANE per entry as k_crypt_decode -- the key chain is serial per entry --
//   but sixteen bytes a step: the head runs byte-wise up to the source's 16-byte boundary, then one 16-byte load feeds sixteen key steps and one 16-byte
//   store.  The scratch is laid out so that source and destination agree modulo 16.  The lane checks the header's last byte itself and stops the entry
//   on a mismatch; an encrypted stored entry is decoded straight into its output range.
// k_uz_gather: the nine header bytes of every LZMA payload (behind the decryption) into one table the host fetches with one copy: what sizes the literal
//   tables in HBM (unlzma_hbm_elems).  The Inflate and BZip2 runners read nothing of a stream on the host (bzd_run's k_bzd_scan gathers the stream headers).
// k_uz_store / k_uz_fold: a stored entry copied and summed in one pass, parallel INSIDE the entry: one wave per piece of 16 KiB stages the piece through
//   LDS at the source's alignment, stores it at the destination's and leaves the piece's raw CRC-32 register (started from 0: the register is affine in
//   its start value); one wave per entry then folds the pieces' registers with the operators "advance over piece << j zero bytes" as a scan across
//   lanes, from the entry's running register.  An entry of one piece is finished by its piece's wave.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <new>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_unzip_plan.h"
#include "zada_inflate_par_batch_plan.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {

constexpr uint32_t UZ_WAVE = 64;
constexpr uint32_t UZ_SUB = 256, UZ_ROW = UZ_SUB + 16, UZ_ROWS = (1u << UZ_PIECE_MAX) / UZ_SUB + 1;   // a piece in LDS: rows of 256 bytes, one more for the source's misalignment
constexpr uint32_t UZ_NOPS = UZ_PIECE_MAX + 6;         // operator b: the register over 1 << b zero bytes
constexpr uint32_t UZ_NONE = 0xFFFFFFFFu;
typedef __attribute__((address_space(1))) uint8_t uz_gu8;
typedef __attribute__((address_space(1))) const uint8_t uz_gcu8;
typedef uint32_t uz_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uz_u32x4 uz_gu4;
typedef __attribute__((address_space(1))) const uz_u32x4 uz_gcu4;

struct UzCryptJob { uint64_t src, dst, n; uint32_t check, pad; };       // n: with the 12 header bytes; dst: where the byte behind the header goes
struct UzGatherJob { uint64_t src, n; uint32_t slot, pad; };            // slot: the entry's verdict of k_uz_decode (UZ_NONE: not encrypted)
struct UzStoreEnt { uint64_t src, dst, len; uint32_t crc_in, first, npieces, flags; };   // flags bit 0: the bytes are in place already (decoded there): sum only
struct UzOps { uint32_t mat[UZ_NOPS][32]; };

__device__ __forceinline__ uint32_t uz_gf2(const uint32_t *m, uint32_t v) {
  uint32_t s = 0;
#pragma unroll
  for (int b = 0; b < 32; b++) s ^= (0u - ((v >> b) & 1u)) & m[b];
  return s;
}
// the register `reg` advanced over len zero bytes (len < 1 << UZ_NOPS)
__device__ __forceinline__ uint32_t uz_zeros(const UzOps *__restrict__ ops, uint32_t reg, uint64_t len) {
  for (uint32_t b = 0; b < UZ_NOPS; b++) if ((len >> b) & 1u) reg = uz_gf2(ops->mat[b], reg);
  return reg;
}
__device__ __forceinline__ void uz_crc_table(uint32_t *tab) {
  for (uint32_t t = threadIdx.x; t < 256; t += UZ_WAVE) {
    uint32_t l = t;
    for (int b = 0; b < 8; b++) l = (l & 1) ? (l >> 1) ^ 0xEDB88320u : l >> 1;      // Prepare_table, zip-crc_crypto.adb:31-47
    tab[t] = l;
  }
}

// ---- CRC_Crypto.Decode out of place, one lane per entry, sixteen bytes a step ----
#define UZ_KEY_STEP(cb, p) do { const uint32_t t_ = (k2 & 0xFFFFu) | 2u;                     /* Crypto_code :102-108 */ \
    p = ((cb) ^ ((t_ * (t_ ^ 1u)) >> 8)) & 0xFFu;                                             /* Decode :130-137 */ \
    k0 = tab[(k0 ^ p) & 0xFF] ^ (k0 >> 8);                                                    /* Update_keys :90-99, with the PLAIN byte */ \
    k1 = (k1 + (k0 & 0xFFu)) * 134775813u + 1u; \
    k2 = tab[(k2 ^ (k1 >> 24)) & 0xFF] ^ (k2 >> 8); } while (0)
#define UZ_KEY_WORD(w, o) do { uint32_t p_; o = 0; \
    UZ_KEY_STEP((w) & 0xFFu, p_); o |= p_; UZ_KEY_STEP(((w) >> 8) & 0xFFu, p_); o |= p_ << 8; \
    UZ_KEY_STEP(((w) >> 16) & 0xFFu, p_); o |= p_ << 16; UZ_KEY_STEP((w) >> 24, p_); o |= p_ << 24; } while (0)

__global__ void __launch_bounds__(UZ_WAVE) k_uz_decode(const UzCryptJob *__restrict__ jobs, uint32_t count, uint32_t key0, uint32_t key1, uint32_t key2, int32_t *verdict) {
  __shared__ uint32_t tab[256];
  uz_crc_table(tab);
  __syncthreads();
  const uint32_t e = blockIdx.x * UZ_WAVE + threadIdx.x;
  if (e >= count) return;
  const UzCryptJob J = jobs[e];
  uz_gcu8 *src = (uz_gcu8 *)J.src;
  uz_gu8 *dst = (uz_gu8 *)J.dst;                         // the byte behind the header goes to dst [0]
  const uint64_t n = J.n;
  uint32_t k0 = key0, k1 = key1, k2 = key2, p = 0;
  for (uint32_t i = 0; i < 12; i++) UZ_KEY_STEP((uint32_t)src[i], p);
  if (p != J.check) { verdict[e] = ZADA_E_PASSWORD; return; }
  verdict[e] = 0;
  uint64_t pos = 12;
  while (pos < n && (((uintptr_t)(src + pos)) & 15u)) { UZ_KEY_STEP((uint32_t)src[pos], p); dst[pos - 12] = (uint8_t)p; pos++; }
  const bool al = ((((uintptr_t)(src + pos)) ^ ((uintptr_t)(dst + (pos - 12)))) & 15u) == 0;     // (the scratch is laid out so; a stored entry's output is where it is)
  while (pos + 16 <= n) {
    const uz_u32x4 w = *(uz_gcu4 *)(src + pos);
    uz_u32x4 o;
    UZ_KEY_WORD(w.x, o.x); UZ_KEY_WORD(w.y, o.y); UZ_KEY_WORD(w.z, o.z); UZ_KEY_WORD(w.w, o.w);
    uz_gu8 *d = dst + (pos - 12);
    if (al) *(uz_gu4 *)d = o;
    else {
      const uint32_t ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (uint32_t b = 0; b < 16; b++) d[b] = (uint8_t)(ow[b >> 2] >> ((b & 3u) * 8u));
    }
    pos += 16;
  }
  while (pos < n) { UZ_KEY_STEP((uint32_t)src[pos], p); dst[pos - 12] = (uint8_t)p; pos++; }
}

// ---- the nine header bytes of the LZMA payloads, sixteen bytes per entry ----
__global__ void __launch_bounds__(UZ_WAVE) k_uz_gather(const UzGatherJob *__restrict__ jobs, uint32_t count, const int32_t *__restrict__ verdict, uint8_t *out16) {
  const uint32_t e = blockIdx.x * UZ_WAVE + threadIdx.x;
  if (e >= count) return;
  const UzGatherJob J = jobs[e];
  const bool live = J.slot == UZ_NONE || verdict[J.slot] == 0;
  uz_gcu8 *src = (uz_gcu8 *)J.src;
  uint32_t w[4] = {0, 0, 0, 0};
  if (live) for (uint32_t i = 0; i < 9 && i < J.n; i++) w[i >> 2] |= (uint32_t)src[i] << ((i & 3u) * 8u);
  uz_u32x4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
  *(uz_u32x4 *)(out16 + (uint64_t)e * 16) = v;
}

// ---- stored entries: copy and CRC-32, one wave per piece ----
__device__ __forceinline__ uint32_t uz_at(uint32_t q) { return (q >> 8) * UZ_ROW + (q & 255u); }        // LDS address of byte q of the staged piece
__device__ __forceinline__ uint32_t uz_bytes(const uint8_t *row, uint32_t len, const uint32_t *tab, uint32_t r) {
  for (uint32_t i = 0; i < len; i++) r = tab[(r ^ row[i]) & 0xFF] ^ (r >> 8);
  return r;
}

__global__ void __launch_bounds__(UZ_WAVE) k_uz_store(const UzPiece *__restrict__ pieces, const UzStoreEnt *__restrict__ ents, const UzOps *__restrict__ ops,
                                                      uint32_t *raw, uint32_t *crc_out) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t m[6][32];
  __shared__ __attribute__((aligned(16))) uint8_t rows[UZ_ROWS * UZ_ROW];
  const uint32_t lane = threadIdx.x;
  const UzPiece P = pieces[blockIdx.x];
  const UzStoreEnt E = ents[P.entry];
  uz_gcu8 *src = (uz_gcu8 *)(E.src + P.off);
  uz_gu8 *dst = (uz_gu8 *)(E.dst + P.off);
  const uint32_t len = P.len;                            // 1 .. 1 << UZ_PIECE_MAX
  uz_crc_table(tab);
  for (uint32_t t = lane; t < 6 * 32; t += UZ_WAVE) m[t >> 5][t & 31] = ops->mat[8 + (t >> 5)][t & 31];      // 256 << j zero bytes
  // the piece in LDS behind sh zero bytes, sh = the source's offset in its 16-byte word: the aligned loads land on aligned LDS words, and zero bytes
  // in front of a register started from 0 leave it 0
  const uint32_t sh = (uint32_t)((uintptr_t)src & 15u), qlen = sh + len;
  if (lane < sh) rows[lane] = 0;
  uint32_t h = (16u - sh) & 15u;
  if (h > len) h = len;
  if (lane < h) rows[uz_at(sh + lane)] = src[lane];
  const uint32_t words = (len - h) / 16u;
  {
    uz_gcu4 *s4 = (uz_gcu4 *)(src + h);
    for (uint32_t w = lane; w < words; w += UZ_WAVE) *(uz_u32x4 *)(rows + uz_at(sh + h + 16u * w)) = s4[w];
  }
  for (uint32_t i = h + words * 16u + lane; i < len; i += UZ_WAVE) rows[uz_at(sh + i)] = src[i];
  __syncthreads();
  // raw register of the staged bytes: per row, then the register behind every row by a scan (every row before the last is full), then the last row
  // again from its true start -- as k_inf_crc does within a tile
  const uint32_t o = lane * UZ_SUB;
  const uint32_t rl = o >= qlen ? 0u : qlen - o < UZ_SUB ? qlen - o : UZ_SUB;
  uint32_t v = uz_bytes(rows + lane * UZ_ROW, rl, tab, 0u);
  for (int j = 0; j < 6; j++) {
    const uint32_t u = __shfl_up(v, 1u << j, 64);
    if (lane >= (1u << j)) v ^= uz_gf2(m[j], u);
  }
  const uint32_t last = (qlen - 1) / UZ_SUB;             // 0 .. 64: row 64 holds what the misalignment pushed out of the 64 rows of the lanes
  const uint32_t doer = last < UZ_WAVE ? last : UZ_WAVE - 1;
  uint32_t before = __shfl_up(v, 1u, 64);
  if (lane == 0) before = 0;
  if (last >= UZ_WAVE) before = v;
  uint32_t after = 0;
  if (lane == doer) after = uz_bytes(rows + last * UZ_ROW, qlen - last * UZ_SUB, tab, before);
  const uint32_t rawp = (uint32_t)__shfl((int)after, (int)doer, 64);
  if (lane == 0) {
    if (E.npieces == 1) crc_out[P.entry] = uz_zeros(ops, E.crc_in, len) ^ rawp;
    else raw[blockIdx.x] = rawp;
  }
  if (E.flags & 1u) return;
  // the piece at the destination's alignment
  const uint32_t da = (uint32_t)((uintptr_t)dst & 15u);
  uint32_t hd = (16u - da) & 15u;
  if (hd > len) hd = len;
  if (lane < hd) dst[lane] = rows[uz_at(sh + lane)];
  const uint32_t dwords = (len - hd) / 16u, qb = sh + hd;
  uz_gu4 *d4 = (uz_gu4 *)(dst + hd);
  if ((qb & 15u) == 0) {
    for (uint32_t w = lane; w < dwords; w += UZ_WAVE) d4[w] = *(const uz_u32x4 *)(rows + uz_at(qb + 16u * w));
  } else if ((qb & 3u) == 0) {
    for (uint32_t w = lane; w < dwords; w += UZ_WAVE) {
      const uint32_t q = qb + 16u * w;
      uz_u32x4 x;
      x.x = *(const uint32_t *)(rows + uz_at(q)); x.y = *(const uint32_t *)(rows + uz_at(q + 4)); x.z = *(const uint32_t *)(rows + uz_at(q + 8)); x.w = *(const uint32_t *)(rows + uz_at(q + 12));
      d4[w] = x;
    }
  } else {
    for (uint32_t w = lane; w < dwords; w += UZ_WAVE) {
      const uint32_t q = qb + 16u * w;
      uint32_t xw[4] = {0, 0, 0, 0};
#pragma unroll
      for (uint32_t b = 0; b < 16; b++) xw[b >> 2] |= (uint32_t)rows[uz_at(q + b)] << ((b & 3u) * 8u);
      uz_u32x4 x; x.x = xw[0]; x.y = xw[1]; x.z = xw[2]; x.w = xw[3];
      d4[w] = x;
    }
  }
  for (uint32_t i = hd + dwords * 16u + lane; i < len; i += UZ_WAVE) dst[i] = rows[uz_at(sh + i)];
}

// ---- the pieces' registers folded, one wave per entry of more than one piece ----
__global__ void __launch_bounds__(UZ_WAVE) k_uz_fold(const UzStoreEnt *__restrict__ ents, const uint32_t *__restrict__ list, const uint32_t *__restrict__ raw,
                                                     const UzOps *__restrict__ ops, uint32_t plog, uint32_t *crc_out) {
  __shared__ uint32_t m[6][32];
  const uint32_t lane = threadIdx.x, e = list[blockIdx.x];
  for (uint32_t t = lane; t < 6 * 32; t += UZ_WAVE) m[t >> 5][t & 31] = ops->mat[plog + (t >> 5)][t & 31];    // piece << j zero bytes
  __syncthreads();
  const UzStoreEnt E = ents[e];
  const uint32_t np = E.npieces;
  const uint32_t part = (uint32_t)(E.len & ((1ull << plog) - 1));         // bytes of the last piece if it is not a full one
  uint32_t reg = E.crc_in;
  for (uint32_t k0 = 0; k0 < np; k0 += UZ_WAVE) {
    const uint32_t cnt = np - k0 < UZ_WAVE ? np - k0 : UZ_WAVE;
    uint32_t v = lane < cnt ? raw[E.first + k0 + lane] : 0u;
    if (lane == 0) v ^= uz_gf2(m[0], reg);
    for (int j = 0; j < 6; j++) {
      const uint32_t u = __shfl_up(v, 1u << j, 64);
      if (lane >= (1u << j)) v ^= uz_gf2(m[j], u);
    }
    // v: the register behind the lane's piece, every piece up to it taken as full -- which the entry's last one may not be
    if (k0 + cnt == np && part) {
      const uint32_t before = cnt >= 2 ? (uint32_t)__shfl((int)v, (int)(cnt - 2), 64) : reg;
      reg = uz_zeros(ops, before, part) ^ raw[E.first + np - 1];
    } else reg = (uint32_t)__shfl((int)v, (int)(cnt - 1), 64);
  }
  if (lane == 0) crc_out[e] = reg;
}

// ---- host side ----
struct UzState {
  UzOps *d_ops = nullptr;
  DevBuf tabs, ptab, scratch, out;      // decode / gather tables; the stored entries' tables; the decoded copies of encrypted entries; the test-only form's outputs
};

static UzState *uz_state(Ctx *c) {
  if (c->uz) return (UzState *)c->uz;
  UzState *S = new (std::nothrow) UzState();
  if (!S) return nullptr;
  UzOps h;
  {
    uint32_t tab[256], op[32], sq[32];
    for (uint32_t t = 0; t < 256; t++) { uint32_t l = t; for (int b = 0; b < 8; b++) l = (l & 1) ? (l >> 1) ^ 0xEDB88320u : l >> 1; tab[t] = l; }
    for (int i = 0; i < 32; i++) { uint32_t r = 1u << i; r = tab[r & 0xFF] ^ (r >> 8); op[i] = r; }                 // one zero byte
    auto square = [&] { for (int i = 0; i < 32; i++) { uint32_t v = op[i], s = 0; for (int j = 0; v; j++, v >>= 1) if (v & 1) s ^= op[j]; sq[i] = s; } memcpy(op, sq, sizeof op); };
    for (uint32_t b = 0; b < UZ_NOPS; b++) { memcpy(h.mat[b], op, sizeof op); square(); }
  }
  if (hipMalloc((void **)&S->d_ops, sizeof(UzOps)) != hipSuccess || hipMemcpy(S->d_ops, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (S->d_ops) hipFree(S->d_ops);
    delete S;
    return nullptr;
  }
  c->uz = S;
  return S;
}
void unzip_destroy(Ctx *c) {
  UzState *S = (UzState *)c->uz;
  if (!S) return;
  for (DevBuf *b : {&S->tabs, &S->ptab, &S->scratch, &S->out}) dev_free(*b);
  hipFree(S->d_ops);
  delete S;
  c->uz = nullptr;
}
struct UzCarve {
  uint64_t at = 0;
  uint64_t take(uint64_t bytes) { const uint64_t o = at; at += (bytes + 255) & ~255ull; return o; }
};

#define UZ_HIP(call, what) do { if (hip_check(c, (call), what)) return ZADA_E_HIP_; } while (0)

// the stored entries se [0 .. ns) (len slen [s] > 0; first / npieces are filled here) through k_uz_store and k_uz_fold, in pieces of 2 ** plog bytes;
// crc [s]: the registers behind them.  zip: the archive writer calls (its errors name that entry point).
static int uz_store_run(Ctx *c, UzState *S, std::vector<UzStoreEnt> &se, const std::vector<uint64_t> &slen, std::vector<uint32_t> &crc, uint32_t plog, bool zip) {
  hipStream_t st = c->stream;
  const uint32_t ns = (uint32_t)se.size();
  std::vector<uint32_t> sid(ns), fold;
  for (uint32_t s = 0; s < ns; s++) sid[s] = s;
  uint64_t total = 0;
  for (uint32_t s = 0; s < ns; s++) total += uz_piece_count(slen[s], plog);
  if (total >= (1ull << 31)) {
    c->err = zip ? "zada_zip_device: more pieces of stored entries than 2 ** 31" : "zada_unzip_device: more pieces of stored entries than 2 ** 31";
    return ZADA_E_TOO_LARGE;
  }
  std::vector<UzPiece> pieces;
  std::vector<uint64_t> first;
  uz_pieces(slen.data(), sid.data(), ns, plog, pieces, first);
  for (uint32_t s = 0; s < ns; s++) {
    se[s].first = (uint32_t)first[s]; se[s].npieces = (uint32_t)(first[s + 1] - first[s]);
    if (se[s].npieces > 1) fold.push_back(s);
  }
  const uint32_t NP = (uint32_t)pieces.size(), nf = (uint32_t)fold.size();
  UzCarve pc;
  const uint64_t p_ent = pc.take((uint64_t)ns * sizeof(UzStoreEnt)), p_pc = pc.take((uint64_t)NP * sizeof(UzPiece)), p_fold = pc.take((uint64_t)nf * 4),
                 p_raw = pc.take((uint64_t)NP * 4), p_crc = pc.take((uint64_t)ns * 4);
  const int rc = dev_grow(c, S->ptab, pc.at, zip ? "hipMalloc (zip piece tables)" : "hipMalloc (unzip piece tables)");
  if (rc) return rc;
  uint8_t *T = S->ptab.p;
  hipMemcpyAsync(T + p_ent, se.data(), (size_t)ns * sizeof(UzStoreEnt), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(T + p_pc, pieces.data(), (size_t)NP * sizeof(UzPiece), hipMemcpyHostToDevice, st);
  if (nf) hipMemcpyAsync(T + p_fold, fold.data(), (size_t)nf * 4, hipMemcpyHostToDevice, st);
  c->tmark("unzip:store begin");
  hipLaunchKernelGGL(k_uz_store, dim3(NP), dim3(UZ_WAVE), 0, st, (const UzPiece *)(T + p_pc), (const UzStoreEnt *)(T + p_ent), (const UzOps *)S->d_ops, (uint32_t *)(T + p_raw),
                     (uint32_t *)(T + p_crc));
  c->tmark("unzip:k_uz_store");
  if (nf) {
    hipLaunchKernelGGL(k_uz_fold, dim3(nf), dim3(UZ_WAVE), 0, st, (const UzStoreEnt *)(T + p_ent), (const uint32_t *)(T + p_fold), (const uint32_t *)(T + p_raw), (const UzOps *)S->d_ops,
                       plog, (uint32_t *)(T + p_crc));
    c->tmark("unzip:k_uz_fold");
  }
  crc.resize(ns);
  hipMemcpyAsync(crc.data(), T + p_crc, (size_t)ns * 4, hipMemcpyDeviceToHost, st);
  UZ_HIP(hipGetLastError(), zip ? "zip store launch" : "unzip store launch");
  UZ_HIP(hipStreamSynchronize(st), zip ? "zip store" : "unzip store");
  return 0;
}
int unzip_store_entries(Ctx *c, uint32_t ns, const uint64_t *src, const uint64_t *dst, const uint64_t *len, uint32_t *crc) {
  if (!ns) return 0;
  UzState *S = uz_state(c);
  if (!S) { c->err = "zip: no memory for the tables"; return ZADA_E_NOMEM; }
  std::vector<UzStoreEnt> se(ns);
  std::vector<uint64_t> slen(len, len + ns);
  for (uint32_t s = 0; s < ns; s++) se[s] = UzStoreEnt{src[s], dst[s], len[s], crc[s], 0, 0, 0};
  std::vector<uint32_t> out;
  const int rc = uz_store_run(c, S, se, slen, out, UZ_PIECE_DEFAULT, true);      // (pieces of 16 KiB, as zw_groups counts them: not the reader's test knob)
  if (rc) return rc;
  for (uint32_t s = 0; s < ns; s++) crc[s] = out[s];
  return 0;
}
int unzip_sum_entries(Ctx *c, uint32_t ns, const uint64_t *at, const uint64_t *len, uint32_t *crc) {
  if (!ns) return 0;
  UzState *S = uz_state(c);
  if (!S) { c->err = "unzip: no memory for the tables"; return ZADA_E_NOMEM; }
  std::vector<UzStoreEnt> se(ns);
  std::vector<uint64_t> slen(len, len + ns);
  for (uint32_t s = 0; s < ns; s++) se[s] = UzStoreEnt{at[s], at[s], len[s], crc[s], 0, 0, 1u};      // (bit 0: the bytes are in place)
  std::vector<uint32_t> out;
  const int rc = uz_store_run(c, S, se, slen, out, UZ_PIECE_DEFAULT, false);
  if (rc) return rc;
  for (uint32_t s = 0; s < ns; s++) crc[s] = out[s];
  return 0;
}

// entries idx [0 .. n) of the table, entry idx [k]'s output at device address out [k]
static int uz_group(Ctx *c, UzState *S, const uint8_t *archive, const zada_unzip_entry *ent, zada_unzip_result *res, const std::vector<int> &idx,
                    const std::vector<uint64_t> &out, const uint32_t *keys0, bool *described) {
  const uint32_t n = (uint32_t)idx.size();
  hipStream_t st = c->stream;
  std::vector<uint8_t> done(n, 0);
  std::vector<uint64_t> src(n);                          // where the decoders find the entry's payload
  std::vector<uint32_t> slot(n, UZ_NONE);
  std::vector<UzCryptJob> cj;
  std::vector<UzGatherJob> gj;
  std::vector<uint32_t> gk;
  auto fail = [&](uint32_t k, int rc) { zada_unzip_result &R = res[idx[k]]; R.rc = rc; R.out_len = 0; R.in_used = 0; done[k] = 1; };
  // what the host decides from the table alone; the scratch of the encrypted entries
  uint64_t scratch = 0;
  for (uint32_t k = 0; k < n; k++) {
    const zada_unzip_entry &e = ent[idx[k]];
    res[idx[k]].rc = ZADA_OK; res[idx[k]].out_len = 0; res[idx[k]].in_used = 0;
    src[k] = (uint64_t)(uintptr_t)(archive + e.in_off);
    if (uz_encrypted(e) && e.n_in < 12) { fail(k, ZADA_E_DATA); continue; }
    if (e.method == 0 && uz_payload(e) > e.cap) { fail(k, ZADA_E_DATA); continue; }
    if (!uz_encrypted(e)) continue;
    slot[k] = (uint32_t)cj.size();
    if (e.method == 0) cj.push_back(UzCryptJob{src[k], out[k], e.n_in, e.check, 0});
    else {
      const uint64_t a = (src[k] + 12) & 15u;            // (an offset for now: the scratch may still move)
      cj.push_back(UzCryptJob{src[k], scratch + a, e.n_in, e.check, 0});
      scratch += (a + uz_payload(e) + 15) & ~15ull;
    }
  }
  std::vector<uint32_t> gslot(n, UZ_NONE);               // an LZMA entry's row of the gathered header bytes
  for (uint32_t k = 0; k < n; k++) if (!done[k] && ent[idx[k]].method == 14) { gslot[k] = (uint32_t)gk.size(); gk.push_back(k); }
  const uint32_t nc = (uint32_t)cj.size(), ng = (uint32_t)gk.size();
  std::vector<int32_t> verdict(nc, 0);
  std::vector<uint8_t> h16((size_t)ng * 16, 0);
  c->tmark("unzip:begin");
  if (nc || ng) {
    int rc = scratch ? dev_grow(c, S->scratch, scratch + 16, "hipMalloc (unzip decoded copies)") : 0;
    if (rc) return rc;
    for (uint32_t k = 0; k < n; k++) {
      if (slot[k] == UZ_NONE) continue;
      UzCryptJob &J = cj[slot[k]];
      if (ent[idx[k]].method != 0) J.dst += (uint64_t)(uintptr_t)S->scratch.p;
      src[k] = J.dst;
    }
    gj.resize(ng);
    for (uint32_t g = 0; g < ng; g++) gj[g] = UzGatherJob{src[gk[g]], uz_payload(ent[idx[gk[g]]]), slot[gk[g]], 0};
    UzCarve tc;
    const uint64_t o_cj = tc.take((uint64_t)nc * sizeof(UzCryptJob)), o_gj = tc.take((uint64_t)ng * sizeof(UzGatherJob)), o_back = tc.take(0),
                   o_ver = tc.take((uint64_t)nc * 4), o_h16 = tc.take((uint64_t)ng * 16);
    rc = dev_grow(c, S->tabs, tc.at + 256, "hipMalloc (unzip tables)");
    if (rc) return rc;
    uint8_t *T = S->tabs.p;
    if (nc) {
      hipMemcpyAsync(T + o_cj, cj.data(), (size_t)nc * sizeof(UzCryptJob), hipMemcpyHostToDevice, st);
      hipLaunchKernelGGL(k_uz_decode, dim3((nc + UZ_WAVE - 1) / UZ_WAVE), dim3(UZ_WAVE), 0, st, (const UzCryptJob *)(T + o_cj), nc, keys0[0], keys0[1], keys0[2], (int32_t *)(T + o_ver));
      c->tmark("unzip:k_uz_decode");
    }
    if (ng) {
      hipMemcpyAsync(T + o_gj, gj.data(), (size_t)ng * sizeof(UzGatherJob), hipMemcpyHostToDevice, st);
      hipLaunchKernelGGL(k_uz_gather, dim3((ng + UZ_WAVE - 1) / UZ_WAVE), dim3(UZ_WAVE), 0, st, (const UzGatherJob *)(T + o_gj), ng, (const int32_t *)(T + o_ver), T + o_h16);
      c->tmark("unzip:k_uz_gather");
    }
    // one small copy: the verdicts and the header bytes lie side by side
    std::vector<uint8_t> back((size_t)(tc.at - o_back));
    hipMemcpyAsync(back.data(), T + o_back, back.size(), hipMemcpyDeviceToHost, st);
    UZ_HIP(hipGetLastError(), "unzip decode launch");
    UZ_HIP(hipStreamSynchronize(st), "unzip decode");
    if (nc) memcpy(verdict.data(), back.data() + (o_ver - o_back), (size_t)nc * 4);
    if (ng) memcpy(h16.data(), back.data() + (o_h16 - o_back), (size_t)ng * 16);
    for (uint32_t k = 0; k < n; k++) if (slot[k] != UZ_NONE && verdict[slot[k]] != 0) fail(k, ZADA_E_PASSWORD);
  }
  // the decoders
  std::vector<ReaderJob> rj;
  std::vector<ReaderRes> rr;
  std::vector<uint32_t> rk;
  // "inflate_par_min_kib": the large Deflate entries (with "inflate_par_deflate64" the Deflate64 ones too) on many waves each (zada_inflate_par.hip): one
  // after the other, or with "inflate_par_batch" all of the group in the same launches.  An entry that path does not take, a damaged one among them, is
  // left to the batch below, whose verdict and error text are the answer
  auto infp_selects = [&](uint32_t k) {
    const zada_unzip_entry &e = ent[idx[k]];
    return !done[k] && (e.method == 8 || (e.method == 9 && c->knob_infp_deflate64)) && uz_payload(e) >= ((uint64_t)c->knob_infp_min_kib << 10);
  };
  if (c->knob_infp_min_kib > 0 && c->knob_infp_batch) {
    std::vector<InfpbIn> bi;
    std::vector<uint32_t> bk;
    for (uint32_t k = 0; k < n; k++) {
      if (!infp_selects(k)) continue;
      const zada_unzip_entry &e = ent[idx[k]];
      bi.push_back(InfpbIn{src[k], uz_payload(e), out[k], e.cap, e.method, res[idx[k]].crc});
      bk.push_back(k);
    }
    std::vector<InfpbRes> br(bi.size());
    const int rc = inflate_par_batch(c, (uint32_t)bi.size(), bi.data(), br.data());
    if (rc < 0) return rc;
    for (size_t j = 0; j < bk.size(); j++) {
      if (!br[j].taken) continue;
      const uint32_t k = bk[j];
      zada_unzip_result &R = res[idx[k]];
      done[k] = 1; R.crc = br[j].crc; R.out_len = br[j].out_len; R.in_used = br[j].in_used + (uz_encrypted(ent[idx[k]]) ? 12 : 0);
    }
  } else if (c->knob_infp_min_kib > 0) {
    zada_inflate_par_info sum{}, one{};
    for (uint32_t k = 0; k < n; k++) {
      if (!infp_selects(k)) continue;
      const zada_unzip_entry &e = ent[idx[k]];
      zada_unzip_result &R = res[idx[k]];
      uint64_t ol = 0, iu = 0;
      uint32_t reg = R.crc;
      const int rc = inflate_par_try(c, (int)e.method, (const void *)(uintptr_t)src[k], uz_payload(e), (void *)(uintptr_t)out[k], e.cap, &ol, &iu, &reg);
      if (rc < 0) return rc;
      inflate_par_record(c, &one, nullptr);
      sum.chunks += one.chunks; sum.live_chunks += one.live_chunks; sum.repairs += one.repairs; sum.scout_rounds += one.scout_rounds;
      sum.marker_bytes += one.marker_bytes; sum.fell_back += one.fell_back; sum.streams += one.streams;
      if (one.fell_back) sum.reason = one.reason;
      if (rc == 0) { done[k] = 1; R.crc = reg; R.out_len = ol; R.in_used = iu + (uz_encrypted(e) ? 12 : 0); }
    }
    inflate_par_record(c, nullptr, &sum);
  }
  for (int pass = 0; pass < 4; pass++) {
    rj.clear(); rr.clear(); rk.clear();
    for (uint32_t k = 0; k < n; k++) {
      const zada_unzip_entry &e = ent[idx[k]];
      const bool lz = e.method == 14;
      if (done[k]) continue;
      if (!(pass == 0 ? (e.method == 8 || e.method == 9) : pass == 1 ? e.method == 12 : pass == 2 ? lz : uz_method_legacy(e.method))) continue;
      ReaderJob J{src[k], out[k], uz_payload(e), e.cap, (int32_t)e.method, (e.flags & 2u) ? 1u : 0u, 0, idx[k], 0};
      if (e.method == 6) J.eos = e.flags & 6u;             // (an Implode row: the entry's general-purpose bits 1 and 2)
      if (lz) J.lit_elems = unlzma_hbm_elems(h16.data() + (size_t)gslot[k] * 16, J.n_in);
      rj.push_back(J); rr.push_back(ReaderRes{0, res[idx[k]].crc, 0, 0}); rk.push_back(k);
    }
    const uint32_t E = (uint32_t)rj.size();
    if (!E) continue;
    const int rc = pass == 0 ? inflate_run_jobs(c, E, rj.data(), rr.data(), described) : pass == 1 ? bunzip2_run_jobs(c, E, rj.data(), rr.data(), described)
                 : pass == 2 ? unlzma_run_jobs(c, E, rj.data(), rr.data(), described) : unlegacy_run_jobs(c, E, rj.data(), rr.data(), described);
    if (rc) return rc;
    for (uint32_t j = 0; j < E; j++) {
      const uint32_t k = rk[j];
      zada_unzip_result &R = res[idx[k]];
      done[k] = 1;
      if (rr[j].rc) { R.rc = rr[j].rc; continue; }
      R.crc = rr[j].crc; R.out_len = rr[j].out_len; R.in_used = rr[j].in_used + (uz_encrypted(ent[idx[k]]) ? 12 : 0);
    }
  }
  // the stored entries
  std::vector<UzStoreEnt> se;
  std::vector<uint64_t> slen;
  std::vector<uint32_t> sk;
  for (uint32_t k = 0; k < n; k++) {
    const zada_unzip_entry &e = ent[idx[k]];
    if (done[k] || e.method != 0) continue;
    const uint64_t len = uz_payload(e);
    res[idx[k]].out_len = len; res[idx[k]].in_used = e.n_in;
    if (len == 0) continue;
    slen.push_back(len); sk.push_back(k);
    se.push_back(UzStoreEnt{src[k], out[k], len, res[idx[k]].crc, 0, 0, uz_encrypted(e) ? 1u : 0u});
  }
  if (!se.empty()) {
    std::vector<uint32_t> crc;
    const int rc = uz_store_run(c, S, se, slen, crc, (uint32_t)c->knob_unzip_piece, false);
    if (rc) return rc;
    for (uint32_t s = 0; s < (uint32_t)se.size(); s++) res[idx[sk[s]]].crc = crc[s];
  }
  return 0;
}

}  // namespace zada

using namespace zada;

int zada_unzip_device(zada_ctx *z, const void *d_archive, uint64_t archive_len, void *d_out, uint64_t out_bytes, int count, const zada_unzip_entry *ent,
                      const uint32_t keys0[3], zada_unzip_result *res) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;                                            // (as every entry point: zada_lzma_export_state)
  if (count && (!ent || !res)) { c->err = "zada_unzip_device: null argument"; return ZADA_E_INVALID; }
  if (archive_len && !d_archive) { c->err = "zada_unzip_device: null archive"; return ZADA_E_INVALID; }
  int bad = -1, why = 0;
  int rc = uz_check(ent, count, archive_len, out_bytes, d_out != nullptr, keys0 != nullptr, &bad, &why, c->knob_unzip_legacy);
  if (rc) {
    char buf[200];
    snprintf(buf, sizeof buf, "zada_unzip_device: entry %d: %s", bad, uz_why_text(why, c->knob_unzip_legacy));
    c->err = buf;
    return rc;
  }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  if (count == 0) { hipStreamSynchronize(c->stream); return ZADA_OK; }
  UzState *S = uz_state(c);
  if (!S) { c->err = "unzip: no memory for the tables"; return ZADA_E_NOMEM; }
  const uint8_t *archive = (const uint8_t *)d_archive;
  bool described = false;
  std::vector<int> idx, ends;
  std::vector<uint64_t> out;
  if (d_out) ends.push_back(count);
  else uz_groups(ent, count, (uint64_t)c->knob_batch_mib << 20, ends);
  c->tbegin();
  int g0 = 0;
  for (int g1 : ends) {
    idx.clear(); out.clear();
    uint64_t bytes = 0;
    for (int i = g0; i < g1; i++) { idx.push_back(i); out.push_back(d_out ? ent[i].out_off : bytes); bytes += uz_slot(ent[i].cap); }
    if (!d_out) {
      rc = dev_grow(c, S->out, bytes + 16, "hipMalloc (unzip test-only outputs)");
      if (rc) { c->tend(); return rc; }
    }
    const uint64_t base = (uint64_t)(uintptr_t)(d_out ? d_out : (void *)S->out.p);
    for (uint64_t &o : out) o += base;
    rc = uz_group(c, S, archive, ent, res, idx, out, keys0, &described);
    if (rc) { hipStreamSynchronize(c->stream); (void)hipGetLastError(); c->tend(); return rc; }
    g0 = g1;
  }
  c->tend();
  hipStreamSynchronize(c->stream);
  int worst = 0;
  for (int i = 0; i < count; i++) {
    if (res[i].rc < worst) worst = res[i].rc;
    if (res[i].rc && !described) {
      char buf[200];
      snprintf(buf, sizeof buf, res[i].rc == ZADA_E_PASSWORD ? "zada_unzip_device: entry %d: the decoded encryption header does not end in the entry's check byte (wrong password)"
                                                             : "zada_unzip_device: entry %d: its data do not fit what the directory promises", i);
      c->err = buf;
      described = true;
    }
  }
  return worst;
}
