// zada_shrink.hip -- Shrink_1 (Zip format 1): Zip.Compress.Shrink_E (zip-compress-shrink_e.adb, shrink.ads) on the device, one wave per entry.
//
// LZW with codes of 9 .. 13 bits, the code size raised by the encoder (256, 1) and a PARTIAL clear when the table is found full (256, 2).  The chain is
// serial -- a byte is looked up under the code the bytes before it led to --, so an entry is one wave's work and a batch is what fills the device.
//
// The table in LDS, per entry:
//   prefix [8192] u16, suffix [8192] u8           the nodes
//   hash [12288] u16                              (prefix, suffix) -> code, linear probing; the wave looks at 64 slots per step.  The first hit in probe
//                                                 order is the EARLIEST added node: Table_Lookup walks the siblings in the order they were added, and the
//                                                 Table_Add behind a clear adds without a lookup, so a pair can be in the table twice
//   child [256] u32                               one bit per node: it is some node's prefix
//   free [256] u32                                one bit per node: it is free.  Free nodes are taken in ascending order (free_list is ascending after
//                                                 Initialize_Data_Structures and after Clear_Leaf_Nodes), so the list is this mask and a cursor
// The partial clear in closed form (Prune is recursive in the reference; tests/legacy/shrink_model.c proves the two equal): every node from 257 on
// that has no child at that moment becomes free; the others stay, the child bits and the hash table are made again from them.  The lanes do it.
// Codes are queued, 64 at a time, and packed by the wave: a scan of their sizes, an OR into LDS words, byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <new>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_legacy.h"

namespace zada {

constexpr uint32_t SH_NODES = 8192, SH_HASH = 12288, SH_EMPTY = 0xFFFF, SH_FIRST = 257, SH_STAGE = 256;
constexpr uint32_t SH_OB_WORDS = 28;                     // 7 carried bits + 64 codes of 13 bits = 839 bits

struct ShrinkLds {
  uint16_t prefix[SH_NODES];
  uint32_t hash32[SH_HASH / 2];                           // u16 slots; words for the compare-and-swap of the rebuild
  uint32_t child[SH_NODES / 32], free_[SH_NODES / 32];
  uint32_t queue[64], ob[SH_OB_WORDS];
  uint8_t suffix[SH_NODES];
  uint8_t stage[SH_STAGE];
};

__device__ __forceinline__ uint32_t sh_hash(uint32_t prefix, uint32_t suffix) {
  return (uint32_t)(((uint64_t)((prefix * 256u + suffix) * 2654435761u) * SH_HASH) >> 32);
}
__device__ __forceinline__ uint32_t sh_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// (prefix, suffix) in the table: the code, or SH_EMPTY with *slot = the first empty slot of the probe sequence.  lookup = false: the first empty slot only.
__device__ __forceinline__ uint32_t sh_probe(const ShrinkLds &S, uint32_t prefix, uint32_t suffix, bool lookup, uint32_t *slot, int lane) {
  const uint16_t *hash = (const uint16_t *)S.hash32;
  uint32_t h = sh_hash(prefix, suffix);
  for (;;) {
    uint32_t s = h + (uint32_t)lane;
    if (s >= SH_HASH) s -= SH_HASH;
    const uint32_t v = hash[s];
    const bool empty = v == SH_EMPTY;
    const bool hit = lookup && !empty && S.prefix[v] == prefix && S.suffix[v] == suffix;
    const uint64_t mh = __ballot(hit), me = __ballot(empty);
    const int fh = mh ? __builtin_ctzll(mh) : 64, fe = me ? __builtin_ctzll(me) : 64;
    if (fh < fe) return sh_uniform(__shfl(v, fh));
    if (fe < 64) { uint32_t t = h + (uint32_t)fe; *slot = t >= SH_HASH ? t - SH_HASH : t; return SH_EMPTY; }
    h += 64;
    if (h >= SH_HASH) h -= SH_HASH;
  }
}

// the lowest free node from `cursor` on: no free node lies below the cursor, and the caller has counted that there is one
__device__ __forceinline__ uint32_t sh_next_free(const ShrinkLds &S, uint32_t cursor) {
  uint32_t w = cursor >> 5;
  uint32_t bits = sh_uniform(S.free_[w]) & (~0u << (cursor & 31));
  while (!bits && w + 1 < SH_NODES / 32) bits = sh_uniform(S.free_[++w]);
  return bits ? w * 32 + (uint32_t)__builtin_ctz(bits) : SH_NODES;
}

struct ShrinkOut { uint8_t *out; uint32_t cap, written, carry_bits, queued; };

// the queued codes go out: sizes scanned over the lanes, bits ORed into LDS words, whole bytes stored; `last`: the trailing bits too
__device__ void sh_flush(ShrinkLds &S, ShrinkOut &O, bool last, int lane) {
  __syncthreads();
  uint32_t code = 0, size = 0;
  if ((uint32_t)lane < O.queued) { const uint32_t q = S.queue[lane]; code = q & 0xFFFF; size = q >> 16; }
  uint32_t incl = size;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if (lane >= d) incl += t; }
  const uint32_t total = O.carry_bits + sh_uniform(__shfl(incl, 63));
  if (size) {
    const uint32_t pos = O.carry_bits + incl - size, w = pos >> 5, sh = pos & 31;
    atomicOr(&S.ob[w], code << sh);
    if (sh + size > 32) atomicOr(&S.ob[w + 1], code >> (32 - sh));
  }
  __syncthreads();
  const uint32_t nbytes = last ? (total + 7) >> 3 : total >> 3;
  const uint8_t *ob = (const uint8_t *)S.ob;
  for (uint32_t i = (uint32_t)lane; i < nbytes; i += 64)
    if (O.written + i < O.cap) O.out[O.written + i] = ob[i];
  const uint32_t keep = last ? 0 : (total & 7) ? ob[nbytes] : 0;
  __syncthreads();
  for (uint32_t i = (uint32_t)lane; i < SH_OB_WORDS; i += 64) S.ob[i] = i == 0 ? keep : 0;
  O.written += nbytes; O.carry_bits = last ? 0 : total & 7; O.queued = 0;
  __syncthreads();
}
__device__ __forceinline__ void sh_put(ShrinkLds &S, ShrinkOut &O, uint32_t code, uint32_t size, int lane) {
  S.queue[O.queued] = code | size << 16;                  // (every lane stores the same word)
  if (++O.queued == 64) sh_flush(S, O, false, lane);
}

__global__ void __launch_bounds__(64) k_shrink(uint32_t E, const uint8_t *__restrict__ in, const LegacyJob *__restrict__ jobs, uint8_t *__restrict__ out,
                                               uint32_t *__restrict__ bytes) {
  __shared__ ShrinkLds S;
  const int lane = threadIdx.x;
  const uint32_t e = blockIdx.x;
  if (e >= E) return;
  const LegacyJob J = jobs[e];
  const uint8_t *src = in + J.in_off;
  uint16_t *hash = (uint16_t *)S.hash32;
  // Initialize_Data_Structures
  for (uint32_t i = lane; i < SH_HASH / 2; i += 64) S.hash32[i] = 0xFFFFFFFFu;
  for (uint32_t i = lane; i < SH_NODES / 32; i += 64) { S.child[i] = 0; S.free_[i] = i < 8 ? 0u : i == 8 ? 0xFFFFFFFEu : 0xFFFFFFFFu; }
  for (uint32_t i = lane; i < SH_OB_WORDS; i += 64) S.ob[i] = 0;
  __syncthreads();
  ShrinkOut O{out + J.out_off, J.cap, 0, 0, 0};
  uint32_t nfree = SH_NODES - SH_FIRST, cursor = SH_FIRST, code_size = 9, max_code = 511, last = 0;

  for (uint32_t base = 0; base < J.n; base += SH_STAGE) {
    const uint32_t cnt = J.n - base < SH_STAGE ? J.n - base : SH_STAGE;
    __syncthreads();
    for (uint32_t i = lane; i < cnt; i += 64) S.stage[i] = src[base + i];
    __syncthreads();
    for (uint32_t k = 0; k < cnt; k++) {
      const uint32_t suffix = sh_uniform(S.stage[k]);
      if (base + k == 0) { last = suffix; continue; }
      uint32_t slot = 0;
      bool may_rise;
      if (nfree == 0) {
        // the table is full: the code, 256, 2, the partial clear, and the pair added without a lookup
        sh_put(S, O, last, code_size, lane); sh_put(S, O, 256, code_size, lane); sh_put(S, O, 2, code_size, lane);
        __syncthreads();
        uint32_t keep[4], cnt_free = 0;
        for (int q = 0; q < 4; q++) {
          const uint32_t w = (uint32_t)lane + 64u * q;
          const uint32_t nodes = w < 8 ? 0u : w == 8 ? 0xFFFFFFFEu : 0xFFFFFFFFu;      // the nodes from 257 on
          keep[q] = S.child[w] & nodes;
          const uint32_t fr = ~S.child[w] & nodes;
          cnt_free += (uint32_t)__builtin_popcount(fr);
          S.free_[w] = fr;
        }
        for (int d = 32; d; d >>= 1) cnt_free += __shfl_xor(cnt_free, d);
        __syncthreads();
        for (int q = 0; q < 4; q++) S.child[lane + 64 * q] = 0;
        for (uint32_t i = lane; i < SH_HASH / 2; i += 64) S.hash32[i] = 0xFFFFFFFFu;
        __syncthreads();
        for (int q = 0; q < 4; q++) {
          for (uint32_t m = keep[q]; m; m &= m - 1) {                               // a node that stays: its prefix has a child, the pair is in the table
            const uint32_t c = ((uint32_t)lane + 64u * q) * 32 + (uint32_t)__builtin_ctz(m), p = S.prefix[c];
            atomicOr(&S.child[p >> 5], 1u << (p & 31));
            uint32_t s = sh_hash(p, S.suffix[c]);
            for (;;) {
              const uint32_t sh = (s & 1) * 16, old = S.hash32[s >> 1];
              if (((old >> sh) & 0xFFFF) == SH_EMPTY) {
                if (atomicCAS(&S.hash32[s >> 1], old, (old & ~(0xFFFFu << sh)) | c << sh) == old) break;
                continue;
              }
              if (++s == SH_HASH) s = 0;
            }
          }
        }
        __syncthreads();
        nfree = sh_uniform(cnt_free); cursor = SH_FIRST;
        sh_probe(S, last, suffix, false, &slot, lane);
        may_rise = false;                                                           // (the table-full branch never looks at the code size)
      } else {
        const uint32_t at = sh_probe(S, last, suffix, true, &slot, lane);
        if (at != SH_EMPTY) { last = at; continue; }
        sh_put(S, O, last, code_size, lane);
        may_rise = true;
      }
      if (nfree) {                                                                  // Table_Add
        const uint32_t node = sh_next_free(S, cursor);
        S.free_[node >> 5] &= ~(1u << (node & 31));
        S.child[node >> 5] &= ~(1u << (node & 31));
        S.child[last >> 5] |= 1u << (last & 31);
        S.prefix[node] = (uint16_t)last; S.suffix[node] = (uint8_t)suffix;
        hash[slot] = (uint16_t)node;
        cursor = node + 1; nfree--;
      }
      last = suffix;
      if (may_rise && code_size < 13 && nfree) {
        cursor = sh_next_free(S, cursor);                                           // free_list (next_free)
        if (cursor > max_code) {
          sh_put(S, O, 256, code_size, lane); sh_put(S, O, 1, code_size, lane);
          code_size++; max_code = (1u << code_size) - 1;
        }
      }
    }
  }
  if (J.n) { sh_put(S, O, last, code_size, lane); }
  if (O.queued || O.carry_bits) sh_flush(S, O, true, lane);
  if (lane == 0) bytes[e] = O.written;
}

LegacyState *legacy_state(Ctx *c) {
  if (!c->lg) c->lg = new (std::nothrow) LegacyState();
  return (LegacyState *)c->lg;
}
int legacy_grow(Ctx *c, void **p, size_t *cap, size_t bytes, const char *what) {
  if (*p && *cap >= bytes) return 0;
  hipStreamSynchronize(c->stream);
  if (*p) { hipFree(*p); *p = nullptr; *cap = 0; }
  const size_t want = bytes + bytes / 8 + 4096;
  const hipError_t e = hipMalloc(p, want);
  if (e != hipSuccess) { (void)hipGetLastError(); hip_check(c, e, what); *p = nullptr; return ZADA_E_NOMEM; }
  *cap = want;
  return 0;
}
void legacy_destroy(Ctx *c) {
  LegacyState *L = (LegacyState *)c->lg;
  if (!L) return;
  if (L->tab) hipFree(L->tab);
  if (L->work) hipFree(L->work);
  delete L;
  c->lg = nullptr;
}

int shrink_encode_group(Ctx *c, uint32_t E, const uint8_t *d_in, const LegacyJob *jobs, uint8_t *d_out, uint64_t *bytes) {
  if (E == 0) return 0;
  LegacyState *L = legacy_state(c);
  if (!L) return ZADA_E_NOMEM;
  int rc = legacy_grow(c, &L->tab, &L->cap_tab, (size_t)E * (sizeof(LegacyJob) + 4), "hipMalloc (Shrink tables)");
  if (rc) return rc;
  LegacyJob *d_jobs = (LegacyJob *)L->tab;
  uint32_t *d_bytes = (uint32_t *)(d_jobs + E);
  hipStream_t st = c->stream;
  hipMemcpyAsync(d_jobs, jobs, (size_t)E * sizeof(LegacyJob), hipMemcpyHostToDevice, st);
  c->tmark("shrink:tables");
  hipLaunchKernelGGL(k_shrink, dim3(E), dim3(64), 0, st, E, d_in, d_jobs, d_out, d_bytes);
  c->tmark("k_shrink");
  std::vector<uint32_t> b(E);
  hipMemcpyAsync(b.data(), d_bytes, (size_t)E * 4, hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipStreamSynchronize(st), "Shrink")) return ZADA_E_HIP;
  for (uint32_t e = 0; e < E; e++) bytes[e] = b[e];
  return 0;
}

}  // namespace zada
