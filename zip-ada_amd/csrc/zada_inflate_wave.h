// zada_inflate_wave.h -- what a wave of the Inflate kernels works with, shared by zada_inflate.hip (one wave per entry) and zada_inflate_par.hip
// (one wave per chunk of one stream): the bit reader over input staged in LDS, and the expansion of a queue of up to 64 tokens.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zada_inflate_logic.h"

namespace zada {

constexpr uint32_t INF_WAVE = 64;
constexpr uint32_t INF_STAGE = 2048;                 // bytes of compressed input in LDS at a time
// the entries' bytes are in device memory: global (not flat) loads and stores, which leave the LDS counter alone
typedef __attribute__((address_space(1))) uint8_t gu8;
typedef __attribute__((address_space(1))) const uint8_t gcu8;
typedef uint32_t inf_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) inf_u32x4 gu4;
typedef __attribute__((address_space(1))) const inf_u32x4 gcu4;
typedef __attribute__((address_space(1))) const uint32_t gcu32;

// ---- the bit reader of a wave: the input staged in LDS, 32 bits at a time into a 64-bit register pair ----
struct InfWaveReader {
  gcu8 *in; uint64_t n, ip, base; uint64_t hold; uint32_t nb; uint32_t *stage;     // stage: INF_STAGE / 4 + 2 words; holds input bytes [base, base + INF_STAGE)
  __device__ __forceinline__ void fill(uint64_t at) {                                       // all lanes; at: multiple of 4
    __syncthreads();
    base = at;
    const uint32_t lane = threadIdx.x;
    const bool al4 = (((uintptr_t)in) & 3u) == 0;
    for (uint32_t w = lane; w < INF_STAGE / 4 + 2; w += INF_WAVE) {
      const uint64_t o = at + (uint64_t)w * 4;
      uint32_t v = 0;
      if (o + 4 <= n) {
        if (al4) v = *(gcu32 *)(in + o);
        else v = (uint32_t)in[o] | (uint32_t)in[o + 1] << 8 | (uint32_t)in[o + 2] << 16 | (uint32_t)in[o + 3] << 24;
      } else {
        for (uint32_t k = 0; k < 4; k++) if (o + k < n) v |= (uint32_t)in[o + k] << (8 * k);
      }
      stage[w] = v;
    }
    __syncthreads();
  }
  __device__ __forceinline__ void open(gcu8 *p, uint64_t len, uint64_t at, uint32_t *st) {
    in = p; n = len; stage = st; hold = 0; nb = 0; ip = at;
    fill(at & ~3ull);
  }
  __device__ __forceinline__ void need32() {
    if (nb > 32) return;
    if (ip < base || ip + 4 > base + INF_STAGE) fill(ip & ~3ull);
    const uint32_t o = (uint32_t)(ip - base);
    const uint32_t lo = ZINF_UNI(stage[o >> 2]), hi = ZINF_UNI(stage[(o >> 2) + 1]);
    const uint32_t w = (uint32_t)((((uint64_t)hi << 32) | lo) >> ((o & 3u) * 8u));
    hold |= (uint64_t)w << nb; nb += 32; ip += 4;
  }
  __device__ __forceinline__ void drop(uint32_t k) { hold >>= k; nb -= k; }
  __device__ __forceinline__ uint64_t used_bits() const { return ip * 8 - nb; }
  __device__ __forceinline__ bool overrun() const { return used_bits() > n * 8; }
};

// The queue of up to 64 tokens, lane q holding token q (len 0: none; dist 0: the literal `val`), written behind `pos`.  fence_pos: every byte
// before it is known to be in memory for all lanes of the wave.
__device__ __forceinline__ void inf_expand(gu8 *out, uint64_t pos, uint32_t q, uint32_t my_len, uint32_t my_dist, uint32_t my_val, uint64_t &fence_pos) {
  const uint32_t lane = threadIdx.x;
  uint32_t len = lane < q ? my_len : 0u, incl = len;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
  const uint64_t start = pos + (incl - len);
  if (len && my_dist == 0) out[start] = (uint8_t)my_val;
  uint64_t mask = __ballot(len != 0 && my_dist != 0);
  while (mask) {
    const int k = __ffsll((unsigned long long)mask) - 1;
    mask &= mask - 1;
    const uint32_t L = (uint32_t)__builtin_amdgcn_readlane((int)len, k), D = (uint32_t)__builtin_amdgcn_readlane((int)my_dist, k);
    const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)(incl - len), k);
    const uint64_t P = pos + off;
    const uint64_t src_end = P - D + (L < D ? L : D);
    if (src_end > fence_pos) {
      // (for a workgroup on one CU the memory model orders a wave's loads behind its stores at the L1 by itself and the fences compile to no
      // instruction; the wait on the wave's outstanding stores is stated on top of them: vmcnt (0), the other counters left alone)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      fence_pos = P;
    }
    gu8 *dst = out + P;
    gu8 *src = out + (P - D);
    if (D >= L) { for (uint32_t i = lane; i < L; i += INF_WAVE) dst[i] = src[i]; }
    else { for (uint32_t i = lane; i < L; i += INF_WAVE) dst[i] = src[i % D]; }         // the overlapping case: the D bytes before P, over and over
  }
}

}  // namespace zada
