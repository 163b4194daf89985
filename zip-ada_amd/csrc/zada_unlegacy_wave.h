// zada_unlegacy_wave.h -- what one wave puts around the chains of zada_unlegacy_logic.h: the compressed input staged through LDS, the literal
// queue, and the copy whose source reads 0 in front of the entry's first byte (Copy_or_zero, unzip-decompress.adb:466-487), which Unreduce and
// Explode share.  It is not Inflate's copy (zada_inflate_wave.h): there a distance beyond the start is an error, here it is data.
// The window is the entry's own output in device memory, read through the pointer it is written through, with vector loads and stores only;
// a lane reads bytes that other lanes of its wave stored an instant ago, so before a copy whose source reaches beyond the bytes known to be
// complete the wave waits for its outstanding stores (settle, as in zada_unlzma.hip).  No other workgroup reads an entry's output inside the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zada {

constexpr uint32_t ULG_WAVE = 64;
constexpr uint32_t ULG_STAGE = 384;                  // bytes of compressed input in LDS at a time (a multiple of 4)
typedef __attribute__((address_space(1))) uint8_t ulg_gu8;
typedef __attribute__((address_space(1))) const uint8_t ulg_gcu8;
typedef __attribute__((address_space(1))) const uint32_t ulg_gcu32;

#define ULG_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))

__shared__ uint32_t s_ulg_stage[ULG_STAGE / 4];

struct UlgWaveBase {
  ulg_gcu8 *in; uint64_t n, ip, base;
  ulg_gu8 *out;
  uint32_t q, my;                  // the literal queue: q literals, lane k holding literal k, go to qpos ..
  uint64_t qpos, fence_pos;        // fence_pos: every byte before it is known to be in memory for all lanes of the wave

  __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
  __device__ __forceinline__ uint32_t lanes() const { return ULG_WAVE; }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ uint32_t uni(uint32_t v) const { return ULG_UNI(v); }

  __device__ __forceinline__ void fill(uint64_t at) {                 // all lanes; at: multiple of 4.  Nothing is read beyond n.
    __syncthreads();
    base = at;
    const uint32_t lane = threadIdx.x;
    const bool al4 = (((uintptr_t)in) & 3u) == 0;
    for (uint32_t w = lane; w < ULG_STAGE / 4; w += ULG_WAVE) {
      const uint64_t o = at + (uint64_t)w * 4;
      uint32_t v = 0;
      if (o + 4 <= n) {
        if (al4) v = *(ulg_gcu32 *)(in + o);
        else v = (uint32_t)in[o] | (uint32_t)in[o + 1] << 8 | (uint32_t)in[o + 2] << 16 | (uint32_t)in[o + 3] << 24;
      } else {
        for (uint32_t k = 0; k < 4; k++) if (o + k < n) v |= (uint32_t)in[o + k] << (8 * k);
      }
      s_ulg_stage[w] = v;
    }
    __syncthreads();
  }
  __device__ __forceinline__ void open(ulg_gcu8 *p, uint64_t len, ulg_gu8 *o) {
    in = p; n = len; ip = 0; out = o; q = 0; my = 0; qpos = 0; fence_pos = 0;
    fill(0);
  }
  // the next input byte; beyond the input it is 0, and ip counts on (zada_unlegacy_logic.h tells from ip what was consumed)
  __device__ __forceinline__ uint32_t byte() {
    uint32_t b = 0;
    if (ip < n) {
      if (ip >= base + ULG_STAGE) fill(ip & ~3ull);
      const uint32_t o = (uint32_t)(ip - base);
      b = (ULG_UNI(s_ulg_stage[o >> 2]) >> ((o & 3u) * 8u)) & 0xFFu;
    }
    ip++;
    return b;
  }
  __device__ __forceinline__ void flush() {
    if (threadIdx.x < q) out[qpos + threadIdx.x] = (uint8_t)my;
    qpos += q; q = 0;
  }
  // the wave's stores so far are complete before anything issued behind this is read: vmcnt (0), the other counters left alone
  __device__ __forceinline__ void settle() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    fence_pos = qpos;
  }
  __device__ __forceinline__ void put(uint32_t b) {
    if (threadIdx.x == q) my = b;
    if (++q == ULG_WAVE) flush();
  }
  // len bytes at pos (= every byte put so far) from dist behind; a source in front of the entry reads 0; dist < len repeats the dist bytes before pos
  __device__ __forceinline__ void copyz(uint64_t pos, uint64_t dist, uint32_t len) {
    flush();                                                    // qpos = pos
    const uint32_t lane = threadIdx.x;
    const uint32_t D = dist < len ? (uint32_t)dist : len;       // bytes of the source that exist before the copy: the period
    if (pos + D > dist && pos - dist + D > fence_pos) settle(); // (the source's end lies in the entry and beyond the bytes known complete)
    ulg_gu8 *dst = out + pos;
    for (uint32_t i = lane; i < len; i += ULG_WAVE) {
      const uint64_t s = pos + (dist < len ? i % D : i);        // the source's position + dist
      dst[i] = s < dist ? (uint8_t)0 : out[s - dist];
    }
    qpos = pos + len;
  }
};

}  // namespace zada
