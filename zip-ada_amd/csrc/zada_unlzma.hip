// zada_unlzma.hip -- UnZip.Decompress.LZMA_Decode (unzip-decompress.adb:1917-1940 over lzma-decoding.adb; Zip format 14) for a batch of entries:
// one wave per entry.
//
// One LZMA stream is one chain of adaptive probabilities: every bit is decoded from the probability the bits before it left.  What runs in
// parallel is the entries.  The chain (zada_unlzma_logic.h) is wave-uniform: every lane holds the same range, code, state and reps, and what is
// read from LDS or memory on its way moves to the scalar side with readfirstlane.  The 64 lanes add what lies around the chain:
//   - the compressed input comes into LDS in coalesced pieces of ULZ_STAGE bytes (INF_STAGE's scheme, zada_inflate.hip);
//   - literals wait in a queue, lane q holding literal q, and are stored 64 at a time (or in front of the next match);
//   - every match is copied by all lanes, dist < len being the periodic case; with it the wave fetches the two bytes the chain needs next --
//     the match's last byte (the next literal's context: the previous byte stays in a register) and the byte behind the source (the "match byte"
//     of a literal that follows) -- so that the chain makes no round trip of its own behind a match;
//   - the CRC-32 of the output is k_inf_crc's (zada_inflate.hip), through inflate_crc_entries.
// The window is the entry's own output in device memory, read through the pointer it is written through, with vector loads and stores only.
// A lane reads bytes that other lanes of its wave stored an instant ago: before a match (or a single byte) whose source reaches beyond the
// bytes known to be complete is read, the wave waits for its outstanding stores -- s_waitcnt vmcnt (0) between a workgroup-scope release /
// acquire fence pair, as in inf_expand -- that wait is what makes it hold.  No other workgroup reads an entry's output inside the launch.
//
// The probability model is 1846 + (0x300 << (lc + lp)) 16-bit values.  The 1846 are always in LDS.  The literal table (LM_LDS / LM_HBM as in
// zada_lzma.hip): lc + lp <= 3 -- 12 KiB at most -- in LDS (k_unlzma <LM_LDS>); lc + lp >= 4 -- the data-type methods, up to 6 MiB -- in HBM, one
// table per entry, filled with 1024 by the entry's wave and written by it alone (k_unlzma <LM_HBM>); the entries of a batch with such tables go
// in launch groups bounded by the knob "lzma_lit_mib".
// LDS per wave (= per workgroup of 64), LM_LDS: 3 692 + 12 288 + ULZ_STAGE (384) + 4 = 16 368 bytes, so 160 KiB of LDS hold TEN entries per CU
// (derived from the sizes, not measured; measured as entries x one entry's kernel time / the batch's kernel time for 10 000 LZMA_3 entries of
// 16 KiB: 6.2 entries per CU in flight on average over the launch, its tail included -- profiles/unlzma/NOTES.md).  LM_HBM: 4 080 bytes; its launches keep 16 waves per CU in flight.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <new>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_reader_host.h"
#include "zada_unlzma_logic.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {

constexpr uint32_t ULZ_WAVE = 64;
constexpr uint32_t ULZ_STAGE = 384;                  // bytes of compressed input in LDS at a time (a multiple of 4)
enum { ULM_LDS = 1, ULM_HBM = 2 };                   // (zada_lzma.hip's LM_LDS / LM_HBM)
struct UlzJob { uint64_t in, out, n_in, cap, lit, lit_elems; uint32_t eos, pad; };
typedef __attribute__((address_space(1))) uint8_t ulz_gu8;
typedef __attribute__((address_space(1))) const uint8_t ulz_gcu8;
typedef __attribute__((address_space(1))) const uint32_t ulz_gcu32;
typedef __attribute__((address_space(1))) uint16_t ulz_gu16;
typedef __attribute__((address_space(1))) uint32_t ulz_gu32;

#define ULZ_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))

// file-scope LDS objects: every access is a ds_ instruction
__shared__ uint16_t s_ulz_probs[ULZ_NPROBS];
__shared__ uint16_t s_ulz_lit[ULZ_LIT_LDS_MAX];       // (k_unlzma <ULM_LDS> only)
__shared__ uint32_t s_ulz_stage[ULZ_STAGE / 4];
__shared__ uint32_t s_ulz_next;

template <int LM> struct UlzWaveIO {
  ulz_gcu8 *in; uint64_t n, ip, base; bool over;
  ulz_gu8 *out; ulz_gu16 *lit;
  uint32_t q, my;                  // the literal queue: q literals, lane k holding literal k, go to qpos ..
  uint64_t qpos, fence_pos;        // fence_pos: every byte before it is known to be in memory for all lanes of the wave
  uint64_t c_pos, c_dist; uint32_t c_byte;      // the byte c_dist behind c_pos, fetched with the last match

  __device__ __forceinline__ void fill(uint64_t at) {                 // all lanes; at: multiple of 4.  Nothing is read beyond n.
    __syncthreads();
    base = at;
    const uint32_t lane = threadIdx.x;
    const bool al4 = (((uintptr_t)in) & 3u) == 0;
    for (uint32_t w = lane; w < ULZ_STAGE / 4; w += ULZ_WAVE) {
      const uint64_t o = at + (uint64_t)w * 4;
      uint32_t v = 0;
      if (o + 4 <= n) {
        if (al4) v = *(ulz_gcu32 *)(in + o);
        else v = (uint32_t)in[o] | (uint32_t)in[o + 1] << 8 | (uint32_t)in[o + 2] << 16 | (uint32_t)in[o + 3] << 24;
      } else {
        for (uint32_t k = 0; k < 4; k++) if (o + k < n) v |= (uint32_t)in[o + k] << (8 * k);
      }
      s_ulz_stage[w] = v;
    }
    __syncthreads();
  }
  __device__ __forceinline__ void open(ulz_gcu8 *p, uint64_t len, ulz_gu8 *o, ulz_gu16 *l) {
    in = p; n = len; ip = 0; over = false; out = o; lit = l; q = 0; my = 0; qpos = 0; fence_pos = 0; c_pos = ~0ull; c_dist = 0; c_byte = 0;
    fill(0);
  }
  __device__ __forceinline__ uint32_t staged(uint32_t o) const { return (ULZ_UNI(s_ulz_stage[o >> 2]) >> ((o & 3u) * 8u)) & 0xFFu; }
  __device__ __forceinline__ uint32_t byte() {
    if (ip >= n) { over = true; return 0; }
    if (ip >= base + ULZ_STAGE) fill(ip & ~3ull);
    const uint32_t b = staged((uint32_t)(ip - base));
    ip++;
    return b;
  }
  __device__ __forceinline__ uint32_t pget(uint32_t i) const { return ULZ_UNI(s_ulz_probs[i]); }
  __device__ __forceinline__ void pset(uint32_t i, uint32_t v) { s_ulz_probs[i] = (uint16_t)v; }
  // (the HBM table: every lane loads and stores the same address, so each lane reads what it wrote itself)
  __device__ __forceinline__ uint32_t lget(uint32_t i) const { if constexpr (LM == ULM_HBM) return ULZ_UNI(lit[i]); else return ULZ_UNI(s_ulz_lit[i]); }
  __device__ __forceinline__ void lset(uint32_t i, uint32_t v) { if constexpr (LM == ULM_HBM) lit[i] = (uint16_t)v; else s_ulz_lit[i] = (uint16_t)v; }

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
  __device__ __forceinline__ void put(uint64_t pos, uint32_t b) {
    if (threadIdx.x == q) my = b;
    if (++q == ULZ_WAVE) flush();
  }
  __device__ __forceinline__ uint32_t peek(uint64_t pos, uint64_t dist) {
    if (pos == c_pos && dist == c_dist) return c_byte;
    const uint64_t a = pos - dist;
    if (a >= qpos) flush();
    if (a >= fence_pos) settle();
    return ULZ_UNI(out[a]);
  }
  __device__ __forceinline__ uint32_t copy(uint64_t pos, uint64_t dist, uint32_t len) {
    flush();                                                    // qpos = pos
    const uint32_t lane = threadIdx.x;
    const uint32_t D = dist < len ? (uint32_t)dist : len;       // bytes of the source that exist before the match: the period
    // the source, and the byte behind it where it is an older byte (the match byte of a literal that follows)
    if (pos - dist + (dist > len ? len + 1 : D) > fence_pos) settle();
    ulz_gu8 *dst = out + pos;
    ulz_gu8 *src = out + (pos - dist);
    const uint32_t last = src[dist < len ? (len - 1) % (uint32_t)dist : len - 1];
    const uint32_t behind = src[dist <= len ? len % (uint32_t)dist : len];
    if (dist >= len) { for (uint32_t i = lane; i < len; i += ULZ_WAVE) dst[i] = src[i]; }
    else { for (uint32_t i = lane; i < len; i += ULZ_WAVE) dst[i] = src[i % D]; }      // the overlapping case: the D bytes before pos, over and over
    qpos = pos + len;
    c_pos = qpos; c_dist = dist; c_byte = ULZ_UNI(behind);
    return ULZ_UNI(last);
  }
};

template <int LM>
__global__ void __launch_bounds__(ULZ_WAVE) k_unlzma(const UlzJob *__restrict__ jobs, const uint32_t *__restrict__ order, uint32_t count, uint32_t *counter,
                                                     UlzResult *results) {
  const uint32_t lane = threadIdx.x;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_ulz_next = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t slot = ULZ_UNI(s_ulz_next);
    if (slot >= count) break;
    const uint32_t e = order[slot];
    const UlzJob J = jobs[e];
    UlzWaveIO<LM> io;
    io.open((ulz_gcu8 *)J.in, J.n_in, (ulz_gu8 *)J.out, (ulz_gu16 *)J.lit);
    uint8_t h9[9];
#pragma unroll
    for (uint32_t k = 0; k < 9; k++) h9[k] = (uint8_t)io.staged(k);           // (zeros beyond n_in)
    UlzResult R;
    UlzProps P{};
    uint32_t rule = ulz_props(h9, J.n_in, P);
    // the host sized the table from the same nine bytes; an entry whose table would not fit what it was given is refused, not run
    if (!rule && ulz_lit_elems(P) > (LM == ULM_HBM ? J.lit_elems : (uint64_t)ULZ_LIT_LDS_MAX)) rule = ULZ_R_PROPERTIES;
    if (rule) ulz_fail(R, rule, J.n_in < 9 ? J.n_in : 4, 0);
    else {
      for (uint32_t i = lane; i < ULZ_NPROBS; i += ULZ_WAVE) s_ulz_probs[i] = (uint16_t)ULZ_PROB_INIT;
      const uint32_t words = (uint32_t)(ulz_lit_elems(P) / 2);
      if constexpr (LM == ULM_HBM) { ulz_gu32 *l32 = (ulz_gu32 *)J.lit; for (uint32_t i = lane; i < words; i += ULZ_WAVE) l32[i] = ULZ_PROB_INIT * 0x10001u; }
      else { uint32_t *l32 = (uint32_t *)s_ulz_lit; for (uint32_t i = lane; i < words; i += ULZ_WAVE) l32[i] = ULZ_PROB_INIT * 0x10001u; }
      __syncthreads();
      if constexpr (LM == ULM_HBM) io.settle();                 // the table's words were stored by other lanes than those that read them
      io.ip = 9;
      ulz_decode(io, P, J.cap, J.eos, R);
      if (R.rc == 0) io.flush();
    }
    R.crc = 0;
    if (lane == 0) results[e] = R;
  }
}

// ---- Trained_Compression: the same wave, started from a snapshot or stopped into one ----
// A snapshot is the decoder between two symbols: ulz_decode_f's UlzFork, the stream's properties and the probability model (the literal table in the
// LDS only: lc + lp <= 3).  The window is not part of it: the text written so far lies in the output slot, where the caller puts a copy of it for
// every stream that starts from the snapshot.
struct UlzSnap { UlzFork f; UlzProps P; uint32_t valid, pad; uint16_t probs[ULZ_NPROBS + 2]; uint16_t lit[ULZ_LIT_LDS_MAX]; };
static_assert(sizeof(UlzSnap) % 4 == 0 && (ULZ_NPROBS + 2) % 2 == 0, "word copies");
__device__ __forceinline__ uint64_t ulz_uni64(uint64_t v) { return (uint64_t)ULZ_UNI((uint32_t)v) | (uint64_t)ULZ_UNI((uint32_t)(v >> 32)) << 32; }

template <bool STOP>
__global__ void __launch_bounds__(ULZ_WAVE) k_unlzma_trained(const UlzTrainedJob *__restrict__ jobs, const uint32_t *__restrict__ order, uint32_t count, uint32_t *counter,
                                                             UlzResult *results, const UlzSnap *start, UlzSnap *snap, uint64_t stop_in) {
  const uint32_t lane = threadIdx.x;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_ulz_next = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t slot = ULZ_UNI(s_ulz_next);
    if (slot >= count) break;
    const uint32_t e = order[slot];
    const UlzTrainedJob J = jobs[e];
    UlzWaveIO<ULM_LDS> io;
    io.open((ulz_gcu8 *)J.in, J.n_in, (ulz_gu8 *)J.out, nullptr);
    UlzResult R;
    UlzProps P{};
    UlzFork F{};
    uint32_t rule = ULZ_OK;
    if (start) {
      P = UlzProps{ULZ_UNI(start->P.lc), ULZ_UNI(start->P.lp), ULZ_UNI(start->P.pb), ULZ_UNI(start->P.dict)};
      F = UlzFork{ULZ_UNI(start->f.range), ULZ_UNI(start->f.code), ULZ_UNI(start->f.corrupted), ULZ_UNI(start->f.state), ULZ_UNI(start->f.rep0), ULZ_UNI(start->f.rep1),
                  ULZ_UNI(start->f.rep2), ULZ_UNI(start->f.rep3), ULZ_UNI(start->f.prev), 0u, 0ull, ulz_uni64(start->f.out_pos)};
      const uint32_t *l32 = (const uint32_t *)start->lit;
      const uint32_t words = (uint32_t)(ulz_lit_elems(P) / 2);                  // (<= ULZ_LIT_LDS_MAX / 2: unlzma_trained_launch's caller saw to it)
      for (uint32_t i = lane; i < ULZ_NPROBS; i += ULZ_WAVE) s_ulz_probs[i] = start->probs[i];
      for (uint32_t i = lane; i < words && i < ULZ_LIT_LDS_MAX / 2; i += ULZ_WAVE) ((uint32_t *)s_ulz_lit)[i] = l32[i];
      __syncthreads();
      io.qpos = F.out_pos; io.fence_pos = F.out_pos;                            // (the text before: written by the launch before this one)
    } else {
      uint8_t h5[5];
#pragma unroll
      for (uint32_t k = 0; k < 5; k++) h5[k] = (uint8_t)io.staged(k);           // (zeros beyond n_in)
      rule = ulz_props5(h5, J.n_in, P);
      if (!rule && ulz_lit_elems(P) > (uint64_t)ULZ_LIT_LDS_MAX) rule = ULZ_R_PROPERTIES;
      if (!rule) {
        for (uint32_t i = lane; i < ULZ_NPROBS; i += ULZ_WAVE) s_ulz_probs[i] = (uint16_t)ULZ_PROB_INIT;
        const uint32_t words = (uint32_t)(ulz_lit_elems(P) / 2);
        uint32_t *l32 = (uint32_t *)s_ulz_lit;
        for (uint32_t i = lane; i < words; i += ULZ_WAVE) l32[i] = ULZ_PROB_INIT * 0x10001u;
        __syncthreads();
        io.ip = 5;
      }
    }
    if (rule) ulz_fail(R, rule, J.n_in < 5 ? J.n_in : 0, 0);
    else {
      const UlzStop stp{stop_in, ~0ull};
      ulz_decode_f<true>(io, P, J.cap, 1u, R, start ? &F : nullptr, STOP ? &stp : nullptr, &F);
      if (R.rc == 0) io.flush();
      if constexpr (STOP) {
        if (R.rc == 0 && R.end == ULZ_END_FORK) {
          __syncthreads();
          uint32_t *l32 = (uint32_t *)snap->lit;
          for (uint32_t i = lane; i < ULZ_NPROBS; i += ULZ_WAVE) snap->probs[i] = s_ulz_probs[i];
          for (uint32_t i = lane; i < ULZ_LIT_LDS_MAX / 2; i += ULZ_WAVE) l32[i] = ((const uint32_t *)s_ulz_lit)[i];
          if (lane == 0) { snap->f = F; snap->P = P; snap->valid = 1u; snap->pad = 0u; }
        }
      }
    }
    R.crc = 0;
    if (lane == 0) results[e] = R;
  }
}

// ---- host side ----
struct UlzState : ReaderState {                       // (d_counter: one per launch of a call)
  DevBuf lit;                                          // the HBM literal tables of a launch group
  int cus = 0;
};
constexpr uint32_t ULZ_MAX_LAUNCHES = 4096;

static UlzState *ulz_state(Ctx *c) {
  if (c->ulz) return (UlzState *)c->ulz;
  UlzState *S = new (std::nothrow) UlzState();
  if (!S) return nullptr;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c->device) != hipSuccess || hipMalloc((void **)&S->d_counter, ULZ_MAX_LAUNCHES * 4) != hipSuccess) {
    (void)hipGetLastError();
    delete S;
    return nullptr;
  }
  S->cus = prop.multiProcessorCount;
  c->ulz = S;
  return S;
}
void unlzma_destroy(Ctx *c) {
  UlzState *S = (UlzState *)c->ulz;
  if (!S) return;
  dev_free(S->tabs); dev_free(S->arena); dev_free(S->lit);
  hipFree(S->d_counter);
  delete S;
  c->ulz = nullptr;
}

// the literal table an entry needs in HBM, in probabilities (0: it fits the LDS, or the header is refused anyway), from its first nine bytes
static uint64_t ulz_hbm_elems(const uint8_t *h9, uint64_t n_in) {
  UlzProps P{};
  if (ulz_props(h9, n_in, P)) return 0;
  const uint64_t n = ulz_lit_elems(P);
  return n > ULZ_LIT_LDS_MAX ? n : 0;
}

// E jobs (device addresses; lit_elems from ulz_hbm_elems) through the launches of k_unlzma and one of k_inf_crc; res [E] receives the records
static int ulz_run(Ctx *c, UlzState *S, std::vector<UlzJob> &jobs, const uint32_t *crc_in, std::vector<UlzResult> &res) {
  const uint32_t E = (uint32_t)jobs.size();
  res.resize(E);
  if (E == 0) return 0;
  // the launches: the entries with their table in LDS, then the others in groups of up to "lzma_lit_mib" of tables; each longest first
  std::vector<uint32_t> order, hbm;
  std::vector<uint32_t> l_begin, l_count, l_mode;
  for (uint32_t i = 0; i < E; i++) (jobs[i].lit_elems ? hbm : order).push_back(i);
  auto longest_first = [&](uint32_t a, uint32_t b) { return jobs[a].n_in > jobs[b].n_in; };
  std::stable_sort(order.begin(), order.end(), longest_first);
  if (!order.empty()) { l_begin.push_back(0); l_count.push_back((uint32_t)order.size()); l_mode.push_back(ULM_LDS); }
  const uint64_t lit_cap = (uint64_t)c->knob_lzma_lit_mib << 20;
  uint64_t lit_max = 0;
  for (size_t k = 0; k < hbm.size();) {
    uint64_t bytes = 0;
    size_t k1 = k;
    while (k1 < hbm.size()) {
      const uint64_t b = jobs[hbm[k1]].lit_elems * 2;
      if (k1 > k && bytes + b > lit_cap) break;
      jobs[hbm[k1]].lit = bytes;                                   // (offset for now)
      bytes += b; k1++;
    }
    l_begin.push_back((uint32_t)order.size()); l_count.push_back((uint32_t)(k1 - k)); l_mode.push_back(ULM_HBM);
    for (size_t j = k; j < k1; j++) order.push_back(hbm[j]);
    std::stable_sort(order.end() - (k1 - k), order.end(), longest_first);
    if (bytes > lit_max) lit_max = bytes;
    k = k1;
  }
  if (l_begin.size() > ULZ_MAX_LAUNCHES) { c->err = "unlzma: more launch groups than 4096: raise the knob lzma_lit_mib"; return ZADA_E_INVALID; }
  int rc = 0;
  if (lit_max) {
    rc = dev_grow(c, S->lit, lit_max, "hipMalloc (unlzma literal tables)");
    if (rc) return rc;
    for (uint32_t i : hbm) jobs[i].lit += (uint64_t)(uintptr_t)S->lit.p;
  }
  ReaderTables<UlzJob, UlzResult> T;
  rc = reader_tables_send(c, S, "unlzma", jobs, order, nullptr, (uint32_t)l_begin.size(), T);
  if (rc) return rc;
  hipStream_t st = c->stream;
  c->tmark("unlzma:begin");
  for (size_t l = 0; l < l_begin.size(); l++) {
    const uint32_t n = l_count[l];
    const uint32_t waves = (uint32_t)S->cus * (l_mode[l] == ULM_LDS ? 10u : 16u);
    const uint32_t grid = n < waves ? n : waves;
    if (l_mode[l] == ULM_LDS) hipLaunchKernelGGL(k_unlzma<ULM_LDS>, dim3(grid), dim3(ULZ_WAVE), 0, st, T.jobs, T.order + l_begin[l], n, S->d_counter + l, T.res);
    else hipLaunchKernelGGL(k_unlzma<ULM_HBM>, dim3(grid), dim3(ULZ_WAVE), 0, st, T.jobs, T.order + l_begin[l], n, S->d_counter + l, T.res);
  }
  c->tmark("unlzma:k_unlzma");
  rc = reader_tables_fetch(c, "unlzma", T, res);
  if (rc) return rc;
  // the entries' Zip CRC-32 (k_inf_crc)
  std::vector<uint64_t> optr(E), olen(E);
  std::vector<uint32_t> regs(E);
  for (uint32_t i = 0; i < E; i++) { optr[i] = jobs[i].out; olen[i] = res[i].rc == 0 ? res[i].out_len : 0; regs[i] = crc_in ? crc_in[i] : 0u; }
  rc = inflate_crc_entries(c, E, optr.data(), olen.data(), regs.data());
  if (rc) return rc;
  c->tmark("unlzma:k_inf_crc");
  for (uint32_t i = 0; i < E; i++) {
    res[i].crc = regs[i];
    for (uint64_t v : {(uint64_t)res[i].rule, res[i].in_pos, res[i].out_pos, (uint64_t)res[i].end}) S->last_entries.push_back(v);
  }
  return 0;
}

static void ulz_describe(Ctx *c, const UlzResult &R, int entry) {
  char buf[240];
  snprintf(buf, sizeof buf, "unlzma: entry %d: %s at input byte %llu", entry, ulz_rule_name(R.rule), (unsigned long long)R.in_pos);
  c->err = buf;
}

struct UlzReader : ReaderTraits<UlzJob, UlzResult, UlzState> {
  static constexpr const char *word = "unlzma";
  static UlzState *state(Ctx *c) { return ulz_state(c); }
  static int run(Ctx *c, UlzState *S, std::vector<UlzJob> &jobs, const uint32_t *crc_in, std::vector<UlzResult> &res, uint32_t) { return ulz_run(c, S, jobs, crc_in, res); }
  static void describe(Ctx *c, const UlzResult &R, int entry) { ulz_describe(c, R, entry); }
};

// ulz_run for zada_unzip_device (zada_internal.h)
uint64_t unlzma_hbm_elems(const uint8_t *h9, uint64_t n_in) { return ulz_hbm_elems(h9, n_in); }
int unlzma_run_jobs(Ctx *c, uint32_t E, const ReaderJob *rj, ReaderRes *rr, bool *described) {
  return reader_run_jobs<UlzReader>(c, E, rj, rr, described, [](const ReaderJob &J) { return UlzJob{J.in, J.out, J.n_in, J.cap, 0, J.lit_elems, J.eos ? 1u : 0u, 0}; });
}

// k_unlzma_trained for zada_trained.hip (zada_internal.h)
uint64_t unlzma_snap_bytes() { return sizeof(UlzSnap); }
int unlzma_snap_info(const uint8_t *snap, uint64_t *in_pos, uint64_t *out_pos, uint64_t *lit_elems) {
  const UlzSnap *S = (const UlzSnap *)snap;
  if (S->valid != 1u) return 0;
  *in_pos = S->f.in_pos; *out_pos = S->f.out_pos; *lit_elems = ulz_lit_elems(S->P);
  return 1;
}
int unlzma_trained_launch(Ctx *c, const UlzTrainedJob *d_jobs, const uint32_t *d_order, uint32_t E, UlzResult *d_res, const void *d_start, void *d_stop, uint64_t stop_in) {
  if (E == 0) return 0;
  if (d_stop && (E != 1 || d_start)) { c->err = "unlzma: one stream from its header stops into a snapshot"; return ZADA_E_INVALID; }
  UlzState *S = ulz_state(c);
  if (!S) { c->err = "unlzma: no memory for the tables"; return ZADA_E_NOMEM; }
  hipStream_t st = c->stream;
  hipMemsetAsync(S->d_counter, 0, 4, st);
  const uint32_t waves = (uint32_t)S->cus * 10u;
  const uint32_t grid = E < waves ? E : waves;
  if (d_stop) hipLaunchKernelGGL(k_unlzma_trained<true>, dim3(grid), dim3(ULZ_WAVE), 0, st, d_jobs, d_order, E, S->d_counter, d_res, (const UlzSnap *)nullptr, (UlzSnap *)d_stop, stop_in);
  else hipLaunchKernelGGL(k_unlzma_trained<false>, dim3(grid), dim3(ULZ_WAVE), 0, st, d_jobs, d_order, E, S->d_counter, d_res, (const UlzSnap *)d_start, (UlzSnap *)nullptr, 0ull);
  return hip_check(c, hipGetLastError(), "k_unlzma_trained") ? ZADA_E_HIP : 0;
}

}  // namespace zada

using namespace zada;

static constexpr uint64_t ULZ_MAX_BYTES = 1ull << 40;      // (as Inflate: a stream or an output of 1 TiB and more is beyond any device)

int zada_unlzma_device(zada_ctx *z, const void *d_in, uint64_t n_in, void *d_out, uint64_t cap, int eos, uint64_t *out_len, uint64_t *in_used, uint32_t *crc_inout) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if ((n_in && !d_in) || (cap && !d_out)) { c->err = "zada_unlzma_device: null buffer"; return ZADA_E_INVALID; }
  if (n_in >= ULZ_MAX_BYTES || cap >= ULZ_MAX_BYTES) { c->err = "zada_unlzma_device: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  return reader_device_one<UlzReader>(c, out_len, in_used, crc_inout, [&](UlzJob &J) {
    uint8_t h9[9] = {0};
    if (n_in && hip_check(c, hipMemcpy(h9, d_in, n_in < 9 ? n_in : 9, hipMemcpyDeviceToHost), "unlzma header")) return (int)ZADA_E_HIP;
    J = UlzJob{(uint64_t)(uintptr_t)d_in, (uint64_t)(uintptr_t)d_out, n_in, cap, 0, ulz_hbm_elems(h9, n_in), eos ? 1u : 0u, 0};
    return 0;
  });
}

int zada_unlzma_batch(zada_ctx *z, int count, const uint8_t *const *in, const uint64_t *n_in, uint8_t *const *out, const uint64_t *cap, const int *eos,
                      uint64_t *out_len, uint64_t *in_used, uint32_t *crc, int *rc_out) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (count && (!in || !n_in || !cap || !eos || !rc_out)) { c->err = "zada_unlzma_batch: null argument"; return ZADA_E_INVALID; }
  for (int i = 0; i < count; i++) {
    if ((n_in[i] && !in[i]) || (out && cap[i] && !out[i])) { c->err = "zada_unlzma_batch: null buffer"; return ZADA_E_INVALID; }
    if (n_in[i] >= ULZ_MAX_BYTES || cap[i] >= ULZ_MAX_BYTES) { c->err = "zada_unlzma_batch: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  }
  if (count == 0) return ZADA_OK;
  return reader_batch<UlzReader>(c, count, in, n_in, out, cap, out_len, in_used, crc, rc_out, [&](int i, uint64_t d_in, uint64_t d_out) {
    uint8_t h9[9] = {0};
    if (n_in[i]) memcpy(h9, in[i], n_in[i] < 9 ? n_in[i] : 9);
    return UlzJob{d_in, d_out, n_in[i], cap[i], 0, ulz_hbm_elems(h9, n_in[i]), eos[i] ? 1u : 0u, 0};
  });
}

int zada_unlzma(zada_ctx *z, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, int eos, uint64_t *out_len, uint64_t *in_used, uint32_t *crc_inout) {
  if (!z) return ZADA_E_INVALID;
  z->c.lz_stopped = false;
  if ((n_in && !in) || (cap && !out)) { z->c.err = "zada_unlzma: null buffer"; return ZADA_E_INVALID; }
  return reader_single(out_len, in_used, crc_inout, [&](uint64_t *ol, uint64_t *iu, uint32_t *reg, int *erc) {
    return zada_unlzma_batch(z, 1, &in, &n_in, &out, &cap, &eos, ol, iu, reg, erc);
  });
}

uint64_t zada_unlzma_last_records(zada_ctx *z, uint64_t *dst, uint64_t cap_items) {
  if (!z || !z->c.ulz || (cap_items && !dst)) return 0;
  return reader_last_records(((const UlzState *)z->c.ulz)->last_entries, dst, cap_items);
}
