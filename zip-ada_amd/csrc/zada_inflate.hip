// zada_inflate.hip -- UnZip.Decompress.Inflate (unzip-decompress.adb:1463-1889) for a batch of entries: one wave per entry.
//
// One stream is a chain: a Huffman code is found only by decoding the one before it, a match reads what earlier tokens wrote.  What runs in
// parallel is the entries -- and, inside one entry, the writing: the wave decodes tokens with every lane in step (zada_inflate_logic.h, each
// decision wave-uniform and moved to the scalar side with readfirstlane), lane q keeps token q, and after 64 tokens the wave expands the
// queue: a prefix sum of the tokens' lengths, literals one lane per byte, every match copied by all lanes.  The window is the entry's own
// output in device memory.  A lane reads bytes that other lanes of its wave stored an instant ago, so a match whose source reaches beyond
// the bytes known to be complete passes a workgroup-scope release / acquire fence pair and an explicit wait on the wave's outstanding stores
// first (see inf_expand); matches that read older bytes -- most of them -- do not wait.  No other workgroup reads an entry's output inside the launch.
// The output is read through the same non-const, non-restrict pointer it is written through, with per-lane addresses: vector loads only.
//
// LDS per wave (= per workgroup of 64): the code tables (InfTables, 3.7 KiB) and INF_STAGE bytes of compressed input, staged in coalesced pieces.
// Entries are handed out through a counter in the order the host sorted them in, longest first.
// k_inf_crc: the CRC-32 of every entry's output, one wave per entry -- the per-entry variant of k_crc_chunks / k_crc_fold: raw registers of
// 256-byte pieces, a wave scan with the "advance over 256 << j zero bytes" operators, strip after strip.
// k_crypt_decode: CRC_Crypto.Decode (zip-crc_crypto.adb:130-137), one LANE per entry: key 0 is a CRC over the plaintext, which is known only
// byte by byte, so unlike Encode there is no scan to find.
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
#include "zada_inflate_logic.h"
#include "zada_inflate_wave.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {

struct InfJob { uint64_t in, out, n_in, cap; int32_t format, pad; };

__global__ void __launch_bounds__(INF_WAVE) k_inflate(const InfJob *__restrict__ jobs, const uint32_t *__restrict__ order, uint32_t count,
                                                      uint32_t *counter, InfResult *results) {
  __shared__ InfTables T;
  __shared__ uint32_t stage[INF_STAGE / 4 + 2];
  __shared__ uint32_t next_s;
  const uint32_t lane = threadIdx.x;
  for (;;) {
    __syncthreads();
    if (lane == 0) next_s = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t slot = ZINF_UNI(next_s);
    if (slot >= count) break;
    const uint32_t e = order[slot];
    const InfJob J = jobs[e];
    gcu8 *in = (gcu8 *)J.in;
    gu8 *out = (gu8 *)J.out;
    const uint64_t n_in = J.n_in, cap = J.cap;
    const bool d64 = J.format == 9;
    uint32_t rule = INF_OK;
    uint64_t pos = 0, fence_pos = 0, fail_bits = 0, in_used = 0;
    if (n_in == 0) rule = INF_R_EMPTY_INPUT;
    else {
      InfWaveReader br;
      br.open(in, n_in, 0, stage);
      int loaded = INF_TAB_NONE;
      uint32_t q = 0, my_len = 0, my_dist = 0, my_val = 0;
      uint64_t qpos = 0;                                         // where the queue's first token goes; pos: behind its last
      for (;;) {
        br.need32();
        const uint32_t hdr = (uint32_t)br.hold & 7u;
        br.drop(3);
        if (br.overrun()) { rule = INF_R_TRUNCATED; break; }
        const uint32_t type = hdr >> 1;
        if (type == 3) { rule = INF_R_BLOCK_TYPE; break; }
        if (type == 0) {
          uint64_t at = (br.used_bits() + 7) / 8;
          if (at + 4 > n_in) { rule = INF_R_TRUNCATED; break; }
          // LEN, NLEN: at most 3 bytes of the bit register are dropped, so both words are among the 32 bits a refill at `at` gives
          br.hold = 0; br.nb = 0; br.ip = at;
          br.need32();
          const uint32_t w = (uint32_t)br.hold;
          const uint32_t len = w & 0xFFFFu, nlen = w >> 16;
          if (len != (nlen ^ 0xFFFFu)) { rule = INF_R_STORED_LEN; break; }
          at += 4;
          if (pos + len > cap) { rule = INF_R_OUTPUT_FULL; break; }
          if (at + len > n_in) { rule = INF_R_TRUNCATED; break; }
          inf_expand(out, qpos, q, my_len, my_dist, my_val, fence_pos);
          q = 0; my_len = 0;
          gcu8 *s = in + at;
          gu8 *d = out + pos;
          uint32_t head = (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u);
          if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0 && len >= 64u) {           // 16 bytes at a time where both sides align
            if (lane < head) d[lane] = s[lane];
            const uint32_t words = (len - head) / 16u;
            gcu4 *s4 = (gcu4 *)(s + head);
            gu4 *d4 = (gu4 *)(d + head);
            for (uint32_t i = lane; i < words; i += INF_WAVE) d4[i] = s4[i];
            for (uint32_t i = head + words * 16u + lane; i < len; i += INF_WAVE) d[i] = s[i];
          } else {
            for (uint32_t i = lane; i < len; i += INF_WAVE) d[i] = s[i];
          }
          pos += len; qpos = pos;
          br.open(in, n_in, at + len, stage);
        } else {
          if (type == 1) {
            if (loaded != INF_TAB_FIXED) {
              inf_fixed_lengths(T, lane, INF_WAVE);
              inf_build(T, INF_T_LIT, T.lens, INF_NLIT, lane, INF_WAVE);
              inf_build(T, INF_T_DIST, T.lens + INF_NLIT, INF_NDIST, lane, INF_WAVE);
            }
            loaded = INF_TAB_FIXED;
          } else {
            loaded = INF_TAB_DYNAMIC;
            rule = inf_dynamic_header(br, T, d64, lane, INF_WAVE);
            if (rule) break;
          }
          for (;;) {
            uint32_t a = 0, b = 0;
            const int32_t k = inf_token(br, T, d64, a, b);
            if (k < 0) { rule = (uint32_t)-k; break; }
            if (br.overrun()) { rule = INF_R_TRUNCATED; break; }
            if (k == 2) break;
            uint32_t len = 1;
            if (k == 1) {
              if (b > pos) { rule = INF_R_DISTANCE_TOO_FAR; break; }
              len = a;
            } else b = 0;
            if (pos + len > cap) { rule = INF_R_OUTPUT_FULL; break; }
            if (lane == q) { my_len = len; my_dist = b; my_val = a; }
            pos += len;
            if (++q == INF_WAVE) {
              inf_expand(out, qpos, q, my_len, my_dist, my_val, fence_pos);
              q = 0; my_len = 0; qpos = pos;
            }
          }
          if (rule) break;
        }
        if (hdr & 1u) break;
      }
      if (!rule) { inf_expand(out, qpos, q, my_len, my_dist, my_val, fence_pos); in_used = (br.used_bits() + 7) / 8; }
      fail_bits = br.used_bits();
    }
    if (lane == 0) {
      InfResult R;
      R.rc = rule ? INF_E_DATA : 0; R.rule = rule; R.out_len = rule ? 0 : pos; R.in_used = rule ? 0 : in_used; R.bitpos = fail_bits; R.crc = 0; R.pad = 0;
      results[e] = R;
    }
  }
}

// ---- CRC-32 of every entry's output ----
constexpr uint32_t IC_SUB = 256, IC_ROW = IC_SUB + 16, IC_TILE = INF_WAVE * IC_SUB;
struct InfCrcOps { uint32_t mat[6][32]; };             // operator j: the register over 256 << j zero bytes

__device__ __forceinline__ uint32_t ic_gf2(const uint32_t *m, uint32_t v) {
  uint32_t s = 0;
#pragma unroll
  for (int b = 0; b < 32; b++) s ^= (0u - ((v >> b) & 1u)) & m[b];
  return s;
}
__device__ __forceinline__ uint32_t ic_bytes(const uint8_t *row, uint32_t len, const uint32_t *tab, uint32_t r) {
  for (uint32_t i = 0; i < len; i++) r = tab[(r ^ row[i]) & 0xFF] ^ (r >> 8);
  return r;
}

__global__ void __launch_bounds__(INF_WAVE) k_inf_crc(const InfJob *__restrict__ jobs, InfResult *results, const uint32_t *__restrict__ crc_in,
                                                      const InfCrcOps *__restrict__ ops, uint32_t count) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t m[6][32];
  __shared__ __attribute__((aligned(16))) uint8_t rows[INF_WAVE * IC_ROW];
  const uint32_t e = blockIdx.x, lane = threadIdx.x;
  if (e >= count) return;
  for (uint32_t t = lane; t < 256; t += INF_WAVE) {
    uint32_t l = t;
    for (int b = 0; b < 8; b++) l = (l & 1) ? (l >> 1) ^ 0xEDB88320u : l >> 1;      // Prepare_table, zip-crc_crypto.adb:31-47
    tab[t] = l;
  }
  for (uint32_t t = lane; t < 6 * 32; t += INF_WAVE) m[t >> 5][t & 31] = ops->mat[t >> 5][t & 31];
  const uint64_t n = results[e].rc == 0 ? results[e].out_len : 0;
  const uint8_t *buf = (const uint8_t *)jobs[e].out;
  const bool al16 = (((uintptr_t)buf) & 15u) == 0;
  uint32_t reg = crc_in[e];
  for (uint64_t s0 = 0; s0 < n; s0 += IC_TILE) {
    const uint32_t left = n - s0 < IC_TILE ? (uint32_t)(n - s0) : IC_TILE;
    __syncthreads();
    if (al16) {
      const uint4 *s = (const uint4 *)(buf + s0);
      const uint32_t words = left / 16;
      for (uint32_t wq = lane; wq < words; wq += INF_WAVE) *(uint4 *)(rows + (wq >> 4) * IC_ROW + (wq & 15) * 16) = s[wq];
      if (lane < (left & 15)) { const uint32_t o = words * 16 + lane; rows[(o / IC_SUB) * IC_ROW + (o % IC_SUB)] = buf[s0 + o]; }
    } else {
      for (uint32_t o = lane; o < left; o += INF_WAVE) rows[(o / IC_SUB) * IC_ROW + (o % IC_SUB)] = buf[s0 + o];
    }
    __syncthreads();
    const uint32_t o = lane * IC_SUB;
    const uint32_t len = o >= left ? 0u : left - o < IC_SUB ? left - o : IC_SUB;
    const uint8_t *row = rows + lane * IC_ROW;
    // raw register of the lane's piece, then the register at the START of every piece: a scan seeded with the register before the strip
    // (every piece before the strip's last one is full, so one operator per distance serves)
    uint32_t v = ic_bytes(row, len, tab, 0u);
    if (lane == 0) v ^= ic_gf2(m[0], reg);
    for (int j = 0; j < 6; j++) {
      const uint32_t u = __shfl_up(v, 1u << j, 64);
      if (lane >= (1u << j)) v ^= ic_gf2(m[j], u);
    }
    uint32_t before = __shfl_up(v, 1u, 64);
    if (lane == 0) before = reg;
    // the lane of the strip's last byte runs its piece again from its true start: the register behind the strip
    const uint32_t last = (left - 1) / IC_SUB;
    uint32_t after = 0;
    if (lane == last) after = ic_bytes(row, len, tab, before);
    reg = (uint32_t)__shfl((int)after, (int)last, 64);
  }
  if (lane == 0) results[e].crc = reg;
}

// ---- CRC_Crypto.Decode, one lane per entry ----
__global__ void __launch_bounds__(INF_WAVE) k_crypt_decode(const uint64_t *__restrict__ ptrs, const uint64_t *__restrict__ lens, uint32_t *keys, uint32_t count) {
  __shared__ uint32_t tab[256];
  for (uint32_t t = threadIdx.x; t < 256; t += INF_WAVE) {
    uint32_t l = t;
    for (int b = 0; b < 8; b++) l = (l & 1) ? (l >> 1) ^ 0xEDB88320u : l >> 1;
    tab[t] = l;
  }
  __syncthreads();
  const uint32_t e = blockIdx.x * INF_WAVE + threadIdx.x;
  if (e >= count) return;
  uint8_t *buf = (uint8_t *)ptrs[e];
  const uint64_t n = lens[e];
  uint32_t k0 = keys[3 * e], k1 = keys[3 * e + 1], k2 = keys[3 * e + 2];
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t t = (k2 & 0xFFFFu) | 2u;                                  // Crypto_code :102-108
    const uint32_t p = (buf[i] ^ ((t * (t ^ 1u)) >> 8)) & 0xFFu;             // Decode :130-137
    k0 = tab[(k0 ^ p) & 0xFF] ^ (k0 >> 8);                                   // Update_keys :90-99, with the PLAIN byte
    k1 = (k1 + (k0 & 0xFFu)) * 134775813u + 1u;
    k2 = tab[(k2 ^ (k1 >> 24)) & 0xFF] ^ (k2 >> 8);
    buf[i] = (uint8_t)p;
  }
  keys[3 * e] = k0; keys[3 * e + 1] = k1; keys[3 * e + 2] = k2;
}

// ---- host side ----
struct InfState : ReaderState {
  InfCrcOps *d_ops = nullptr;
  int waves = 0;                                       // waves a launch keeps in flight
};

static InfState *inf_state(Ctx *c) {
  if (c->inf) return (InfState *)c->inf;
  InfState *S = new (std::nothrow) InfState();
  if (!S) return nullptr;
  InfCrcOps h;
  {
    uint32_t tab[256], op[32], sq[32];
    for (uint32_t t = 0; t < 256; t++) { uint32_t l = t; for (int b = 0; b < 8; b++) l = (l & 1) ? (l >> 1) ^ 0xEDB88320u : l >> 1; tab[t] = l; }
    for (int i = 0; i < 32; i++) { uint32_t r = 1u << i; r = tab[r & 0xFF] ^ (r >> 8); op[i] = r; }                 // one zero byte
    auto square = [&] { for (int i = 0; i < 32; i++) { uint32_t v = op[i], s = 0; for (int j = 0; v; j++, v >>= 1) if (v & 1) s ^= op[j]; sq[i] = s; } memcpy(op, sq, sizeof op); };
    for (int k = 0; k < 8; k++) square();                                                                            // 256 bytes
    for (int j = 0; j < 6; j++) { memcpy(h.mat[j], op, sizeof op); square(); }
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) { (void)hipGetLastError(); delete S; return nullptr; }
  S->waves = prop.multiProcessorCount * 24;
  if (hipMalloc((void **)&S->d_ops, sizeof(InfCrcOps)) != hipSuccess || hipMalloc((void **)&S->d_counter, 64) != hipSuccess ||
      hipMemcpy(S->d_ops, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (S->d_ops) hipFree(S->d_ops);
    if (S->d_counter) hipFree(S->d_counter);
    delete S;
    return nullptr;
  }
  c->inf = S;
  return S;
}
void inflate_destroy(Ctx *c) {
  InfState *S = (InfState *)c->inf;
  if (!S) return;
  dev_free(S->tabs); dev_free(S->arena);
  hipFree(S->d_ops); hipFree(S->d_counter);
  delete S;
  c->inf = nullptr;
}

// E jobs (device addresses) through one launch of k_inflate and one of k_inf_crc; res [E] receives the records
static int inf_run(Ctx *c, InfState *S, const std::vector<InfJob> &jobs, const uint32_t *crc_in, std::vector<InfResult> &res) {
  const uint32_t E = (uint32_t)jobs.size();
  res.resize(E);
  if (E == 0) return 0;
  std::vector<uint32_t> order(E);
  for (uint32_t i = 0; i < E; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].n_in > jobs[b].n_in; });      // longest first
  ReaderTables<InfJob, InfResult> T;
  const int rc = reader_tables_send(c, S, "inflate", jobs, order, crc_in, 1, T);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const uint32_t grid = E < (uint32_t)S->waves ? E : (uint32_t)S->waves;
  c->tmark("inflate:begin");
  hipLaunchKernelGGL(k_inflate, dim3(grid), dim3(INF_WAVE), 0, st, T.jobs, T.order, E, S->d_counter, T.res);
  c->tmark("inflate:k_inflate");
  hipLaunchKernelGGL(k_inf_crc, dim3(E), dim3(INF_WAVE), 0, st, T.jobs, T.res, T.crc, (const InfCrcOps *)S->d_ops, E);
  c->tmark("inflate:k_inf_crc");
  return reader_tables_fetch(c, "inflate", T, res);
}

// The Zip CRC-32 of E outputs in device memory through k_inf_crc, for the BZip2 reader (zada_bunzip2.hip): regs [i] is the register before
// entry i's out_len [i] bytes at out [i] on entry, the one behind them on return.
int inflate_crc_entries(Ctx *c, uint32_t E, const uint64_t *out, const uint64_t *out_len, uint32_t *regs) {
  if (E == 0) return 0;
  InfState *S = inf_state(c);
  if (!S) { c->err = "inflate: no memory for the tables"; return ZADA_E_NOMEM; }
  std::vector<InfJob> jobs(E);
  std::vector<InfResult> res(E);
  for (uint32_t i = 0; i < E; i++) {
    jobs[i] = InfJob{0, out[i], 0, out_len[i], 8, 0};
    res[i] = InfResult{0, 0, out_len[i], 0, 0, 0, 0};
  }
  const uint64_t o_jobs = 0, o_crc = o_jobs + (uint64_t)E * sizeof(InfJob), o_res = (o_crc + (uint64_t)E * 4 + 15) & ~15ull, total = o_res + (uint64_t)E * sizeof(InfResult);
  int rc = dev_grow(c, S->tabs, total, "hipMalloc (inflate tables)");
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipMemcpyAsync(S->tabs.p + o_jobs, jobs.data(), (size_t)E * sizeof(InfJob), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(S->tabs.p + o_crc, regs, (size_t)E * 4, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(S->tabs.p + o_res, res.data(), (size_t)E * sizeof(InfResult), hipMemcpyHostToDevice, st);
  hipLaunchKernelGGL(k_inf_crc, dim3(E), dim3(INF_WAVE), 0, st, (const InfJob *)(S->tabs.p + o_jobs), (InfResult *)(S->tabs.p + o_res), (const uint32_t *)(S->tabs.p + o_crc),
                     (const InfCrcOps *)S->d_ops, E);
  hipMemcpyAsync(res.data(), S->tabs.p + o_res, (size_t)E * sizeof(InfResult), hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipGetLastError(), "crc launch") || hip_check(c, hipStreamSynchronize(st), "crc")) return ZADA_E_HIP_;
  for (uint32_t i = 0; i < E; i++) regs[i] = res[i].crc;
  return 0;
}

static void inf_describe(Ctx *c, const InfResult &R, int entry) {
  char buf[200];
  snprintf(buf, sizeof buf, "inflate: entry %d: %s at bit %llu", entry, inf_rule_name(R.rule), (unsigned long long)R.bitpos);
  c->err = buf;
}

struct InfReader : ReaderTraits<InfJob, InfResult, InfState> {
  static constexpr const char *word = "inflate";
  static InfState *state(Ctx *c) { return inf_state(c); }
  static int run(Ctx *c, InfState *S, std::vector<InfJob> &jobs, const uint32_t *crc_in, std::vector<InfResult> &res, uint32_t) { return inf_run(c, S, jobs, crc_in, res); }
  static void describe(Ctx *c, const InfResult &R, int entry) { inf_describe(c, R, entry); }
};

// inf_run for zada_unzip_device (zada_internal.h)
int inflate_run_jobs(Ctx *c, uint32_t E, const ReaderJob *rj, ReaderRes *rr, bool *described) {
  return reader_run_jobs<InfReader>(c, E, rj, rr, described, [](const ReaderJob &J) { return InfJob{J.in, J.out, J.n_in, J.cap, J.format, 0}; });
}

}  // namespace zada

using namespace zada;

// a stream or an output of 1 TiB and more is beyond any device (and keeps the sums of a group's slots far from 2 ** 64, whatever a directory claims)
static constexpr uint64_t INF_MAX_BYTES = 1ull << 40;

static int inf_prepare(zada_ctx *z, int format, const char *who) {
  if (!z) return ZADA_E_INVALID;
  z->c.lz_stopped = false;                                          // (as every entry point: zada_lzma_export_state)
  if (format != 8 && format != 9) { z->c.err = std::string(who) + ": format must be 8 (Deflate) or 9 (Deflate64)"; return ZADA_E_INVALID; }
  return 0;
}

int zada_inflate_device(zada_ctx *z, int format, const void *d_in, uint64_t n_in, void *d_out, uint64_t cap, uint64_t *out_len, uint64_t *in_used,
                        uint32_t *crc_inout) {
  int rc = inf_prepare(z, format, "zada_inflate_device");
  if (rc) return rc;
  Ctx *c = &z->c;
  if ((n_in && !d_in) || (cap && !d_out)) { c->err = "zada_inflate_device: null buffer"; return ZADA_E_INVALID; }
  if (n_in >= INF_MAX_BYTES || cap >= INF_MAX_BYTES) { c->err = "zada_inflate_device: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  return reader_device_one<InfReader>(c, out_len, in_used, crc_inout, [&](InfJob &J) {
    J = InfJob{(uint64_t)(uintptr_t)d_in, (uint64_t)(uintptr_t)d_out, n_in, cap, format, 0};
    return 0;
  });
}

int zada_inflate_batch(zada_ctx *z, int count, const int *format, const uint8_t *const *in, const uint64_t *n_in, uint8_t *const *out, const uint64_t *cap,
                       uint64_t *out_len, uint64_t *in_used, uint32_t *crc, int *rc_out) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (count && (!format || !in || !n_in || !cap || !rc_out)) { c->err = "zada_inflate_batch: null argument"; return ZADA_E_INVALID; }
  for (int i = 0; i < count; i++) {
    if (format[i] != 8 && format[i] != 9) { c->err = "zada_inflate_batch: format must be 8 (Deflate) or 9 (Deflate64)"; return ZADA_E_INVALID; }
    if ((n_in[i] && !in[i]) || (out && cap[i] && !out[i])) { c->err = "zada_inflate_batch: null buffer"; return ZADA_E_INVALID; }
    if (n_in[i] >= INF_MAX_BYTES || cap[i] >= INF_MAX_BYTES) { c->err = "zada_inflate_batch: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  }
  if (count == 0) return ZADA_OK;
  return reader_batch<InfReader>(c, count, in, n_in, out, cap, out_len, in_used, crc, rc_out,
                                 [&](int i, uint64_t d_in, uint64_t d_out) { return InfJob{d_in, d_out, n_in[i], cap[i], format[i], 0}; });
}

int zada_inflate(zada_ctx *z, int format, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used, uint32_t *crc_inout) {
  int rc = inf_prepare(z, format, "zada_inflate");
  if (rc) return rc;
  if ((n_in && !in) || (cap && !out)) { z->c.err = "zada_inflate: null buffer"; return ZADA_E_INVALID; }
  return reader_single(out_len, in_used, crc_inout, [&](uint64_t *ol, uint64_t *iu, uint32_t *reg, int *erc) {
    return zada_inflate_batch(z, 1, &format, &in, &n_in, &out, &cap, ol, iu, reg, erc);
  });
}

int zada_crypt_decode_batch(zada_ctx *z, int count, uint32_t (*keys)[3], uint8_t *const *buf, const uint64_t *n) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (count && (!keys || !buf || !n)) { c->err = "zada_crypt_decode_batch: null argument"; return ZADA_E_INVALID; }
  for (int i = 0; i < count; i++) if (n[i] && !buf[i]) { c->err = "zada_crypt_decode_batch: null buffer"; return ZADA_E_INVALID; }
  if (count == 0) return ZADA_OK;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  InfState *S = inf_state(c);
  if (!S) { c->err = "inflate: no memory for the tables"; return ZADA_E_NOMEM; }
  const uint64_t limit = (uint64_t)c->knob_batch_mib << 20;
  std::vector<uint8_t> host;
  std::vector<uint64_t> tab;
  for (int g0 = 0; g0 < count;) {
    uint64_t bytes = 0;
    int g1 = g0;
    while (g1 < count && (g1 == g0 || bytes + n[g1] <= limit)) bytes += n[g1++];
    const uint32_t E = (uint32_t)(g1 - g0);
    const uint64_t o_ptr = 0, o_len = (uint64_t)E * 8, o_key = (uint64_t)E * 16, tbytes = o_key + (uint64_t)E * 12;
    int rc = dev_grow(c, S->arena, bytes + 16, "hipMalloc (crypt arena)");
    if (!rc) rc = dev_grow(c, S->tabs, tbytes, "hipMalloc (crypt tables)");
    if (rc) return rc;
    host.resize(bytes ? bytes : 1);
    tab.assign((size_t)(tbytes + 7) / 8, 0);
    uint64_t o = 0;
    for (uint32_t k = 0; k < E; k++) {
      const int i = g0 + (int)k;
      if (n[i]) memcpy(host.data() + o, buf[i], n[i]);
      tab[k] = (uint64_t)(uintptr_t)(S->arena.p + o); tab[E + k] = n[i];
      memcpy((uint8_t *)tab.data() + o_key + 12 * (uint64_t)k, keys[i], 12);
      o += n[i];
    }
    hipStream_t st = c->stream;
    if (bytes) hipMemcpyAsync(S->arena.p, host.data(), bytes, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(S->tabs.p, tab.data(), tbytes, hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(k_crypt_decode, dim3((E + INF_WAVE - 1) / INF_WAVE), dim3(INF_WAVE), 0, st, (const uint64_t *)(S->tabs.p + o_ptr), (const uint64_t *)(S->tabs.p + o_len),
                       (uint32_t *)(S->tabs.p + o_key), E);
    if (bytes) hipMemcpyAsync(host.data(), S->arena.p, bytes, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync((uint8_t *)tab.data() + o_key, S->tabs.p + o_key, (size_t)E * 12, hipMemcpyDeviceToHost, st);
    if (hip_check(c, hipGetLastError(), "crypt decode") || hip_check(c, hipStreamSynchronize(st), "crypt decode")) { (void)hipGetLastError(); return ZADA_E_HIP; }
    o = 0;
    for (uint32_t k = 0; k < E; k++) {
      const int i = g0 + (int)k;
      if (n[i]) memcpy(buf[i], host.data() + o, n[i]);
      memcpy(keys[i], (uint8_t *)tab.data() + o_key + 12 * (uint64_t)k, 12);
      o += n[i];
    }
    g0 = g1;
  }
  return ZADA_OK;
}
