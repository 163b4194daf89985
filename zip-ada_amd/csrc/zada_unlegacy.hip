// zada_unlegacy.hip -- UnZip.Decompress.Unshrink, Unreduce and Explode (unzip-decompress.adb:590-1418; Zip formats 1, 2 .. 5 and 6) for a batch of
// entries: one wave per entry.
//
// All three formats are chains: an LZW code is read through the table the codes before it built, a Reduce byte through the follower set of the
// byte before it, an Implode symbol from the bit behind the symbol before it.  What runs in parallel is the entries: the batch is what the design
// serves, and one stream alone runs at one wave's pace (as for Inflate, DESIGN.md 13, and LZMA, 15).  The chain (zada_unlegacy_logic.h) is
// wave-uniform: every lane holds the same bit buffer and state, and what is read from LDS on its way moves to the scalar side with readfirstlane.
// The 64 lanes add what lies around the chain (zada_unlegacy_wave.h): the compressed input comes into LDS in coalesced pieces of ULG_STAGE bytes;
// literals wait in a queue and are stored 64 at a time; copies are done by all lanes out of the entry's own output.  One kernel per format, since
// the LDS footprints differ:
//   k_unshrink  parent u16 [8194], literal u8 [8196], the "free" and "has a child" bit sets (257 words each) and the string stack (8196 bytes)
//               in LDS: 35 280 bytes with the stage, FOUR entries per CU.  The walk up the tree is the chain; the lanes do the partial clear (child marks over
//               the allocated nodes with LDS atomics, free |= not child) and move a finished string from the stack into the queue, so that Shrink
//               never reads its own output.
//   k_unreduce  followers u8 [256][64] and Slen u8 [256] in LDS: 17 028 bytes with the stage, NINE entries per CU.
//   k_explode   the three trees in their canonical form (counts per length u16 [3][17], symbols u8 [3][256]) and the lengths while a tree is
//               built: 1 556 bytes with the stage; its launches keep 16 waves per CU in flight.  A code is found length by length from the counts.
// (39 / 26 / 122 VGPRs, no scratch: DESIGN.md 23.)
// The CRC-32 of the output is k_inf_crc's (zada_inflate.hip), through inflate_crc_entries.
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
#include "zada_unlegacy_logic.h"
#include "zada_unlegacy_wave.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {

struct UlgJob { uint64_t in, out, n_in, cap; uint32_t method, flags; };
enum { ULG_K_SHRINK = 0, ULG_K_REDUCE = 1, ULG_K_EXPLODE = 2, ULG_NKERNELS = 3 };

// file-scope LDS objects: every access is a ds_ instruction; a kernel is given only those it names
__shared__ uint32_t s_ulg_next;
__shared__ uint16_t s_sh_par[ULG_SH_NODES];
__shared__ uint8_t s_sh_lit[(ULG_SH_NODES + 3) & ~3u];
__shared__ uint32_t s_sh_free[ULG_SH_WORDS];
__shared__ uint32_t s_sh_child[ULG_SH_WORDS];
__shared__ uint8_t s_sh_stack[ULG_SH_STACK];
__shared__ uint8_t s_rd_slen[256];
__shared__ uint8_t s_rd_fol[256 * 64];
__shared__ uint16_t s_ex_cnt[3 * 17 + 1];
__shared__ uint16_t s_ex_off[18];
__shared__ uint8_t s_ex_sym[3 * 256];
__shared__ uint8_t s_ex_len[256];

struct UlgWaveIO : UlgWaveBase {
  // Unshrink
  __device__ __forceinline__ uint32_t sh_par(uint32_t i) const { return s_sh_par[i]; }
  __device__ __forceinline__ void sh_set_par(uint32_t i, uint32_t v) { s_sh_par[i] = (uint16_t)v; }
  __device__ __forceinline__ uint32_t sh_lit(uint32_t i) const { return s_sh_lit[i]; }
  __device__ __forceinline__ void sh_set_lit(uint32_t i, uint32_t v) { s_sh_lit[i] = (uint8_t)v; }
  __device__ __forceinline__ uint32_t sh_free(uint32_t w) const { return s_sh_free[w]; }
  __device__ __forceinline__ void sh_set_free(uint32_t w, uint32_t v) { s_sh_free[w] = v; }
  __device__ __forceinline__ uint32_t sh_child(uint32_t w) const { return s_sh_child[w]; }
  __device__ __forceinline__ void sh_set_child(uint32_t w, uint32_t v) { s_sh_child[w] = v; }
  __device__ __forceinline__ void sh_child_or(uint32_t w, uint32_t v) { atomicOr(&s_sh_child[w], v); }
  __device__ __forceinline__ void sh_set_stack(uint32_t i, uint32_t v) { s_sh_stack[i] = (uint8_t)v; }
  // a finished string goes from the stack into the queue: every lane wrote the stack's bytes itself, so each reads its own store
  __device__ __forceinline__ void put_stack(uint32_t from, uint32_t len) {
    const uint32_t lane = threadIdx.x;
    while (len) {
      const uint32_t room = ULG_WAVE - q, take = len < room ? len : room;
      if (lane >= q && lane < q + take) my = s_sh_stack[from + lane - q];
      q += take; from += take; len -= take;
      if (q == ULG_WAVE) flush();
    }
  }
  // Unreduce
  __device__ __forceinline__ uint32_t rd_slen(uint32_t i) const { return s_rd_slen[i]; }
  __device__ __forceinline__ void rd_set_slen(uint32_t i, uint32_t v) { s_rd_slen[i] = (uint8_t)v; }
  __device__ __forceinline__ uint32_t rd_fol(uint32_t i) const { return s_rd_fol[i]; }
  __device__ __forceinline__ void rd_set_fol(uint32_t i, uint32_t v) { s_rd_fol[i] = (uint8_t)v; }
  __device__ __forceinline__ void rd_zero() {
    __syncthreads();
    uint32_t *w = (uint32_t *)s_rd_fol;
    for (uint32_t i = threadIdx.x; i < 256 * 64 / 4; i += ULG_WAVE) w[i] = 0u;
    __syncthreads();
  }
  // Explode
  __device__ __forceinline__ uint32_t ex_cnt(uint32_t i) const { return s_ex_cnt[i]; }
  __device__ __forceinline__ void ex_set_cnt(uint32_t i, uint32_t v) { s_ex_cnt[i] = (uint16_t)v; }
  __device__ __forceinline__ uint32_t ex_off(uint32_t i) const { return s_ex_off[i]; }
  __device__ __forceinline__ void ex_set_off(uint32_t i, uint32_t v) { s_ex_off[i] = (uint16_t)v; }
  __device__ __forceinline__ uint32_t ex_sym(uint32_t i) const { return s_ex_sym[i]; }
  __device__ __forceinline__ void ex_set_sym(uint32_t i, uint32_t v) { s_ex_sym[i] = (uint8_t)v; }
  __device__ __forceinline__ uint32_t ex_len(uint32_t i) const { return s_ex_len[i]; }
  __device__ __forceinline__ void ex_set_len(uint32_t i, uint32_t v) { s_ex_len[i] = (uint8_t)v; }
};

// the entries of one launch are handed out from a counter, longest first (order)
template <int K>
__device__ __forceinline__ void ulg_wave(const UlgJob *__restrict__ jobs, const uint32_t *__restrict__ order, uint32_t count, uint32_t *counter, UlgResult *results) {
  const uint32_t lane = threadIdx.x;
  for (;;) {
    __syncthreads();
    if (lane == 0) s_ulg_next = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t slot = ULG_UNI(s_ulg_next);
    if (slot >= count) break;
    const uint32_t e = order[slot];
    const UlgJob J = jobs[e];
    UlgWaveIO io;
    io.open((ulg_gcu8 *)J.in, J.n_in, (ulg_gu8 *)J.out);
    UlgResult R;
    if constexpr (K == ULG_K_SHRINK) ulg_unshrink(io, J.cap, R);
    else if constexpr (K == ULG_K_REDUCE) ulg_unreduce(io, ULG_UNI(J.method) - 1u, J.cap, R);
    else ulg_explode(io, ULG_UNI(J.flags), J.cap, R);
    if (lane == 0) results[e] = R;
  }
}
__global__ void __launch_bounds__(ULG_WAVE) k_unshrink(const UlgJob *__restrict__ jobs, const uint32_t *__restrict__ order, uint32_t count, uint32_t *counter, UlgResult *results) {
  ulg_wave<ULG_K_SHRINK>(jobs, order, count, counter, results);
}
__global__ void __launch_bounds__(ULG_WAVE) k_unreduce(const UlgJob *__restrict__ jobs, const uint32_t *__restrict__ order, uint32_t count, uint32_t *counter, UlgResult *results) {
  ulg_wave<ULG_K_REDUCE>(jobs, order, count, counter, results);
}
__global__ void __launch_bounds__(ULG_WAVE) k_explode(const UlgJob *__restrict__ jobs, const uint32_t *__restrict__ order, uint32_t count, uint32_t *counter, UlgResult *results) {
  ulg_wave<ULG_K_EXPLODE>(jobs, order, count, counter, results);
}

// ---- host side ----
struct UlgState : ReaderState {                       // (d_counter: one per launch of a call)
  int cus = 0;
};

static UlgState *ulg_state(Ctx *c) {
  if (c->ulg) return (UlgState *)c->ulg;
  UlgState *S = new (std::nothrow) UlgState();
  if (!S) return nullptr;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c->device) != hipSuccess || hipMalloc((void **)&S->d_counter, ULG_NKERNELS * 4) != hipSuccess) {
    (void)hipGetLastError();
    delete S;
    return nullptr;
  }
  S->cus = prop.multiProcessorCount;
  c->ulg = S;
  return S;
}
void unlegacy_destroy(Ctx *c) {
  UlgState *S = (UlgState *)c->ulg;
  if (!S) return;
  dev_free(S->tabs); dev_free(S->arena);
  hipFree(S->d_counter);
  delete S;
  c->ulg = nullptr;
}

// E jobs (device addresses) through one launch per format present and one of k_inf_crc; res [E] receives the records
static int ulg_run(Ctx *c, UlgState *S, const std::vector<UlgJob> &jobs, const uint32_t *crc_in, std::vector<UlgResult> &res) {
  const uint32_t E = (uint32_t)jobs.size();
  res.resize(E);
  if (E == 0) return 0;
  std::vector<uint32_t> by[ULG_NKERNELS], order;
  for (uint32_t i = 0; i < E; i++) by[jobs[i].method == 1 ? ULG_K_SHRINK : jobs[i].method == 6 ? ULG_K_EXPLODE : ULG_K_REDUCE].push_back(i);
  uint32_t begin[ULG_NKERNELS];
  for (int k = 0; k < ULG_NKERNELS; k++) {
    std::stable_sort(by[k].begin(), by[k].end(), [&](uint32_t a, uint32_t b) { return jobs[a].n_in > jobs[b].n_in; });
    begin[k] = (uint32_t)order.size();
    order.insert(order.end(), by[k].begin(), by[k].end());
  }
  ReaderTables<UlgJob, UlgResult> T;
  int rc = reader_tables_send(c, S, "unlegacy", jobs, order, nullptr, ULG_NKERNELS, T);
  if (rc) return rc;
  hipStream_t st = c->stream;
  c->tmark("unlegacy:begin");
  static const uint32_t per_cu[ULG_NKERNELS] = {4u, 9u, 16u};
  static const char *const mark[ULG_NKERNELS] = {"unlegacy:k_unshrink", "unlegacy:k_unreduce", "unlegacy:k_explode"};
  for (int k = 0; k < ULG_NKERNELS; k++) {
    const uint32_t n = (uint32_t)by[k].size();
    if (!n) continue;
    const uint32_t waves = (uint32_t)S->cus * per_cu[k];
    const uint32_t grid = n < waves ? n : waves;
    const uint32_t *d_order = T.order + begin[k];
    if (k == ULG_K_SHRINK) hipLaunchKernelGGL(k_unshrink, dim3(grid), dim3(ULG_WAVE), 0, st, T.jobs, d_order, n, S->d_counter + k, T.res);
    else if (k == ULG_K_REDUCE) hipLaunchKernelGGL(k_unreduce, dim3(grid), dim3(ULG_WAVE), 0, st, T.jobs, d_order, n, S->d_counter + k, T.res);
    else hipLaunchKernelGGL(k_explode, dim3(grid), dim3(ULG_WAVE), 0, st, T.jobs, d_order, n, S->d_counter + k, T.res);
    c->tmark(mark[k]);
  }
  rc = reader_tables_fetch(c, "unlegacy", T, res);
  if (rc) return rc;
  // the entries' Zip CRC-32 (k_inf_crc)
  std::vector<uint64_t> optr(E), olen(E);
  std::vector<uint32_t> regs(E);
  for (uint32_t i = 0; i < E; i++) { optr[i] = jobs[i].out; olen[i] = res[i].rc == 0 ? res[i].out_len : 0; regs[i] = crc_in ? crc_in[i] : 0u; }
  rc = inflate_crc_entries(c, E, optr.data(), olen.data(), regs.data());
  if (rc) return rc;
  c->tmark("unlegacy:k_inf_crc");
  for (uint32_t i = 0; i < E; i++) {
    res[i].crc = regs[i];
    for (uint64_t v : {(uint64_t)res[i].rule, res[i].in_pos, res[i].out_pos, (uint64_t)0}) S->last_entries.push_back(v);
  }
  return 0;
}

static void ulg_describe(Ctx *c, const UlgResult &R, int entry) {
  char buf[240];
  snprintf(buf, sizeof buf, "unlegacy: entry %d: %s at input byte %llu", entry, ulg_rule_name(R.rule), (unsigned long long)R.in_pos);
  c->err = buf;
}

struct UlgReader : ReaderTraits<UlgJob, UlgResult, UlgState> {
  static constexpr const char *word = "unlegacy";
  static UlgState *state(Ctx *c) { return ulg_state(c); }
  static int run(Ctx *c, UlgState *S, std::vector<UlgJob> &jobs, const uint32_t *crc_in, std::vector<UlgResult> &res, uint32_t) { return ulg_run(c, S, jobs, crc_in, res); }
  static void describe(Ctx *c, const UlgResult &R, int entry) { ulg_describe(c, R, entry); }
};

// ulg_run for zada_unzip_device (zada_internal.h): ReaderJob::format is the method (1 .. 6), eos the entry's general-purpose bits 1 and 2
int unlegacy_run_jobs(Ctx *c, uint32_t E, const ReaderJob *rj, ReaderRes *rr, bool *described) {
  return reader_run_jobs<UlgReader>(c, E, rj, rr, described, [](const ReaderJob &J) { return UlgJob{J.in, J.out, J.n_in, J.cap, (uint32_t)J.format, J.eos & 6u}; });
}

}  // namespace zada

using namespace zada;

static constexpr uint64_t ULG_MAX_BYTES = 1ull << 40;      // (as Inflate: a stream or an output of 1 TiB and more is beyond any device)

int zada_unlegacy_device(zada_ctx *z, int method, int flags, const void *d_in, uint64_t n_in, void *d_out, uint64_t cap, uint64_t *out_len, uint64_t *in_used,
                         uint32_t *crc_inout) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (method < 1 || method > 6) { c->err = "zada_unlegacy_device: method outside 1 .. 6 (1 Shrink, 2 .. 5 Reduce, 6 Implode)"; return ZADA_E_INVALID; }
  if ((n_in && !d_in) || (cap && !d_out)) { c->err = "zada_unlegacy_device: null buffer"; return ZADA_E_INVALID; }
  if (n_in >= ULG_MAX_BYTES || cap >= ULG_MAX_BYTES) { c->err = "zada_unlegacy_device: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  return reader_device_one<UlgReader>(c, out_len, in_used, crc_inout, [&](UlgJob &J) {
    J = UlgJob{(uint64_t)(uintptr_t)d_in, (uint64_t)(uintptr_t)d_out, n_in, cap, (uint32_t)method, (uint32_t)flags & 6u};
    return 0;
  });
}

int zada_unlegacy_batch(zada_ctx *z, int count, const uint8_t *const *in, const uint64_t *n_in, uint8_t *const *out, const uint64_t *cap, const uint16_t *method,
                        const uint8_t *flags, uint64_t *out_len, uint64_t *in_used, uint32_t *crc, int *rc_out) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (count && (!in || !n_in || !cap || !method || !rc_out)) { c->err = "zada_unlegacy_batch: null argument"; return ZADA_E_INVALID; }
  for (int i = 0; i < count; i++) {
    if (method[i] < 1 || method[i] > 6) { c->err = "zada_unlegacy_batch: method outside 1 .. 6 (1 Shrink, 2 .. 5 Reduce, 6 Implode)"; return ZADA_E_INVALID; }
    if ((n_in[i] && !in[i]) || (out && cap[i] && !out[i])) { c->err = "zada_unlegacy_batch: null buffer"; return ZADA_E_INVALID; }
    if (n_in[i] >= ULG_MAX_BYTES || cap[i] >= ULG_MAX_BYTES) { c->err = "zada_unlegacy_batch: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  }
  if (count == 0) return ZADA_OK;
  return reader_batch<UlgReader>(c, count, in, n_in, out, cap, out_len, in_used, crc, rc_out, [&](int i, uint64_t d_in, uint64_t d_out) {
    return UlgJob{d_in, d_out, n_in[i], cap[i], method[i], flags ? (uint32_t)flags[i] & 6u : 0u};
  });
}

int zada_unlegacy(zada_ctx *z, int method, int flags, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used,
                  uint32_t *crc_inout) {
  if (!z) return ZADA_E_INVALID;
  z->c.lz_stopped = false;
  if (method < 1 || method > 6) { z->c.err = "zada_unlegacy: method outside 1 .. 6 (1 Shrink, 2 .. 5 Reduce, 6 Implode)"; return ZADA_E_INVALID; }
  if ((n_in && !in) || (cap && !out)) { z->c.err = "zada_unlegacy: null buffer"; return ZADA_E_INVALID; }
  const uint16_t m = (uint16_t)method;
  const uint8_t f = (uint8_t)(flags & 6);
  return reader_single(out_len, in_used, crc_inout, [&](uint64_t *ol, uint64_t *iu, uint32_t *reg, int *erc) {
    return zada_unlegacy_batch(z, 1, &in, &n_in, &out, &cap, &m, &f, ol, iu, reg, erc);
  });
}

uint64_t zada_unlegacy_last_records(zada_ctx *z, uint64_t *dst, uint64_t cap_items) {
  if (!z || !z->c.ulg || (cap_items && !dst)) return 0;
  return reader_last_records(((const UlgState *)z->c.ulg)->last_entries, dst, cap_items);
}
