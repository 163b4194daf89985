// zada_inflate_par.hip -- one large raw Deflate stream (Zip format 8; Deflate64, format 9, with the knob "inflate_par_deflate64") on many waves:
// the method of zada_inflate_par_logic.h (two-stage decoding with window markers).  Every dependency between chunks is a kernel boundary or a host step: no kernel waits on another workgroup.
//   k_infp_scout : one wave per chunk: find the first candidate block start (64 bit offsets per step through infp_filter, read from the staged
//                  input in LDS; survivors one at a time through inf_dynamic_header), then count from it without writing.
//   (host)       : the chain over the records (infp_walk); a chunk whose start is not the end of the one before is scouted again, exactly.
//   k_infp_decode: one wave per live chunk: k_inflate's token queue and expansion, on 16-bit symbols in a workspace of 2 bytes per output byte
//                  (Deflate64: 32-bit symbols, 4 bytes per output byte -- InfpFmt in zada_inflate_par_logic.h says why).
//   k_infp_window: one workgroup, the live chunks in order: the markers in the last 32 KiB (Deflate64: 64 KiB) of each chunk become symbols.
//   k_infp_finish: symbols to bytes in d_out, all chunks in parallel.
//   CRC-32       : the encoder's k_crc_chunks / k_crc_fold (crc_launch / crc_finish), the bytes before d_out's first 16-byte boundary on the host.
// The batch forms k_infpb_* ("inflate_par_batch") do the same over a table of streams: the large entries of one zada_unzip_device
// group share every launch -- a wave per (stream, chunk) job, a wave per live row, a window workgroup per stream -- by the plan of
// zada_inflate_par_batch_plan.h; their CRC-32 goes through the stored entries' k_uz_store / k_uz_fold (unzip_sum_entries).
// A stream the method does not take (damaged, too many repairs, one live chunk, Deflate64 without its knob, no memory) is decoded by
// zada_inflate_device's one wave, whose verdict is the answer; nothing has been written to d_out before that.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_inflate_par_logic.h"
#include "zada_inflate_par_batch_plan.h"
#include "zada_inflate_wave.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {

// the reader of a wave behind the interface infp_blocks asks for
struct InfpWaveEnvBase {
  gcu8 *in; uint64_t n_in; uint32_t *stage;
  __device__ __forceinline__ void reopen(InfWaveReader &br, uint64_t at) { br.open(in, n_in, at, stage); }
};
// count: nothing is written
struct InfpCountEnv : InfpWaveEnvBase {
  uint64_t bytes;
  __device__ __forceinline__ uint32_t stored(uint64_t, uint32_t len) { bytes += len; return INF_OK; }
  __device__ __forceinline__ uint32_t token(uint32_t len, uint32_t, uint32_t) { bytes += len; return INF_OK; }
};

// inf_expand on symbols: lane q holds token q, written behind `pos`; base: the chunk's first output position.  A source before base is a marker.
// (A Deflate64 token has up to 65 538 symbols and may begin at base itself: every source of a token lies before its first symbol P, so the i % D
// loop reads nothing the token writes, whatever its length, and the fence rule asks only where the sources end.)
template <int FORMAT> __device__ __forceinline__ void infp_expand(__attribute__((address_space(1))) typename InfpFmt<FORMAT>::sym_t *sym, uint64_t base, uint64_t pos,
                                                                  uint32_t q, uint32_t my_len, uint32_t my_dist, uint32_t my_val, uint64_t &fence_pos) {
  typedef typename InfpFmt<FORMAT>::sym_t sym_t;
  const uint32_t lane = threadIdx.x;
  uint32_t len = lane < q ? my_len : 0u, incl = len;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
  const uint64_t start = pos + (incl - len);
  if (len && my_dist == 0) sym[start] = (sym_t)my_val;
  uint64_t mask = __ballot(len != 0 && my_dist != 0);
  while (mask) {
    const int k = __ffsll((unsigned long long)mask) - 1;
    mask &= mask - 1;
    const uint32_t L = (uint32_t)__builtin_amdgcn_readlane((int)len, k), D = (uint32_t)__builtin_amdgcn_readlane((int)my_dist, k);
    const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)(incl - len), k);
    const uint64_t P = pos + off;
    const uint64_t src_end = P - D + (L < D ? L : D);
    if (src_end > fence_pos && src_end > base) {
      // (the fence rule of inf_expand: a wave that reads its own stores of an instant ago waits for them first)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      fence_pos = P;
    }
    for (uint32_t i = lane; i < L; i += INF_WAVE) {
      const uint64_t sp = P - D + (D >= L ? i : i % D);
      sym[P + i] = sp >= base ? sym[sp] : (sym_t)infp_marker<FORMAT>(base, sp);
    }
  }
}

// decode: the token queue of k_inflate; pos is the position in the whole output, so "distance beyond the bytes written so far" is exact
template <int FORMAT> struct InfpDecodeEnv : InfpWaveEnvBase {
  __attribute__((address_space(1))) typename InfpFmt<FORMAT>::sym_t *sym; uint64_t base, limit, pos, qpos, fence_pos; uint32_t q, my_len, my_dist, my_val;
  __device__ __forceinline__ void flush() { infp_expand<FORMAT>(sym, base, qpos, q, my_len, my_dist, my_val, fence_pos); q = 0; my_len = 0; qpos = pos; }
  __device__ __forceinline__ uint32_t stored(uint64_t at, uint32_t len) {
    if (pos + len > limit) return INF_R_OUTPUT_FULL;
    flush();
    for (uint32_t i = threadIdx.x; i < len; i += INF_WAVE) sym[pos + i] = in[at + i];
    pos += len; qpos = pos;
    return INF_OK;
  }
  __device__ __forceinline__ uint32_t token(uint32_t len, uint32_t dist, uint32_t val) {
    if (dist > pos) return INF_R_DISTANCE_TOO_FAR;
    if (pos + len > limit) return INF_R_OUTPUT_FULL;          // (the count said how many symbols the chunk has: none is written beyond them)
    if (threadIdx.x == q) { my_len = len; my_dist = dist; my_val = val; }
    pos += len;
    if (++q == INF_WAVE) flush();
    return INF_OK;
  }
};

// ---- what a wave does with one chunk, one workgroup with one stream's live rows: shared by the kernels of one stream and their batch forms ----
// scout: the chunk `chunk` of the stream (in, n_in), bit positions the stream's own; start_bit exact or INFP_SEARCH
template <bool D64> __device__ __forceinline__ InfpRec infp_scout_chunk(gcu8 *in, uint64_t n_in, uint64_t chunk_bytes, uint32_t chunk, uint64_t start_bit, InfTables &T, uint32_t *stage) {
  const uint32_t lane = threadIdx.x;
  const uint64_t lo_bit = (uint64_t)chunk * chunk_bytes * 8, total_bits = n_in * 8;
  const uint64_t stop_bits = lo_bit + chunk_bytes * 8;
  const uint64_t hi_bit = stop_bits < total_bits ? stop_bits : total_bits;
  InfpCountEnv env;
  env.in = in; env.n_in = n_in; env.stage = stage; env.bytes = 0;
  InfWaveReader br;
  uint64_t start = start_bit;
  bool found = start != INFP_SEARCH;
  if (!found) {
    // ---- find: 64 bit offsets per step; every lane takes the 96 bits at its offset from the stage ----
    br.open(in, n_in, lo_bit >> 3, stage);
    for (uint64_t o = lo_bit; o < hi_bit && !found; o += 64) {
      // (a lane's window: the four words from the word that holds its first bit; the step's last lane begins at byte (o + 63) / 8)
      if ((o >> 3) < br.base || ((o + 63) >> 3) + 20 > br.base + INF_STAGE + 8) br.fill((o >> 3) & ~3ull);
      const uint64_t my = o + lane;
      const uint32_t b = (uint32_t)((my >> 3) - br.base), w0 = b >> 2, sh = (b & 3u) * 8u + (uint32_t)(my & 7u);      // sh <= 31
      const uint64_t q0 = (uint64_t)stage[w0] | (uint64_t)stage[w0 + 1] << 32, q1 = (uint64_t)stage[w0 + 2] | (uint64_t)stage[w0 + 3] << 32;
      const uint64_t lo = sh ? (q0 >> sh) | (q1 << (64u - sh)) : q0, hi = q1 >> sh;
      uint64_t mask = __ballot(my < hi_bit && infp_filter(lo, hi, D64));
      while (mask) {
        const int k = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        const uint64_t cand = o + (uint32_t)k;
        infp_seek(br, env, cand);
        if (infp_candidate(br, T, lane, INF_WAVE, D64)) { start = cand; found = true; break; }      // (a survivor's header may move the stage: asked again above)
      }
    }
  }
  InfpRec R;
  R.start_bit = found ? start : 0; R.end_bit = 0; R.bytes = 0; R.flags = (found ? INFP_F_FOUND : 0u) | (start_bit != INFP_SEARCH ? INFP_F_EXACT : 0u); R.rule = 0;
  if (found) {
    // ---- count ----
    infp_seek(br, env, start);
    uint32_t final = 0;
    R.rule = infp_blocks(br, T, n_in, stop_bits, lane, INF_WAVE, env, final, D64);
    R.end_bit = br.used_bits(); R.bytes = env.bytes;
    if (final) R.flags |= INFP_F_FINAL;
  }
  return R;
}

// decode: one live chunk from start_bit into the symbols sym [off, off + bytes) of its stream; -> the rule broken, end_bit and final as found
template <int FORMAT> __device__ __forceinline__ uint32_t infp_decode_chunk(gcu8 *in, uint64_t n_in, uint64_t start_bit, uint64_t stop_bits, uint64_t off, uint64_t bytes,
                                                                            typename InfpFmt<FORMAT>::sym_t *sym_, InfTables &T, uint32_t *stage, uint64_t &end_bit, uint32_t &final) {
  InfpDecodeEnv<FORMAT> env;
  env.in = in; env.n_in = n_in; env.stage = stage;
  env.sym = (__attribute__((address_space(1))) typename InfpFmt<FORMAT>::sym_t *)sym_;
  env.base = off; env.limit = off + bytes; env.pos = env.qpos = off; env.fence_pos = off;
  env.q = 0; env.my_len = env.my_dist = env.my_val = 0;
  InfWaveReader br;
  infp_seek(br, env, start_bit);
  final = 0;
  uint32_t rule = infp_blocks(br, T, n_in, stop_bits, threadIdx.x, INF_WAVE, env, final, InfpFmt<FORMAT>::D64);
  if (!rule) env.flush();
  if (!rule && env.pos != env.limit) rule = INF_R_OUTPUT_FULL;          // (not what the count saw: the stream goes to the one-wave decoder)
  end_bit = br.used_bits();
  return rule;
}

// window: one workgroup walks the live rows live [1 .. nlive) of ONE stream in order; Row: InfpLive or InfpbLive.  -> the markers this thread resolved
constexpr uint32_t INFP_WIN_THREADS = 1024, INFP_WIN_PIECE = 32768, INFP_WIN_DONE = 0x40000000u;      // (the flag of a resolved symbol: no bit of either marker layout)
template <int FORMAT, class Row> __device__ __forceinline__ uint32_t infp_window_walk(const Row *__restrict__ live, uint32_t nlive, typename InfpFmt<FORMAT>::sym_t *sym) {
  typedef typename InfpFmt<FORMAT>::sym_t sym_t;
  constexpr uint32_t WINDOW = InfpFmt<FORMAT>::WINDOW, MARK = InfpFmt<FORMAT>::MARK, PER = INFP_WIN_PIECE / INFP_WIN_THREADS;
  uint32_t mine = 0;
  for (uint32_t j = 1; j < nlive; j++) {
    const uint64_t base = live[j].off, end = base + live[j].bytes;
    const uint64_t from = end - base > WINDOW ? end - WINDOW : base;
    // The window in pieces of 32 Ki symbols -- one for Deflate, two for Deflate64: the markers of a chunk point in front of it, never into it, so
    // its pieces do not depend on one another and a thread holds 32 symbols at a time for either format.
    // A thread's 32 symbols first, then what its markers point at, then the stores: the loads of a step do not wait for one another (a chunk is
    // two memory latencies and a barrier, not sixty-four)
#pragma unroll 1
    for (uint32_t piece = 0; piece < WINDOW / INFP_WIN_PIECE; piece++) {
      const uint64_t first = from + (uint64_t)piece * INFP_WIN_PIECE + threadIdx.x;
      uint32_t v[PER];
#pragma unroll
      for (uint32_t k = 0; k < PER; k++) {
        const uint64_t i = first + (uint64_t)k * INFP_WIN_THREADS;
        v[k] = i < end ? sym[i] : 0u;
      }
#pragma unroll
      for (uint32_t k = 0; k < PER; k++)
        if (v[k] & MARK) v[k] = INFP_WIN_DONE | sym[infp_marker_source<FORMAT>(base, v[k])];
#pragma unroll
      for (uint32_t k = 0; k < PER; k++)
        if (v[k] & INFP_WIN_DONE) { sym[first + (uint64_t)k * INFP_WIN_THREADS] = (sym_t)(v[k] & ~INFP_WIN_DONE); mine++; }
    }
    __syncthreads();            // the next chunk reads what this one resolved
  }
  return mine;
}

// finish: the symbols [base, base + bytes) of one live row to bytes, the pieces blockIdx.y, blockIdx.y + gridDim.y, ... of it; out [0] is the
// stream's first byte, at any alignment: byte stores, so that two streams' adjacent ranges never share a store
constexpr uint32_t INFP_FIN_THREADS = 256, INFP_FIN_PIECE = 16384;
template <int FORMAT> __device__ __forceinline__ uint32_t infp_finish_row(uint64_t base, uint64_t bytes, const typename InfpFmt<FORMAT>::sym_t *__restrict__ sym, uint8_t *out) {
  uint32_t mine = 0;
  for (uint64_t p0 = (uint64_t)blockIdx.y * INFP_FIN_PIECE; p0 < bytes; p0 += (uint64_t)gridDim.y * INFP_FIN_PIECE) {
    const uint64_t p1 = p0 + INFP_FIN_PIECE < bytes ? p0 + INFP_FIN_PIECE : bytes;
    for (uint64_t i = base + p0 + threadIdx.x; i < base + p1; i += INFP_FIN_THREADS) {
      uint32_t v = sym[i];
      if (v & InfpFmt<FORMAT>::MARK) { v = sym[infp_marker_source<FORMAT>(base, v)]; mine++; }
      out[i] = (uint8_t)v;
    }
  }
  return mine;
}

// ---- one stream ----
template <bool D64> __global__ void __launch_bounds__(INF_WAVE) k_infp_scout(const uint8_t *in_, uint64_t n_in, uint64_t chunk_bytes, const InfpJob *__restrict__ jobs,
                                                                             uint32_t njobs, InfpRec *recs) {
  __shared__ InfTables T;
  __shared__ uint32_t stage[INF_STAGE / 4 + 2];
  if (blockIdx.x >= njobs) return;
  const InfpJob J = jobs[blockIdx.x];
  const InfpRec R = infp_scout_chunk<D64>((gcu8 *)in_, n_in, chunk_bytes, J.chunk, J.start_bit, T, stage);
  if (threadIdx.x == 0) recs[J.chunk] = R;
}

template <int FORMAT> __global__ void __launch_bounds__(INF_WAVE) k_infp_decode(const uint8_t *in_, uint64_t n_in, InfpLive *live, uint32_t nlive,
                                                                                typename InfpFmt<FORMAT>::sym_t *sym_) {
  __shared__ InfTables T;
  __shared__ uint32_t stage[INF_STAGE / 4 + 2];
  if (blockIdx.x >= nlive) return;
  const InfpLive J = live[blockIdx.x];
  uint64_t end_bit;
  uint32_t final;
  const uint32_t rule = infp_decode_chunk<FORMAT>((gcu8 *)in_, n_in, J.start_bit, J.stop_bits, J.off, J.bytes, sym_, T, stage, end_bit, final);
  if (threadIdx.x == 0) { live[blockIdx.x].end_bit = end_bit; live[blockIdx.x].rule = rule; live[blockIdx.x].final = final; }
}

template <int FORMAT> __global__ void __launch_bounds__(INFP_WIN_THREADS) k_infp_window(const InfpLive *__restrict__ live, uint32_t nlive,
                                                                                        typename InfpFmt<FORMAT>::sym_t *sym, uint64_t *markers) {
  const uint32_t mine = infp_window_walk<FORMAT>(live, nlive, sym);
  if (mine) atomicAdd((unsigned long long *)markers, (unsigned long long)mine);
}

template <int FORMAT> __global__ void __launch_bounds__(INFP_FIN_THREADS) k_infp_finish(const InfpLive *__restrict__ live, uint32_t nlive,
                                                                                        const typename InfpFmt<FORMAT>::sym_t *__restrict__ sym, uint8_t *out, uint64_t *markers) {
  const uint32_t j = blockIdx.x;
  if (j >= nlive) return;
  const uint32_t mine = infp_finish_row<FORMAT>(live[j].off, live[j].bytes, sym, out);
  if (mine) atomicAdd((unsigned long long *)markers, (unsigned long long)mine);
}

// ---- the batch forms ("inflate_par_batch"): the same work over a table of streams (zada_inflate_par_batch_plan.h) ----
// scout: one wave per job = (stream, chunk, start); the record goes to the chunk's global index, and to back [job] where the host asks for the
// records of a repair round alone
template <bool D64> __global__ void __launch_bounds__(INF_WAVE) k_infpb_scout(const InfpbStream *__restrict__ streams, uint64_t chunk_bytes, const InfpbJob *__restrict__ jobs,
                                                                              uint32_t njobs, InfpRec *recs, InfpRec *back) {
  __shared__ InfTables T;
  __shared__ uint32_t stage[INF_STAGE / 4 + 2];
  if (blockIdx.x >= njobs) return;
  const InfpbJob J = jobs[blockIdx.x];
  const InfpbStream S = streams[J.stream];
  const InfpRec R = infp_scout_chunk<D64>((gcu8 *)S.in, S.n_in, chunk_bytes, J.chunk - S.first, J.start_bit, T, stage);
  if (threadIdx.x == 0) { recs[J.chunk] = R; if (back) back[blockIdx.x] = R; }
}

// decode: one wave per live row; off / bytes are positions in the stream's own output, the symbols lie from the stream's base on
template <int FORMAT> __global__ void __launch_bounds__(INF_WAVE) k_infpb_decode(const InfpbStream *__restrict__ streams, InfpbLive *live, uint32_t nlive,
                                                                                 typename InfpFmt<FORMAT>::sym_t *sym_) {
  __shared__ InfTables T;
  __shared__ uint32_t stage[INF_STAGE / 4 + 2];
  if (blockIdx.x >= nlive) return;
  const InfpbLive J = live[blockIdx.x];
  const InfpbStream S = streams[J.stream];
  uint64_t end_bit;
  uint32_t final;
  const uint32_t rule = infp_decode_chunk<FORMAT>((gcu8 *)S.in, S.n_in, J.start_bit, J.stop_bits, J.off, J.bytes, sym_ + S.sym, T, stage, end_bit, final);
  if (threadIdx.x == 0) { live[blockIdx.x].end_bit = end_bit; live[blockIdx.x].rule = rule; live[blockIdx.x].final = final; }
}

// window: one workgroup per stream, the streams' walks independent of one another (n_live = 0: the stream left after the decode)
template <int FORMAT> __global__ void __launch_bounds__(INFP_WIN_THREADS) k_infpb_window(const InfpbStream *__restrict__ streams, uint32_t nstreams, const InfpbLive *__restrict__ live,
                                                                                         typename InfpFmt<FORMAT>::sym_t *sym, uint64_t *markers) {
  if (blockIdx.x >= nstreams) return;
  const InfpbStream S = streams[blockIdx.x];
  const uint32_t mine = infp_window_walk<FORMAT>(live + S.first_live, S.n_live, sym + S.sym);
  if (mine) atomicAdd((unsigned long long *)markers, (unsigned long long)mine);
}

// finish: all live rows of the streams that stayed, in parallel, each into its stream's own output range
template <int FORMAT> __global__ void __launch_bounds__(INFP_FIN_THREADS) k_infpb_finish(const InfpbStream *__restrict__ streams, const InfpbLive *__restrict__ live, uint32_t nlive,
                                                                                         const typename InfpFmt<FORMAT>::sym_t *__restrict__ sym, uint64_t *markers) {
  const uint32_t j = blockIdx.x;
  if (j >= nlive) return;
  const InfpbStream S = streams[live[j].stream];
  if (!S.n_live) return;
  const uint32_t mine = infp_finish_row<FORMAT>(live[j].off, live[j].bytes, sym + S.sym, (uint8_t *)S.out);
  if (mine) atomicAdd((unsigned long long *)markers, (unsigned long long)mine);
}

// ---- host side ----
// the launches that know the symbol: sym is the workspace of InfpFmt <FORMAT>::sym_t
template <int FORMAT> static void infp_launch_decode(hipStream_t st, const uint8_t *in, uint64_t n_in, InfpLive *d_live, uint32_t nl, void *sym) {
  hipLaunchKernelGGL(k_infp_decode<FORMAT>, dim3(nl), dim3(INF_WAVE), 0, st, in, n_in, d_live, nl, (typename InfpFmt<FORMAT>::sym_t *)sym);
}
template <int FORMAT> static void infp_launch_resolve(Ctx *c, hipStream_t st, const InfpLive *d_live, uint32_t nl, void *sym, uint8_t *out, uint64_t *d_mark) {
  typedef typename InfpFmt<FORMAT>::sym_t sym_t;
  hipLaunchKernelGGL(k_infp_window<FORMAT>, dim3(1), dim3(INFP_WIN_THREADS), 0, st, d_live, nl, (sym_t *)sym, d_mark);
  c->tmark("inflate_par:k_infp_window");
  hipLaunchKernelGGL(k_infp_finish<FORMAT>, dim3(nl, 8), dim3(INFP_FIN_THREADS), 0, st, d_live, nl, (const sym_t *)sym, out, d_mark);
  c->tmark("inflate_par:k_infp_finish");
}

struct InfpState {
  DevBuf tabs;                                         // jobs, records, live chunks, the marker counter
  DevBuf sym;                                          // the symbols: 2 bytes per output byte, Deflate64 4
  zada_inflate_par_info last{};
};
static InfpState *infp_state(Ctx *c) {
  if (!c->infp) c->infp = new (std::nothrow) InfpState();
  return (InfpState *)c->infp;
}
void inflate_par_destroy(Ctx *c) {
  InfpState *S = (InfpState *)c->infp;
  if (!S) return;
  dev_free(S->tabs); dev_free(S->sym);
  delete S;
  c->infp = nullptr;
}

static uint32_t infp_crc_bytes(uint32_t r, const uint8_t *p, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) { r ^= p[i]; for (int b = 0; b < 8; b++) r = (r & 1u) ? (r >> 1) ^ 0xEDB88320u : r >> 1; }
  return r;
}

// One stream through the parallel path.  0: done, *out_len / *in_used / *crc_inout are set; 1: not taken, the record (zada_inflate_par_last) says
// why and nothing was written to d_out -- the caller runs the one-wave decoder; < 0: a HIP error.
int inflate_par_try(Ctx *c, int format, const void *d_in, uint64_t n_in, void *d_out, uint64_t cap, uint64_t *out_len, uint64_t *in_used, uint32_t *crc_inout) {
  InfpState *S = infp_state(c);
  if (!S) { c->err = "inflate_par: no memory for the state"; return ZADA_E_NOMEM; }
  zada_inflate_par_info &I = S->last;
  memset(&I, 0, sizeof I);
  I.streams = 1;
  auto fall = [&](int reason) { I.fell_back = 1; I.reason = reason; return 1; };
  if (format != 8 && !(format == 9 && c->knob_infp_deflate64)) return fall(INFP_FORMAT);
  const bool d64 = format == 9;
  const uint64_t chunk_bytes = (uint64_t)c->knob_infp_chunk_kib << 10;
  const uint64_t nch64 = (n_in + chunk_bytes - 1) / chunk_bytes;
  I.chunks = nch64;
  if (nch64 < 2) return fall(INFP_SINGLE_CHUNK);
  if (nch64 >= (1ull << 31)) return fall(INFP_MEMORY);
  const uint32_t nch = (uint32_t)nch64;
  // the tables: jobs [nch], records [nch], live chunks [nch], the marker counter
  const uint64_t o_jobs = 0, o_recs = o_jobs + (uint64_t)nch * sizeof(InfpJob), o_live = o_recs + (uint64_t)nch * sizeof(InfpRec),
                 o_mark = o_live + (uint64_t)nch * sizeof(InfpLive), total_tabs = o_mark + 16;
  if (dev_grow(c, S->tabs, total_tabs, nullptr)) return fall(INFP_MEMORY);
  hipStream_t st = c->stream;
  const uint8_t *in = (const uint8_t *)d_in;
  std::vector<InfpJob> jobs(nch);
  std::vector<InfpRec> recs(nch);
  for (uint32_t k = 0; k < nch; k++) jobs[k] = InfpJob{k ? INFP_SEARCH : 0ull, k, 0};
  hipMemcpyAsync(S->tabs.p + o_jobs, jobs.data(), (size_t)nch * sizeof(InfpJob), hipMemcpyHostToDevice, st);
  c->tmark("inflate_par:begin");
  auto scout = [&](uint32_t njobs) {
    hipLaunchKernelGGL(d64 ? k_infp_scout<true> : k_infp_scout<false>, dim3(njobs), dim3(INF_WAVE), 0, st, in, n_in, chunk_bytes, (const InfpJob *)(S->tabs.p + o_jobs), njobs,
                       (InfpRec *)(S->tabs.p + o_recs));
  };
  scout(nch);
  c->tmark("inflate_par:k_infp_scout");
  hipMemcpyAsync(recs.data(), S->tabs.p + o_recs, (size_t)nch * sizeof(InfpRec), hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipGetLastError(), "inflate_par scout launch") || hip_check(c, hipStreamSynchronize(st), "inflate_par scout")) return ZADA_E_HIP_;
  I.scout_rounds = 1;
  // the chain
  std::vector<uint8_t> is_live(nch, 0);
  std::vector<uint64_t> off(nch, 0);
  InfpWalk W;
  const uint64_t bound = infp_repair_bound(nch, (uint32_t)c->knob_infp_repair_pct);
  for (;;) {
    const int w = infp_walk(W, recs.data(), nch, chunk_bytes * 8, is_live.data(), off.data());
    I.repairs = W.repairs; I.live_chunks = W.live;
    if (w == INFP_W_DAMAGED) return fall(INFP_DAMAGED);
    if (w == INFP_W_DONE) break;
    if (W.repairs > bound) return fall(INFP_REPAIRS);
    const InfpJob J{W.expect, W.cur, 0};
    hipMemcpyAsync(S->tabs.p + o_jobs, &J, sizeof J, hipMemcpyHostToDevice, st);
    scout(1u);
    hipMemcpyAsync(&recs[W.cur], S->tabs.p + o_recs + (uint64_t)W.cur * sizeof(InfpRec), sizeof(InfpRec), hipMemcpyDeviceToHost, st);
    if (hip_check(c, hipGetLastError(), "inflate_par repair launch") || hip_check(c, hipStreamSynchronize(st), "inflate_par repair")) return ZADA_E_HIP_;
    I.scout_rounds++;
  }
  c->tmark("inflate_par:chain");
  if (W.total > cap) return fall(INFP_DAMAGED);
  if (W.live < 2) return fall(INFP_SINGLE_CHUNK);
  const uint64_t total = W.total;
  if (total && dev_grow(c, S->sym, total * (d64 ? sizeof(InfpFmt<9>::sym_t) : sizeof(InfpFmt<8>::sym_t)), nullptr)) return fall(INFP_MEMORY);
  // the live chunks, in order
  std::vector<InfpLive> live;
  live.reserve(W.live);
  for (uint32_t k = 0; k < nch; k++)
    if (is_live[k]) live.push_back(InfpLive{recs[k].start_bit, ((uint64_t)k + 1) * chunk_bytes * 8, off[k], recs[k].bytes, 0, 0, 0});
  const uint32_t nl = (uint32_t)live.size();
  hipMemcpyAsync(S->tabs.p + o_live, live.data(), (size_t)nl * sizeof(InfpLive), hipMemcpyHostToDevice, st);
  hipMemsetAsync(S->tabs.p + o_mark, 0, 16, st);
  InfpLive *d_live = (InfpLive *)(S->tabs.p + o_live);
  uint64_t *d_mark = (uint64_t *)(S->tabs.p + o_mark);
  std::vector<InfpLive> back(nl);
  if (d64) infp_launch_decode<9>(st, in, n_in, d_live, nl, S->sym.p); else infp_launch_decode<8>(st, in, n_in, d_live, nl, S->sym.p);
  c->tmark("inflate_par:k_infp_decode");
  hipMemcpyAsync(back.data(), d_live, (size_t)nl * sizeof(InfpLive), hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipGetLastError(), "inflate_par decode launch") || hip_check(c, hipStreamSynchronize(st), "inflate_par decode")) return ZADA_E_HIP_;
  {
    uint32_t j = 0;
    for (uint32_t k = 0; k < nch; k++) {
      if (!is_live[k]) continue;
      // a distance beyond the bytes written so far (exact, now that the offsets are known), or anything the count did not see
      if (back[j].rule || back[j].end_bit != recs[k].end_bit || (back[j].final != 0) != ((recs[k].flags & INFP_F_FINAL) != 0)) return fall(INFP_DAMAGED);
      j++;
    }
  }
  if (total) {
    if (d64) infp_launch_resolve<9>(c, st, d_live, nl, S->sym.p, (uint8_t *)d_out, d_mark); else infp_launch_resolve<8>(c, st, d_live, nl, S->sym.p, (uint8_t *)d_out, d_mark);
  }
  uint64_t marks = 0;
  uint8_t head[16];
  const uint64_t nhead = total ? std::min<uint64_t>(total, (16u - ((uintptr_t)d_out & 15u)) & 15u) : 0;
  hipMemcpyAsync(&marks, d_mark, 8, hipMemcpyDeviceToHost, st);
  if (nhead) hipMemcpyAsync(head, d_out, nhead, hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipGetLastError(), "inflate_par finish launch") || hip_check(c, hipStreamSynchronize(st), "inflate_par finish")) return ZADA_E_HIP_;
  // the CRC-32 of the output: the head on the host, the rest through the chunked kernels from the first 16-byte boundary
  uint32_t reg = crc_inout ? *crc_inout : 0u;
  reg = infp_crc_bytes(reg, head, (uint32_t)nhead);
  const uint64_t rest = total - nhead, piece = 2ull << 30;
  if (rest) {
    int rc = ensure_crc_workspace(c, rest < piece ? rest : piece);
    if (rc) return rc;
    for (uint64_t o = 0; o < rest; o += piece) {
      const uint64_t k = rest - o < piece ? rest - o : piece;
      if ((rc = crc_launch(c, (const uint8_t *)d_out + nhead + o, k)) || (rc = crc_finish(c, k, &reg))) return rc;
    }
  }
  c->tmark("inflate_par:crc");
  I.marker_bytes = marks;
  if (out_len) *out_len = total;
  if (in_used) *in_used = (recs[W.last].end_bit + 7) / 8;
  if (crc_inout) *crc_inout = reg;
  return 0;
}

// ---- the batch ("inflate_par_batch"): the plan of zada_inflate_par_batch_plan.h between the launches of the k_infpb_* kernels ----
template <int FORMAT> static void infpb_launch_decode(hipStream_t st, const InfpbStream *d_str, InfpbLive *d_live, uint32_t nl, void *sym) {
  hipLaunchKernelGGL(k_infpb_decode<FORMAT>, dim3(nl), dim3(INF_WAVE), 0, st, d_str, d_live, nl, (typename InfpFmt<FORMAT>::sym_t *)sym);
}
template <int FORMAT> static void infpb_launch_resolve(Ctx *c, hipStream_t st, const InfpbStream *d_str, uint32_t ns, const InfpbLive *d_live, uint32_t nl, void *sym, uint64_t *d_mark) {
  typedef typename InfpFmt<FORMAT>::sym_t sym_t;
  hipLaunchKernelGGL(k_infpb_window<FORMAT>, dim3(ns), dim3(INFP_WIN_THREADS), 0, st, d_str, ns, d_live, (sym_t *)sym, d_mark);
  c->tmark("inflate_par_batch:k_infpb_window");
  hipLaunchKernelGGL(k_infpb_finish<FORMAT>, dim3(nl, 8), dim3(INFP_FIN_THREADS), 0, st, d_str, d_live, nl, (const sym_t *)sym, d_mark);
  c->tmark("inflate_par_batch:k_infpb_finish");
}

// One sub-pass: the streams rows [idx [..]] (one format, two chunks or more each).  It synchronises after the scout, after each repair round, after
// the decode and once at the end (inside unzip_sum_entries).  0, or < 0: a HIP error
static int infpb_sub(Ctx *c, InfpState *S, const InfpbIn *rows, InfpbRes *res, const std::vector<uint32_t> &idx, uint32_t format, uint64_t chunk_bytes, zada_inflate_par_info &I) {
  hipStream_t st = c->stream;
  const bool d64 = format == 9;
  InfpbSub B;
  std::vector<InfpbJob> jobs;
  std::vector<InfpbStream> streams;
  std::vector<InfpbLive> lives;
  auto leave = [&]() { infpb_results(B, res); I.scout_rounds += B.launches; return 0; };
  if (!infpb_begin(B, rows, idx, format, chunk_bytes, (uint32_t)c->knob_infp_repair_pct, jobs)) return leave();
  const uint32_t ns = (uint32_t)idx.size(), nch = (uint32_t)B.nchunks;
  // the tables: streams [ns], jobs [nch], records [nch], a round's records [ns] (a stream has one pending job at the most), live rows [nch], the marker counter
  auto up = [](uint64_t v) { return (v + 255) & ~255ull; };
  const uint64_t o_str = 0, o_jobs = o_str + up((uint64_t)ns * sizeof(InfpbStream)), o_recs = o_jobs + up((uint64_t)nch * sizeof(InfpbJob)),
                 o_back = o_recs + up((uint64_t)nch * sizeof(InfpRec)), o_live = o_back + up((uint64_t)ns * sizeof(InfpRec)), o_mark = o_live + up((uint64_t)nch * sizeof(InfpbLive)),
                 total_tabs = o_mark + 16;
  if (dev_grow(c, S->tabs, total_tabs, nullptr)) { infpb_drop(B, INFP_MEMORY); return leave(); }
  const InfpbStream *d_str = (const InfpbStream *)(S->tabs.p + o_str);
  InfpbLive *d_live = (InfpbLive *)(S->tabs.p + o_live);
  uint64_t *d_mark = (uint64_t *)(S->tabs.p + o_mark);
  streams.resize(ns);
  for (uint32_t s = 0; s < ns; s++) { const InfpbIn &R = rows[B.st[s].row]; streams[s] = InfpbStream{R.in, R.n_in, R.out, 0, B.st[s].first, 0, 0, 0}; }
  hipMemcpyAsync(S->tabs.p + o_str, streams.data(), (size_t)ns * sizeof(InfpbStream), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(S->tabs.p + o_jobs, jobs.data(), (size_t)nch * sizeof(InfpbJob), hipMemcpyHostToDevice, st);
  auto scout = [&](uint32_t njobs, InfpRec *d_back) {
    hipLaunchKernelGGL(d64 ? k_infpb_scout<true> : k_infpb_scout<false>, dim3(njobs), dim3(INF_WAVE), 0, st, d_str, chunk_bytes, (const InfpbJob *)(S->tabs.p + o_jobs), njobs,
                       (InfpRec *)(S->tabs.p + o_recs), d_back);
  };
  scout(nch, nullptr);
  c->tmark("inflate_par_batch:k_infpb_scout");
  hipMemcpyAsync(B.recs.data(), S->tabs.p + o_recs, (size_t)nch * sizeof(InfpRec), hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipGetLastError(), "inflate_par_batch scout launch") || hip_check(c, hipStreamSynchronize(st), "inflate_par_batch scout")) return ZADA_E_HIP_;
  B.launches = 1;
  // the chain in rounds: the one pending repair of every stream that asked for one in the same launch, exactly those records back
  std::vector<InfpRec> back(ns);
  for (;;) {
    infpb_round(B, rows, jobs);
    const uint32_t nj = (uint32_t)jobs.size();
    if (!nj) break;
    hipMemcpyAsync(S->tabs.p + o_jobs, jobs.data(), (size_t)nj * sizeof(InfpbJob), hipMemcpyHostToDevice, st);
    scout(nj, (InfpRec *)(S->tabs.p + o_back));
    hipMemcpyAsync(back.data(), S->tabs.p + o_back, (size_t)nj * sizeof(InfpRec), hipMemcpyDeviceToHost, st);
    if (hip_check(c, hipGetLastError(), "inflate_par_batch repair launch") || hip_check(c, hipStreamSynchronize(st), "inflate_par_batch repair")) return ZADA_E_HIP_;
    B.launches++;
    for (uint32_t j = 0; j < nj; j++) B.recs[jobs[j].chunk] = back[j];
  }
  c->tmark("inflate_par_batch:chain");
  const uint64_t nsym = infpb_tables(B, rows, streams, lives);
  const uint32_t nsl = (uint32_t)streams.size(), nl = (uint32_t)lives.size();
  if (!nsl) return leave();
  if (nsym && dev_grow(c, S->sym, nsym * infpb_sym_bytes(format), nullptr)) { infpb_drop(B, INFP_MEMORY); return leave(); }
  // (from here on the stream table holds the chained streams alone, in order: a live row's `stream` is its row of this table, InfpbState::slot)
  hipMemcpyAsync(S->tabs.p + o_str, streams.data(), (size_t)nsl * sizeof(InfpbStream), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(d_live, lives.data(), (size_t)nl * sizeof(InfpbLive), hipMemcpyHostToDevice, st);
  hipMemsetAsync(d_mark, 0, 16, st);
  std::vector<InfpbLive> got(nl);
  if (d64) infpb_launch_decode<9>(st, d_str, d_live, nl, S->sym.p); else infpb_launch_decode<8>(st, d_str, d_live, nl, S->sym.p);
  c->tmark("inflate_par_batch:k_infpb_decode");
  hipMemcpyAsync(got.data(), d_live, (size_t)nl * sizeof(InfpbLive), hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipGetLastError(), "inflate_par_batch decode launch") || hip_check(c, hipStreamSynchronize(st), "inflate_par_batch decode")) return ZADA_E_HIP_;
  // a stream with a row that is not what the count saw leaves before a byte of it is written
  const uint32_t left = infpb_compare(B, got, streams);
  if (left == nsl) return leave();
  if (left) hipMemcpyAsync(S->tabs.p + o_str, streams.data(), (size_t)nsl * sizeof(InfpbStream), hipMemcpyHostToDevice, st);
  if (nsym) {
    if (d64) infpb_launch_resolve<9>(c, st, d_str, nsl, d_live, nl, S->sym.p, d_mark); else infpb_launch_resolve<8>(c, st, d_str, nsl, d_live, nl, S->sym.p, d_mark);
  }
  uint64_t marks = 0;
  hipMemcpyAsync(&marks, d_mark, 8, hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipGetLastError(), "inflate_par_batch finish launch")) return ZADA_E_HIP_;
  // the CRC-32 of every stream that stayed: k_uz_store / k_uz_fold over the bytes in place, parallel inside a stream, one synchronisation for all
  std::vector<uint64_t> at, len;
  std::vector<uint32_t> reg, who;
  for (const InfpbState &T : B.st) {
    if (T.state != INFPB_CHAINED) continue;
    res[T.row].crc = rows[T.row].crc;
    if (!T.W.total) continue;
    at.push_back(rows[T.row].out); len.push_back(T.W.total); reg.push_back(rows[T.row].crc); who.push_back(T.row);
  }
  if (at.empty()) { if (hip_check(c, hipStreamSynchronize(st), "inflate_par_batch finish")) return ZADA_E_HIP_; }
  else {
    const int rc = unzip_sum_entries(c, (uint32_t)at.size(), at.data(), len.data(), reg.data());
    if (rc) return rc < 0 ? rc : ZADA_E_HIP_;
    for (size_t k = 0; k < who.size(); k++) res[who[k]].crc = reg[k];
  }
  c->tmark("inflate_par_batch:crc");
  I.marker_bytes += marks;
  return leave();
}

// The selected entries of one zada_unzip_device group (formats 8 and, where the knob allows them, 9).  res [k].taken: entry k is done; otherwise
// nothing was written to its output range and its register is untouched: the one-wave batch decodes it.  0, or < 0: an error
int inflate_par_batch(Ctx *c, uint32_t n, const InfpbIn *rows, InfpbRes *res) {
  InfpState *S = infp_state(c);
  if (!S) { c->err = "inflate_par: no memory for the state"; return ZADA_E_NOMEM; }
  zada_inflate_par_info I;
  memset(&I, 0, sizeof I);
  const uint64_t chunk_bytes = (uint64_t)c->knob_infp_chunk_kib << 10;
  for (uint32_t k = 0; k < n; k++) {
    res[k] = InfpbRes{0, 0, infpb_chunks(rows[k].n_in, chunk_bytes), 0, 0, rows[k].crc, 0, INFP_SINGLE_CHUNK, 0};      // (what a stream of one chunk leaves; the others: infpb_results)
  }
  std::vector<uint32_t> ends, idx;
  infpb_passes(rows, n, (uint64_t)c->knob_infp_batch_mib << 20, ends);
  c->tmark("inflate_par_batch:begin");
  uint32_t p0 = 0;
  for (uint32_t p1 : ends) {
    for (uint32_t format = 8; format <= 9; format++) {
      idx.clear();
      for (uint32_t k = p0; k < p1; k++) if (rows[k].format == format && res[k].chunks >= 2) idx.push_back(k);
      if (idx.empty()) continue;
      const int rc = infpb_sub(c, S, rows, res, idx, format, chunk_bytes, I);
      if (rc < 0) return rc;
    }
    p0 = p1;
  }
  uint64_t sum[6];
  infpb_sum(res, n, sum);
  I.chunks = sum[0]; I.live_chunks = sum[1]; I.repairs = sum[2]; I.fell_back = (int32_t)sum[3]; I.reason = (int32_t)sum[4]; I.streams = sum[5];
  S->last = I;
  return 0;
}

// zada_unzip_device sums the records of a call's entries
void inflate_par_record(Ctx *c, zada_inflate_par_info *get, const zada_inflate_par_info *set) {
  InfpState *S = infp_state(c);
  if (!S) return;
  if (get) *get = S->last;
  if (set) S->last = *set;
}

}  // namespace zada

using namespace zada;

static constexpr uint64_t INFP_MAX_BYTES = 1ull << 40;

int zada_inflate_par_device(zada_ctx *z, int format, const void *d_in, uint64_t n_in, void *d_out, uint64_t cap, uint64_t *out_len, uint64_t *in_used,
                            uint32_t *crc_inout) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (format != 8 && format != 9) { c->err = "zada_inflate_par_device: format must be 8 (Deflate) or 9 (Deflate64)"; return ZADA_E_INVALID; }
  if ((n_in && !d_in) || (cap && !d_out)) { c->err = "zada_inflate_par_device: null buffer"; return ZADA_E_INVALID; }
  if (n_in >= INFP_MAX_BYTES || cap >= INFP_MAX_BYTES) { c->err = "zada_inflate_par_device: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  if (out_len) *out_len = 0;
  if (in_used) *in_used = 0;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  c->tbegin();
  const int rc = inflate_par_try(c, format, d_in, n_in, d_out, cap, out_len, in_used, crc_inout);
  c->tend();
  if (rc < 0) { hipStreamSynchronize(c->stream); (void)hipGetLastError(); return rc; }
  if (rc == 0) return ZADA_OK;
  return zada_inflate_device(z, format, d_in, n_in, d_out, cap, out_len, in_used, crc_inout);      // the one wave: its verdict, its text
}

int zada_inflate_par(zada_ctx *z, int format, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used, uint32_t *crc_inout) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (format != 8 && format != 9) { c->err = "zada_inflate_par: format must be 8 (Deflate) or 9 (Deflate64)"; return ZADA_E_INVALID; }
  if ((n_in && !in) || (cap && !out)) { c->err = "zada_inflate_par: null buffer"; return ZADA_E_INVALID; }
  if (n_in >= INFP_MAX_BYTES || cap >= INFP_MAX_BYTES) { c->err = "zada_inflate_par: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  if (out_len) *out_len = 0;
  if (in_used) *in_used = 0;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  // the stream and the output in one device buffer of the call's own, every part at a multiple of 16 (pageable copies: no pinned staging here)
  const uint64_t a = (n_in + 15) & ~15ull;
  uint8_t *d = nullptr;
  if (hipMalloc((void **)&d, a + cap + 16) != hipSuccess) { (void)hipGetLastError(); c->err = "hipMalloc (inflate_par buffers)"; return ZADA_E_NOMEM; }
  uint64_t ol = 0, iu = 0;
  uint32_t reg = crc_inout ? *crc_inout : 0u;
  int rc = ZADA_OK;
  if (n_in && hip_check(c, hipMemcpy(d, in, n_in, hipMemcpyHostToDevice), "inflate_par copy in")) rc = ZADA_E_HIP;
  if (!rc) rc = zada_inflate_par_device(z, format, d, n_in, d + a, cap, &ol, &iu, &reg);
  if (!rc && ol && hip_check(c, hipMemcpy(out, d + a, ol, hipMemcpyDeviceToHost), "inflate_par copy out")) rc = ZADA_E_HIP;
  hipFree(d);
  if (rc) return rc;
  if (out_len) *out_len = ol;
  if (in_used) *in_used = iu;
  if (crc_inout) *crc_inout = reg;
  return ZADA_OK;
}

int zada_inflate_par_last(zada_ctx *z, zada_inflate_par_info *info) {
  if (!z || !info) return ZADA_E_INVALID;
  InfpState *S = (InfpState *)z->c.infp;
  if (S) *info = S->last; else memset(info, 0, sizeof *info);
  return ZADA_OK;
}
