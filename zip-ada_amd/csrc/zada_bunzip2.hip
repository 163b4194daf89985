// zada_bunzip2.hip -- BZip2.Decoding.Decompress (bzip2-decoding.adb) for a batch of entries: the unit of work is the BLOCK, not the entry.
//
// A BZip2 block starts with a 48-bit magic and is independent of every other block, so one stream of three hundred blocks and ten thousand
// entries of one block each run through the same launches:
//   k_bzd_scan     every bit position of every entry's stream against the block and the footer magic: candidates
//   k_bzd_block    one wave per candidate: header, tables, Huffman / MTF chain (zada_bunzip2_logic.h, the chain on the scalar side), RUNA / RUNB
//                  runs filled by all lanes -> the block's last column in its slot, the 256 counts, a record
//   (host)         chain resolve: from bit 32 of each entry, end bit -> candidate; candidates the chain never reaches are dropped
//   k_bzd_hist / k_bzd_offsets / k_bzd_scatter   cf_tab and the stable scatter of BWT_Detransform as one stable 8-bit counting-sort pass
//   k_bzd_walk1 / k_bzd_rank / k_bzd_walk2       the chase as a walk along a permutation between splitters (every 64th index and the origin)
//   k_bzd_rle_a / k_bzd_rle_b / k_bzd_rle_fill   RLE_1 as a five-state machine over pieces of 256 bytes: lengths, prefix, fill
//   k_bzd_crc      bzip2's CRC of every block's output, strip by strip; the entries' Zip CRC-32 comes from k_inf_crc (zada_inflate.hip)
// Plain C++ and vector stores only.  Every index that comes from the stream is compared with its array before it is used.
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
#include "zada_bunzip2_logic.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {

constexpr uint32_t BZD_WAVE = 64;
constexpr uint32_t BZD_STAGE = 2048;                 // bytes of compressed input in LDS at a time
constexpr uint32_t BZD_SC = 2048;                    // positions of a block per counting-sort chunk (one wave)
constexpr uint32_t BZD_SPLIT = 64;                   // every BZD_SPLIT-th index of a block is a splitter of the walk
constexpr uint32_t BZD_RC = 256;                     // bytes behind the inverse BWT per RLE_1 piece (one lane)
constexpr uint32_t BZD_NONE = 0xFFFFFFFFu;
constexpr uint64_t BZD_M48 = (1ull << 48) - 1;

struct BzdJob { uint64_t in, out, n_in, cap; };
struct BzdCand { uint32_t entry, kind; uint64_t bit; };                        // kind 0: block magic, 1: footer magic
struct BzdRec { int32_t rc; uint32_t rule, nsym, origin, stored_crc, kind; uint64_t end_bit, fail_bit; };
// a block of the chain on its way through the stages behind k_bzd_block
struct BzdBlk {
  uint64_t L_off, sym0, out;          // its slot; where its symbols begin in tt / T; where its output goes
  uint32_t n, origin, cand, chunk0, split0, rchunk0;
  uint32_t out_len, period, crc, skip;
};

typedef __attribute__((address_space(1))) uint8_t gu8;
typedef __attribute__((address_space(1))) const uint8_t gcu8;

// ---- candidates ----
__global__ void __launch_bounds__(256) k_bzd_scan(const BzdJob *__restrict__ jobs, const uint64_t *__restrict__ boff, uint32_t E, uint64_t total, BzdCand *cand, uint32_t cap,
                                                  uint32_t *counter, uint32_t *hdr) {
  for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256) {
    uint32_t lo = 0, hi = E - 1;                                     // the entry of byte g: the first one that ends behind it
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (boff[mid + 1] > g) hi = mid; else lo = mid + 1; }
    const uint32_t e = lo;
    const uint64_t p = g - boff[e], n = jobs[e].n_in;
    const uint8_t *in = (const uint8_t *)jobs[e].in;
    uint64_t w = 0;                                                  // the 64-bit window at byte p, confined to [0, n_in) of the entry
    for (uint32_t k = 0; k < 8; k++) if (p + k < n) w |= (uint64_t)in[p + k] << (56 - 8 * k);
    if (p == 0) hdr[e] = (uint32_t)(w >> 32);
    for (uint32_t o = 0; o < 8; o++) {
      if (p * 8 + o + 48 > n * 8) break;
      const uint64_t v = (w >> (16 - o)) & BZD_M48;
      if (v == BZD_BLOCK_MAGIC || v == BZD_FOOTER_MAGIC) {
        const uint32_t at = atomicAdd(counter, 1u);
        if (at < cap) cand[at] = BzdCand{e, v == BZD_FOOTER_MAGIC ? 1u : 0u, p * 8 + o};
      }
    }
  }
}

// ---- the bit reader of a wave: the input staged in LDS as big-endian words, 32 bits at a time into a 64-bit register pair ----
struct BzdWaveReader {
  gcu8 *in; uint64_t n, ip, base; uint64_t hold; uint32_t nb; uint32_t *stage;        // stage: BZD_STAGE / 4 + 2 words; input bytes [base, base + BZD_STAGE)
  __device__ __forceinline__ void fill(uint64_t at) {
    __syncthreads();
    base = at;
    for (uint32_t w = threadIdx.x; w < BZD_STAGE / 4 + 2; w += BZD_WAVE) {
      const uint64_t o = at + (uint64_t)w * 4;
      uint32_t v = 0;
      if (o + 4 <= n) v = (uint32_t)in[o] << 24 | (uint32_t)in[o + 1] << 16 | (uint32_t)in[o + 2] << 8 | (uint32_t)in[o + 3];
      else for (uint32_t k = 0; k < 4; k++) if (o + k < n) v |= (uint32_t)in[o + k] << (24 - 8 * k);
      stage[w] = v;
    }
    __syncthreads();
  }
  __device__ __forceinline__ void need32() {
    if (nb > 32) return;
    if (ip < base || ip + 4 > base + BZD_STAGE) fill(ip & ~3ull);
    const uint32_t o = (uint32_t)(ip - base);
    const uint32_t w0 = ZBZD_UNI(stage[o >> 2]), w1 = ZBZD_UNI(stage[(o >> 2) + 1]);
    const uint32_t w = (uint32_t)((((uint64_t)w0 << 32) | w1) >> (32u - (o & 3u) * 8u));
    hold |= (uint64_t)w << (32 - nb); nb += 32; ip += 4;
  }
  __device__ __forceinline__ uint32_t bits(uint32_t k) { need32(); const uint32_t v = (uint32_t)(hold >> (64 - k)); hold <<= k; nb -= k; return v; }
  __device__ __forceinline__ void open(gcu8 *p, uint64_t len, uint64_t bit, uint32_t *st) {
    in = p; n = len; stage = st; hold = 0; nb = 0; ip = bit >> 3;
    fill(ip & ~3ull);
    if (bit & 7u) (void)bits((uint32_t)(bit & 7u));
  }
  __device__ __forceinline__ uint64_t used_bits() const { return ip * 8 - nb; }
  __device__ __forceinline__ bool overrun() const { return used_bits() > n * 8; }
};

// the last column on its way to the slot: lane q keeps symbol q of up to 64, a run is filled by all lanes
struct BzdWaveSink {
  gu8 *slot; uint32_t qpos, q, my;
  __device__ __forceinline__ void flush() { if (threadIdx.x < q) slot[qpos + threadIdx.x] = (uint8_t)my; qpos += q; q = 0; }
  __device__ __forceinline__ void put(uint32_t uc, uint32_t) { if (threadIdx.x == q) my = uc; if (++q == BZD_WAVE) flush(); }
  __device__ __forceinline__ void run(uint32_t uc, uint32_t at, uint32_t es) {
    flush();
    for (uint32_t i = threadIdx.x; i < es; i += BZD_WAVE) slot[at + i] = (uint8_t)uc;
    qpos = at + es;
  }
};

__global__ void __launch_bounds__(BZD_WAVE) k_bzd_block(const BzdJob *__restrict__ jobs, const BzdCand *__restrict__ cand, const uint32_t *__restrict__ order,
                                                        const uint64_t *__restrict__ slot_off, const uint32_t *__restrict__ slot_cap, uint32_t count, uint32_t *counter,
                                                        uint8_t *slots, uint32_t *counts, BzdRec *rec) {
  __shared__ BzdTables T;
  __shared__ uint32_t stage[BZD_STAGE / 4 + 2];
  __shared__ uint32_t next_s;
  const uint32_t lane = threadIdx.x;
  for (;;) {
    __syncthreads();
    if (lane == 0) next_s = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t at = ZBZD_UNI(next_s);
    if (at >= count) break;
    const uint32_t c = order[at];
    const BzdCand C = cand[c];
    const BzdJob J = jobs[C.entry];
    gcu8 *in = (gcu8 *)J.in;
    BzdWaveReader br;
    br.open(in, J.n_in, C.bit + 48, stage);
    BzdRec R;
    R.rc = 0; R.rule = 0; R.nsym = 0; R.origin = 0; R.stored_crc = 0; R.kind = C.kind; R.end_bit = 0; R.fail_bit = 0;
    if (C.kind == 1) {
      uint32_t crc = br.bits(16) << 16;
      crc |= br.bits(16);
      R.stored_crc = crc;
      if (br.overrun()) R.rule = BZD_R_TRUNCATED;
    } else {
      const uint32_t level = ZBZD_UNI((uint32_t)in[3]) - (uint32_t)'0';                 // (the host has seen BZh1 .. BZh9 before it lists a candidate)
      BzdWaveSink sink{(gu8 *)(slots + slot_off[c]), 0, 0, 0};
      BzdBlockHdr H{};
      uint32_t n = 0;
      R.rule = bzd_block(br, T, level, slot_cap[c], sink, H, n, lane, BZD_WAVE);
      if (!R.rule) sink.flush();
      __syncthreads();
      for (uint32_t i = lane; i < 256; i += BZD_WAVE) counts[(uint64_t)c * 256 + i] = T.counts[i];
      R.nsym = n; R.origin = H.origin; R.stored_crc = H.stored_crc;
    }
    R.rc = R.rule ? BZD_E_DATA : 0;
    R.end_bit = br.used_bits(); R.fail_bit = br.used_bits();
    if (lane == 0) rec[c] = R;
  }
}

// ---- the stages behind the chain: every kernel finds the block of its piece of work by a search over the blocks' first pieces ----
#define BZD_FIND(field)                                                                                      \
  uint32_t lo = 0, hi = nb - 1;                                                                              \
  while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (blk[mid].field <= idx) lo = mid; else hi = mid - 1; } \
  return lo;
__device__ __forceinline__ uint32_t bzd_find_chunk(const BzdBlk *blk, uint32_t nb, uint32_t idx) { BZD_FIND(chunk0) }
__device__ __forceinline__ uint32_t bzd_find_split(const BzdBlk *blk, uint32_t nb, uint32_t idx) { BZD_FIND(split0) }
__device__ __forceinline__ uint32_t bzd_find_rchunk(const BzdBlk *blk, uint32_t nb, uint32_t idx) { BZD_FIND(rchunk0) }

__global__ void __launch_bounds__(BZD_WAVE) k_bzd_hist(const BzdBlk *__restrict__ blk, uint32_t nb, const uint8_t *__restrict__ slots, uint32_t *hist) {
  __shared__ uint32_t h[256];
  const uint32_t ch = blockIdx.x, lane = threadIdx.x;
  const uint32_t b = bzd_find_chunk(blk, nb, ch);
  const BzdBlk B = blk[b];
  const uint8_t *L = slots + B.L_off;
  const uint32_t p0 = (ch - B.chunk0) * BZD_SC, p1 = p0 + BZD_SC < B.n ? p0 + BZD_SC : B.n;
  for (uint32_t i = lane; i < 256; i += BZD_WAVE) h[i] = 0;
  __syncthreads();
  for (uint32_t p = p0 + lane; p < p1; p += BZD_WAVE) atomicAdd(&h[L[p]], 1u);
  __syncthreads();
  for (uint32_t i = lane; i < 256; i += BZD_WAVE) hist[(uint64_t)ch * 256 + i] = h[i];
}

// Setup_Table, and where every chunk's bytes of a value begin: one workgroup per block, one thread per byte value
__global__ void __launch_bounds__(256) k_bzd_offsets(const BzdBlk *__restrict__ blk, const uint32_t *__restrict__ counts, uint32_t *hist) {
  __shared__ uint32_t cnt[256];
  const BzdBlk B = blk[blockIdx.x];
  const uint32_t c = threadIdx.x;
  cnt[c] = counts[(uint64_t)B.cand * 256 + c];
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t i = 0; i < c; i++) run += cnt[i];
  const uint32_t nch = (B.n + BZD_SC - 1) / BZD_SC;
  for (uint32_t k = 0; k < nch; k++) {
    uint32_t *h = hist + (uint64_t)(B.chunk0 + k) * 256 + c;
    const uint32_t t = *h;
    *h = run;
    run += t;
  }
}

// BWT_Detransform: tt [cf [L [p]] ++] = p, stable -- one wave per chunk, 64 positions at a time, equal bytes ranked by ballots.  The word written at
// sorted place r is (p << 8) | F [r]: F [r] = L [p] is the byte the chase delivers when it stands at r.
__global__ void __launch_bounds__(BZD_WAVE) k_bzd_scatter(const BzdBlk *__restrict__ blk, uint32_t nb, const uint8_t *__restrict__ slots, const uint32_t *__restrict__ hist,
                                                          uint32_t *tt) {
  __shared__ uint32_t ctr[256];
  const uint32_t ch = blockIdx.x, lane = threadIdx.x;
  const uint32_t b = bzd_find_chunk(blk, nb, ch);
  const BzdBlk B = blk[b];
  const uint8_t *L = slots + B.L_off;
  uint32_t *t = tt + B.sym0;
  const uint32_t p0 = (ch - B.chunk0) * BZD_SC, p1 = p0 + BZD_SC < B.n ? p0 + BZD_SC : B.n;
  for (uint32_t i = lane; i < 256; i += BZD_WAVE) ctr[i] = hist[(uint64_t)ch * 256 + i];
  __syncthreads();
  for (uint32_t s = p0; s < p1; s += BZD_WAVE) {
    const uint32_t p = s + lane;
    const bool active = p < p1;
    const uint32_t c = active ? L[p] : 0u;
    uint64_t mask = __ballot(active);
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
      const bool bit = (c >> k) & 1u;
      const uint64_t bk = __ballot(bit);
      mask &= bit ? bk : ~bk;
    }
    const uint32_t rank = __popcll(mask & ((1ull << lane) - 1ull));
    const uint32_t base = ctr[c];
    const uint32_t r = base + rank;
    if (active && r < B.n) t[r] = (p << 8) | c;
    __syncthreads();
    if (active && (mask >> lane) == 1ull) ctr[c] = base + (uint32_t)__popcll(mask);
    __syncthreads();
  }
}

// The chase is a walk along the permutation r -> tt [r] >> 8 from the origin.  Splitters: every 64th index, and the origin.  One lane per splitter
// walks to the next splitter: length and successor.  (A hostile permutation makes one lane walk a whole cycle; never more than n steps.)
__global__ void __launch_bounds__(256) k_bzd_walk1(const BzdBlk *__restrict__ blk, uint32_t nb, uint32_t nsplit, const uint32_t *__restrict__ tt, uint32_t *seg_len,
                                                   uint32_t *seg_succ, uint32_t *rank) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nsplit) return;
  const uint32_t b = bzd_find_split(blk, nb, s);
  const BzdBlk B = blk[b];
  const uint32_t *t = tt + B.sym0;
  const uint32_t id = s - B.split0, S = (B.n + BZD_SPLIT - 1) / BZD_SPLIT;
  uint32_t cur = id == S ? B.origin : id * BZD_SPLIT, len = 0, succ = S;
  if (cur < B.n) {
    do {
      cur = t[cur] >> 8;
      len++;
      if (cur >= B.n) break;
    } while (!(cur % BZD_SPLIT == 0 || cur == B.origin) && len < B.n);
    if (cur < B.n && cur != B.origin) succ = cur / BZD_SPLIT;
  }
  seg_len[s] = len; seg_succ[s] = succ; rank[s] = BZD_NONE;
}

// The splitters in the order the chase meets them, from the origin: one lane per block over a few thousand splitters.  A permutation with several
// cycles brings the walk back to the origin before n steps: the serial chase then goes round that cycle again, so the output has its period.
__global__ void __launch_bounds__(BZD_WAVE) k_bzd_rank(BzdBlk *blk, uint32_t nb, const uint32_t *__restrict__ seg_len, const uint32_t *__restrict__ seg_succ, uint32_t *rank) {
  const uint32_t b = blockIdx.x * BZD_WAVE + threadIdx.x;
  if (b >= nb) return;
  const BzdBlk B = blk[b];
  const uint32_t S = (B.n + BZD_SPLIT - 1) / BZD_SPLIT;
  uint32_t cur = S, r = 0;
  for (uint32_t it = 0; it <= S && r < B.n; it++) {
    const uint32_t s = B.split0 + cur;
    if (rank[s] != BZD_NONE) break;
    rank[s] = r;
    const uint32_t len = seg_len[s];
    if (len == 0) break;
    r += len;
    cur = seg_succ[s];
    if (cur > S) break;
  }
  blk[b].period = r < B.n ? (r ? r : 1u) : B.n;
}

// ... and every ranked splitter's stretch again, each byte written at its rank (and at every period behind it)
__global__ void __launch_bounds__(256) k_bzd_walk2(const BzdBlk *__restrict__ blk, uint32_t nb, uint32_t nsplit, const uint32_t *__restrict__ tt,
                                                   const uint32_t *__restrict__ seg_len, const uint32_t *__restrict__ rank, uint8_t *T) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nsplit) return;
  const uint32_t r0 = rank[s];
  if (r0 == BZD_NONE) return;
  const uint32_t b = bzd_find_split(blk, nb, s);
  const BzdBlk B = blk[b];
  const uint32_t *t = tt + B.sym0;
  uint8_t *o = T + B.sym0;
  const uint32_t id = s - B.split0, S = (B.n + BZD_SPLIT - 1) / BZD_SPLIT, len = seg_len[s];
  uint32_t cur = id == S ? B.origin : id * BZD_SPLIT;
  for (uint32_t k = 0; k < len && cur < B.n; k++) {
    const uint32_t w = t[cur];
    for (uint64_t q = (uint64_t)r0 + k; q < B.n; q += B.period) o[q] = (uint8_t)w;
    cur = w >> 8;
  }
}

// RLE_1, first pass: every piece of 256 bytes from each of the five states it may be entered in -> output length and state behind it
__global__ void __launch_bounds__(256) k_bzd_rle_a(const BzdBlk *__restrict__ blk, uint32_t nb, uint32_t nrc, const uint8_t *__restrict__ T, uint32_t *rle_len, uint8_t *rle_exit) {
  const uint32_t rc = blockIdx.x * 256 + threadIdx.x;
  if (rc >= nrc) return;
  const uint32_t b = bzd_find_rchunk(blk, nb, rc);
  const BzdBlk B = blk[b];
  const uint8_t *t = T + B.sym0;
  const uint32_t a = (rc - B.rchunk0) * BZD_RC, e = a + BZD_RC < B.n ? a + BZD_RC : B.n;
  uint32_t st[5] = {0, 1, 2, 3, 4}, len[5] = {0, 0, 0, 0, 0};
  uint32_t old = a ? t[a - 1] : 0u;
  for (uint32_t i = a; i < e; i++) {
    const uint32_t d = t[i];
#pragma unroll
    for (int j = 0; j < 5; j++) len[j] += bzd_rle_step(st[j], old, d);
    old = d;
  }
#pragma unroll
  for (int j = 0; j < 5; j++) { rle_len[(uint64_t)rc * 5 + j] = len[j]; rle_exit[(uint64_t)rc * 5 + j] = (uint8_t)st[j]; }
}

// ... the pieces of a block in order: the state every piece is entered in, where its output begins, the block's output length
__global__ void __launch_bounds__(BZD_WAVE) k_bzd_rle_b(BzdBlk *blk, uint32_t nb, const uint32_t *__restrict__ rle_len, const uint8_t *__restrict__ rle_exit, uint8_t *rle_entry,
                                                        uint32_t *rle_off) {
  const uint32_t b = blockIdx.x * BZD_WAVE + threadIdx.x;
  if (b >= nb) return;
  const BzdBlk B = blk[b];
  const uint32_t nrc = (B.n + BZD_RC - 1) / BZD_RC;
  uint32_t state = 0;
  uint64_t off = 0;
  for (uint32_t k = 0; k < nrc; k++) {
    const uint64_t rc = (uint64_t)B.rchunk0 + k;
    rle_entry[rc] = (uint8_t)state;
    rle_off[rc] = (uint32_t)off;
    off += rle_len[rc * 5 + state];
    state = rle_exit[rc * 5 + state];
  }
  blk[b].out_len = (uint32_t)off;                     // (at most 900 000 / 5 x 259 bytes)
}

// ... and the fill, once the host has compared the entries' sums with their caps and said where every block's output goes
__global__ void __launch_bounds__(256) k_bzd_rle_fill(const BzdBlk *__restrict__ blk, uint32_t nb, uint32_t nrc, const uint8_t *__restrict__ T,
                                                      const uint8_t *__restrict__ rle_entry, const uint32_t *__restrict__ rle_off) {
  const uint32_t rc = blockIdx.x * 256 + threadIdx.x;
  if (rc >= nrc) return;
  const uint32_t b = bzd_find_rchunk(blk, nb, rc);
  const BzdBlk B = blk[b];
  if (B.skip) return;
  const uint8_t *t = T + B.sym0;
  const uint32_t a = (rc - B.rchunk0) * BZD_RC, e = a + BZD_RC < B.n ? a + BZD_RC : B.n;
  uint32_t state = rle_entry[rc], old = a ? t[a - 1] : 0u;
  uint64_t off = rle_off[rc];
  uint8_t *out = (uint8_t *)B.out;
  for (uint32_t i = a; i < e; i++) {
    const uint32_t d = t[i];
    const uint32_t by = state == 4 ? old : d;
    const uint32_t m = bzd_rle_step(state, old, d);
    for (uint32_t k = 0; k < m && off + k < B.out_len; k++) out[off + k] = (uint8_t)by;
    off += m;
    old = d;
  }
}

// ---- bzip2's CRC of every block's output, one wave per block: the strips of k_inf_crc with the byte step and the operators of the other CRC ----
constexpr uint32_t BC_SUB = 256, BC_ROW = BC_SUB + 16, BC_TILE = BZD_WAVE * BC_SUB;
struct BzdCrcOps { uint32_t mat[6][32]; };             // operator j: the register over 256 << j zero bytes

__device__ __forceinline__ uint32_t bc_gf2(const uint32_t *m, uint32_t v) {
  uint32_t s = 0;
#pragma unroll
  for (int b = 0; b < 32; b++) s ^= (0u - ((v >> b) & 1u)) & m[b];
  return s;
}
__device__ __forceinline__ uint32_t bc_bytes(const uint8_t *row, uint32_t len, const uint32_t *tab, uint32_t r) {
  for (uint32_t i = 0; i < len; i++) r = (r << 8) ^ tab[(r >> 24) ^ row[i]];
  return r;
}

__global__ void __launch_bounds__(BZD_WAVE) k_bzd_crc(BzdBlk *blk, const BzdCrcOps *__restrict__ ops) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t m[6][32];
  __shared__ __attribute__((aligned(16))) uint8_t rows[BZD_WAVE * BC_ROW];
  const uint32_t lane = threadIdx.x;
  const BzdBlk B = blk[blockIdx.x];
  if (B.skip) return;
  for (uint32_t t = lane; t < 256; t += BZD_WAVE) tab[t] = bzd_crc_byte(0u, t);
  for (uint32_t t = lane; t < 6 * 32; t += BZD_WAVE) m[t >> 5][t & 31] = ops->mat[t >> 5][t & 31];
  const uint64_t n = B.out_len;
  const uint8_t *buf = (const uint8_t *)B.out;
  uint32_t reg = 0xFFFFFFFFu;
  for (uint64_t s0 = 0; s0 < n; s0 += BC_TILE) {
    const uint32_t left = n - s0 < BC_TILE ? (uint32_t)(n - s0) : BC_TILE;
    __syncthreads();
    for (uint32_t o = lane; o < left; o += BZD_WAVE) rows[(o / BC_SUB) * BC_ROW + (o % BC_SUB)] = buf[s0 + o];
    __syncthreads();
    const uint32_t o = lane * BC_SUB;
    const uint32_t len = o >= left ? 0u : left - o < BC_SUB ? left - o : BC_SUB;
    const uint8_t *row = rows + lane * BC_ROW;
    uint32_t v = bc_bytes(row, len, tab, 0u);
    if (lane == 0) v ^= bc_gf2(m[0], reg);
    for (int j = 0; j < 6; j++) {
      const uint32_t u = __shfl_up(v, 1u << j, 64);
      if (lane >= (1u << j)) v ^= bc_gf2(m[j], u);
    }
    uint32_t before = __shfl_up(v, 1u, 64);
    if (lane == 0) before = reg;
    const uint32_t last = (left - 1) / BC_SUB;
    uint32_t after = 0;
    if (lane == last) after = bc_bytes(row, len, tab, before);
    reg = (uint32_t)__shfl((int)after, (int)last, 64);
  }
  if (lane == 0) blk[blockIdx.x].crc = ~reg;
}

// ---- host side ----
struct BzdState : ReaderState {           // (tabs: jobs and offsets; last_entries: rule, block, bit, blocks of its chain)
  BzdCrcOps *d_ops = nullptr;
  DevBuf cands, wa, wb;                   // candidates; a round's slots and records; a round's later stages
  std::vector<uint64_t> last_blocks;      // the last call, per block of a chain, in order: entry, symbols, origin, stored CRC, end bit (zada_bunzip2_last_records)
};

static BzdState *bzd_state(Ctx *c) {
  if (c->bzd) return (BzdState *)c->bzd;
  BzdState *S = new (std::nothrow) BzdState();
  if (!S) return nullptr;
  BzdCrcOps h;
  {
    uint32_t op[32], sq[32];
    for (int i = 0; i < 32; i++) { const uint32_t r = 1u << i; op[i] = (r << 8) ^ bzd_crc_byte(0u, r >> 24); }                      // one zero byte
    auto square = [&] { for (int i = 0; i < 32; i++) { uint32_t v = op[i], s = 0; for (int j = 0; v; j++, v >>= 1) if (v & 1) s ^= op[j]; sq[i] = s; } memcpy(op, sq, sizeof op); };
    for (int k = 0; k < 8; k++) square();                                                                                            // 256 bytes
    for (int j = 0; j < 6; j++) { memcpy(h.mat[j], op, sizeof op); square(); }
  }
  if (hipMalloc((void **)&S->d_ops, sizeof(BzdCrcOps)) != hipSuccess || hipMalloc((void **)&S->d_counter, 64) != hipSuccess ||
      hipMemcpy(S->d_ops, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (S->d_ops) hipFree(S->d_ops);
    if (S->d_counter) hipFree(S->d_counter);
    delete S;
    return nullptr;
  }
  c->bzd = S;
  return S;
}
void bunzip2_destroy(Ctx *c) {
  BzdState *S = (BzdState *)c->bzd;
  if (!S) return;
  for (DevBuf *b : {&S->tabs, &S->cands, &S->wa, &S->wb, &S->arena}) dev_free(*b);
  hipFree(S->d_ops); hipFree(S->d_counter);
  delete S;
  c->bzd = nullptr;
}
// pieces of one device buffer, each at a multiple of 256
struct BzdCarve {
  uint64_t at = 0;
  uint64_t take(uint64_t bytes) { const uint64_t o = at; at += (bytes + 255) & ~255ull; return o; }
};

// what the host keeps per entry while the rounds go by
struct BzdEnt {
  uint32_t level = 0;
  int status = 0;                     // 0: its chain is open; 1: done; 2: failed
  uint32_t rule = 0, block = 0, comb = 0;
  uint64_t fail_bit = 0, pos = 32, out_off = 0, in_used = 0;
  // what the chain met in the round at hand, to be settled behind the round's later stages
  int ev = 0;                         // 0: nothing; 1: the footer; 2: a block that failed in k_bzd_block (or no magic)
  uint32_t ev_rule = 0, ev_block = 0, ev_crc = 0;
  uint64_t ev_bit = 0, ev_end = 0;
  // the first block of the round that failed in a later stage
  uint32_t st_rule = 0, st_block = 0;
  uint64_t st_bit = 0;
};
struct BzdBlkHost { uint32_t entry, block; uint64_t end_bit; uint32_t stored_crc; };

static void bzd_fail(BzdEnt &e, uint32_t rule, uint32_t block, uint64_t bit) { e.status = 2; e.rule = rule; e.block = block; e.fail_bit = bit; }
// no candidate at the bit where a block has to begin
static void bzd_no_magic(BzdEnt &e, const BzdJob &J) {
  e.ev = 2; e.ev_rule = e.pos + 48 > J.n_in * 8 ? BZD_R_TRUNCATED : BZD_R_BLOCK_MAGIC; e.ev_block = e.block; e.ev_bit = e.pos;
}

#define BZD_HIP(call, what) do { if (hip_check(c, (call), what)) return ZADA_E_HIP_; } while (0)

// E jobs (device addresses) through the launches; res [E] receives the records
static int bzd_run(Ctx *c, BzdState *S, const std::vector<BzdJob> &jobs, const uint32_t *crc_in, std::vector<BzdResult> &res, uint32_t entry0) {
  const uint32_t E = (uint32_t)jobs.size();
  res.assign(E, BzdResult{});
  if (E == 0) return 0;
  hipStream_t st = c->stream;
  std::vector<uint64_t> boff(E + 1, 0);
  for (uint32_t i = 0; i < E; i++) boff[i + 1] = boff[i] + jobs[i].n_in;
  const uint64_t total = boff[E];
  std::vector<BzdEnt> ent(E);
  std::vector<BzdCand> cand;
  std::vector<uint32_t> hdr(E, 0);
  BzdCarve tc;
  const uint64_t o_jobs = tc.take((uint64_t)E * sizeof(BzdJob)), o_boff = tc.take((uint64_t)(E + 1) * 8), o_hdr = tc.take((uint64_t)E * 4);
  int rc = dev_grow(c, S->tabs, tc.at, "hipMalloc (bunzip2 tables)");
  if (rc) return rc;
  const BzdJob *d_jobs = (const BzdJob *)(S->tabs.p + o_jobs);
  hipMemcpyAsync(S->tabs.p + o_jobs, jobs.data(), (size_t)E * sizeof(BzdJob), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(S->tabs.p + o_boff, boff.data(), (size_t)(E + 1) * 8, hipMemcpyHostToDevice, st);
  hipMemsetAsync(S->tabs.p + o_hdr, 0, (size_t)E * 4, st);
  c->tmark("bunzip2:begin");
  if (total) {
    uint64_t cap = total / 32 + 4ull * E + 1024;
    for (int attempt = 0; attempt < 2; attempt++) {
      if (cap >= (1ull << 32)) { c->err = "bunzip2: too many block candidates"; return ZADA_E_TOO_LARGE; }
      rc = dev_grow(c, S->cands, cap * sizeof(BzdCand), "hipMalloc (bunzip2 candidates)");
      if (rc) return rc;
      hipMemsetAsync(S->d_counter, 0, 4, st);
      const uint64_t wgs = (total + 255) / 256;
      hipLaunchKernelGGL(k_bzd_scan, dim3((uint32_t)(wgs < 4096 ? wgs : 4096)), dim3(256), 0, st, d_jobs, (const uint64_t *)(S->tabs.p + o_boff), E, total,
                         (BzdCand *)S->cands.p, (uint32_t)cap, S->d_counter, (uint32_t *)(S->tabs.p + o_hdr));
      uint32_t found = 0;
      hipMemcpyAsync(&found, S->d_counter, 4, hipMemcpyDeviceToHost, st);
      BZD_HIP(hipGetLastError(), "bunzip2 scan launch");
      BZD_HIP(hipStreamSynchronize(st), "bunzip2 scan");
      if (found <= cap) {
        cand.resize(found);
        if (found) hipMemcpyAsync(cand.data(), S->cands.p, (size_t)found * sizeof(BzdCand), hipMemcpyDeviceToHost, st);
        hipMemcpyAsync(hdr.data(), S->tabs.p + o_hdr, (size_t)E * 4, hipMemcpyDeviceToHost, st);
        BZD_HIP(hipStreamSynchronize(st), "bunzip2 candidates");
        break;
      }
      if (attempt == 1) { c->err = "bunzip2: the candidate count changed between two scans"; return ZADA_E_HIP_; }
      cap = found;
    }
  }
  c->tmark("bunzip2:k_bzd_scan");
  // per-entry candidate lists in bit order; stream headers
  std::sort(cand.begin(), cand.end(), [](const BzdCand &a, const BzdCand &b) { return a.entry != b.entry ? a.entry < b.entry : a.bit < b.bit; });
  for (uint32_t i = 0; i < E; i++) {
    const uint8_t h[4] = {(uint8_t)(hdr[i] >> 24), (uint8_t)(hdr[i] >> 16), (uint8_t)(hdr[i] >> 8), (uint8_t)hdr[i]};
    const uint32_t rule = bzd_stream_header(h, jobs[i].n_in, ent[i].level);
    if (rule) bzd_fail(ent[i], rule, 0, 0);
  }
  const uint64_t budget = std::max<uint64_t>(((uint64_t)c->knob_bunzip_batch_mib << 20) / 16, 1u << 20);     // bytes of slots per round: the later stages take six more per symbol
  std::vector<uint32_t> rcand, order, scap;
  std::vector<uint64_t> soff;
  std::vector<BzdCand> rc_cands;
  std::vector<BzdRec> recs;
  std::vector<BzdBlk> blks;
  std::vector<BzdBlkHost> bh;
  size_t g = 0;
  while (g < cand.size()) {
    // a round: the next candidates an open chain may still reach, as many as the slots' budget holds
    rcand.clear(); soff.clear(); scap.clear();
    uint64_t slots = 0;
    while (g < cand.size()) {
      const BzdCand &C = cand[g];
      const BzdEnt &e = ent[C.entry];
      if (e.status != 0 || C.bit < e.pos) { g++; continue; }
      const uint32_t sc = C.kind == 1 ? 0u : bzd_slot_cap(e.level, jobs[C.entry].cap);
      const uint64_t bytes = ((uint64_t)sc + 255) & ~255ull;
      if (!rcand.empty() && slots + bytes > budget) break;
      rcand.push_back((uint32_t)g); soff.push_back(slots); scap.push_back(sc);
      slots += bytes; g++;
    }
    const uint32_t R = (uint32_t)rcand.size();
    if (R == 0) break;
    rc_cands.resize(R); order.resize(R);
    for (uint32_t k = 0; k < R; k++) { rc_cands[k] = cand[rcand[k]]; order[k] = k; }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return scap[a] > scap[b]; });      // largest slots first
    BzdCarve wa;
    const uint64_t a_cand = wa.take((uint64_t)R * sizeof(BzdCand)), a_order = wa.take((uint64_t)R * 4), a_soff = wa.take((uint64_t)R * 8), a_scap = wa.take((uint64_t)R * 4),
                   a_rec = wa.take((uint64_t)R * sizeof(BzdRec)), a_counts = wa.take((uint64_t)R * 1024), a_slots = wa.take(slots + 256);
    rc = dev_grow(c, S->wa, wa.at, "hipMalloc (bunzip2 slots)");
    if (rc) return rc;
    uint8_t *A = S->wa.p;
    hipMemcpyAsync(A + a_cand, rc_cands.data(), (size_t)R * sizeof(BzdCand), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(A + a_order, order.data(), (size_t)R * 4, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(A + a_soff, soff.data(), (size_t)R * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(A + a_scap, scap.data(), (size_t)R * 4, hipMemcpyHostToDevice, st);
    hipMemsetAsync(A + a_counts, 0, (size_t)R * 1024, st);
    hipMemsetAsync(S->d_counter, 0, 4, st);
    hipLaunchKernelGGL(k_bzd_block, dim3(R < 8192 ? R : 8192), dim3(BZD_WAVE), 0, st, d_jobs, (const BzdCand *)(A + a_cand), (const uint32_t *)(A + a_order),
                       (const uint64_t *)(A + a_soff), (const uint32_t *)(A + a_scap), R, S->d_counter, A + a_slots, (uint32_t *)(A + a_counts), (BzdRec *)(A + a_rec));
    recs.resize(R);
    hipMemcpyAsync(recs.data(), A + a_rec, (size_t)R * sizeof(BzdRec), hipMemcpyDeviceToHost, st);
    BZD_HIP(hipGetLastError(), "bunzip2 block launch");
    BZD_HIP(hipStreamSynchronize(st), "bunzip2 blocks");
    c->tmark("bunzip2:k_bzd_block");
    // chain resolve: exactly the serial reading
    blks.clear(); bh.clear();
    uint64_t sym = 0;
    uint32_t nchunk = 0, nsplit = 0, nrc = 0;
    for (uint32_t k = 0; k < R; k++) {
      const BzdCand &C = rc_cands[k];
      BzdEnt &e = ent[C.entry];
      if (e.status != 0 || e.ev != 0 || C.bit < e.pos) continue;
      if (C.bit > e.pos) { bzd_no_magic(e, jobs[C.entry]); continue; }
      const BzdRec &Q = recs[k];
      if (C.kind == 1) {
        if (Q.rc) { e.ev = 2; e.ev_rule = Q.rule; e.ev_block = e.block; e.ev_bit = C.bit; }
        else { e.ev = 1; e.ev_crc = Q.stored_crc; e.ev_end = Q.end_bit; e.ev_bit = C.bit; }
        continue;
      }
      e.block++;
      if (Q.rc) { e.ev = 2; e.ev_rule = Q.rule; e.ev_block = e.block; e.ev_bit = Q.fail_bit; continue; }
      BzdBlk B{};
      B.L_off = soff[k]; B.sym0 = sym; B.out = 0; B.n = Q.nsym; B.origin = Q.origin; B.cand = k; B.chunk0 = nchunk; B.split0 = nsplit; B.rchunk0 = nrc;
      B.out_len = 0; B.period = Q.nsym; B.crc = 0; B.skip = 0;
      sym += ((uint64_t)Q.nsym + 3) & ~3ull;
      nchunk += (Q.nsym + BZD_SC - 1) / BZD_SC; nsplit += (Q.nsym + BZD_SPLIT - 1) / BZD_SPLIT + 1; nrc += (Q.nsym + BZD_RC - 1) / BZD_RC;
      blks.push_back(B);
      bh.push_back(BzdBlkHost{C.entry, e.block, Q.end_bit, Q.stored_crc});
      for (uint64_t v : {(uint64_t)entry0 + C.entry, (uint64_t)Q.nsym, (uint64_t)Q.origin, (uint64_t)Q.stored_crc, Q.end_bit}) S->last_blocks.push_back(v);
      e.pos = Q.end_bit;
    }
    const uint32_t NB = (uint32_t)blks.size();
    if (NB) {
      BzdCarve wb;
      const uint64_t b_blk = wb.take((uint64_t)NB * sizeof(BzdBlk)), b_hist = wb.take((uint64_t)nchunk * 1024), b_tt = wb.take(sym * 4 + 16), b_T = wb.take(sym + 16),
                     b_len = wb.take((uint64_t)nsplit * 4), b_succ = wb.take((uint64_t)nsplit * 4), b_rank = wb.take((uint64_t)nsplit * 4),
                     b_rlen = wb.take((uint64_t)nrc * 20), b_rexit = wb.take((uint64_t)nrc * 5), b_rentry = wb.take(nrc), b_roff = wb.take((uint64_t)nrc * 4);
      rc = dev_grow(c, S->wb, wb.at, "hipMalloc (bunzip2 inverse BWT)");
      if (rc) return rc;
      uint8_t *W = S->wb.p;
      BzdBlk *d_blk = (BzdBlk *)(W + b_blk);
      uint32_t *d_hist = (uint32_t *)(W + b_hist), *d_tt = (uint32_t *)(W + b_tt), *d_len = (uint32_t *)(W + b_len), *d_succ = (uint32_t *)(W + b_succ),
               *d_rank = (uint32_t *)(W + b_rank), *d_rlen = (uint32_t *)(W + b_rlen), *d_roff = (uint32_t *)(W + b_roff);
      hipMemcpyAsync(d_blk, blks.data(), (size_t)NB * sizeof(BzdBlk), hipMemcpyHostToDevice, st);
      hipLaunchKernelGGL(k_bzd_hist, dim3(nchunk), dim3(BZD_WAVE), 0, st, (const BzdBlk *)d_blk, NB, (const uint8_t *)(A + a_slots), d_hist);
      hipLaunchKernelGGL(k_bzd_offsets, dim3(NB), dim3(256), 0, st, (const BzdBlk *)d_blk, (const uint32_t *)(A + a_counts), d_hist);
      hipLaunchKernelGGL(k_bzd_scatter, dim3(nchunk), dim3(BZD_WAVE), 0, st, (const BzdBlk *)d_blk, NB, (const uint8_t *)(A + a_slots), (const uint32_t *)d_hist, d_tt);
      c->tmark("bunzip2:counting sort");
      hipLaunchKernelGGL(k_bzd_walk1, dim3((nsplit + 255) / 256), dim3(256), 0, st, (const BzdBlk *)d_blk, NB, nsplit, (const uint32_t *)d_tt, d_len, d_succ, d_rank);
      hipLaunchKernelGGL(k_bzd_rank, dim3((NB + BZD_WAVE - 1) / BZD_WAVE), dim3(BZD_WAVE), 0, st, d_blk, NB, (const uint32_t *)d_len, (const uint32_t *)d_succ, d_rank);
      hipLaunchKernelGGL(k_bzd_walk2, dim3((nsplit + 255) / 256), dim3(256), 0, st, (const BzdBlk *)d_blk, NB, nsplit, (const uint32_t *)d_tt, (const uint32_t *)d_len,
                         (const uint32_t *)d_rank, W + b_T);
      c->tmark("bunzip2:walk");
      hipLaunchKernelGGL(k_bzd_rle_a, dim3((nrc + 255) / 256), dim3(256), 0, st, (const BzdBlk *)d_blk, NB, nrc, (const uint8_t *)(W + b_T), d_rlen, W + b_rexit);
      hipLaunchKernelGGL(k_bzd_rle_b, dim3((NB + BZD_WAVE - 1) / BZD_WAVE), dim3(BZD_WAVE), 0, st, d_blk, NB, (const uint32_t *)d_rlen, (const uint8_t *)(W + b_rexit),
                         W + b_rentry, d_roff);
      hipMemcpyAsync(blks.data(), d_blk, (size_t)NB * sizeof(BzdBlk), hipMemcpyDeviceToHost, st);
      BZD_HIP(hipGetLastError(), "bunzip2 inverse BWT launch");
      BZD_HIP(hipStreamSynchronize(st), "bunzip2 inverse BWT");
      c->tmark("bunzip2:RLE_1 lengths");
      // placement: the sums per entry against cap before anything is written
      for (uint32_t b = 0; b < NB; b++) {
        BzdEnt &e = ent[bh[b].entry];
        if (e.st_rule) { blks[b].skip = 1; continue; }
        if (e.out_off + blks[b].out_len > jobs[bh[b].entry].cap) { e.st_rule = BZD_R_OUTPUT_FULL; e.st_block = bh[b].block; e.st_bit = bh[b].end_bit; blks[b].skip = 1; continue; }
        blks[b].out = jobs[bh[b].entry].out + e.out_off;
        e.out_off += blks[b].out_len;
      }
      hipMemcpyAsync(d_blk, blks.data(), (size_t)NB * sizeof(BzdBlk), hipMemcpyHostToDevice, st);
      hipLaunchKernelGGL(k_bzd_rle_fill, dim3((nrc + 255) / 256), dim3(256), 0, st, (const BzdBlk *)d_blk, NB, nrc, (const uint8_t *)(W + b_T), (const uint8_t *)(W + b_rentry),
                         (const uint32_t *)d_roff);
      c->tmark("bunzip2:k_bzd_rle_fill");
      hipLaunchKernelGGL(k_bzd_crc, dim3(NB), dim3(BZD_WAVE), 0, st, d_blk, (const BzdCrcOps *)S->d_ops);
      hipMemcpyAsync(blks.data(), d_blk, (size_t)NB * sizeof(BzdBlk), hipMemcpyDeviceToHost, st);
      BZD_HIP(hipGetLastError(), "bunzip2 fill launch");
      BZD_HIP(hipStreamSynchronize(st), "bunzip2 fill");
      c->tmark("bunzip2:k_bzd_crc");
      for (uint32_t b = 0; b < NB; b++) {
        BzdEnt &e = ent[bh[b].entry];
        if (blks[b].skip || (e.st_rule && e.st_block < bh[b].block)) continue;
        if (blks[b].crc != bh[b].stored_crc) { e.st_rule = BZD_R_BLOCK_CRC; e.st_block = bh[b].block; e.st_bit = bh[b].end_bit; continue; }
        e.comb = ((e.comb << 1) | (e.comb >> 31)) ^ blks[b].crc;
      }
    }
    // what the chains met in this round, in the order of the serial reading: a later stage's failure lies before the event
    for (uint32_t k = 0; k < R; k++) {
      BzdEnt &e = ent[rc_cands[k].entry];
      if (e.status != 0) continue;
      if (e.st_rule) { bzd_fail(e, e.st_rule, e.st_block, e.st_bit); continue; }
      if (e.ev == 2) bzd_fail(e, e.ev_rule, e.ev_block, e.ev_bit);
      else if (e.ev == 1) {
        if (e.ev_crc != e.comb) bzd_fail(e, BZD_R_STREAM_CRC, e.block, e.ev_bit);
        else { e.status = 1; e.in_used = (e.ev_end + 7) / 8; e.fail_bit = e.ev_end; }
      }
    }
  }
  for (uint32_t i = 0; i < E; i++) {
    BzdEnt &e = ent[i];
    if (e.status == 0) { bzd_no_magic(e, jobs[i]); bzd_fail(e, e.ev_rule, e.ev_block, e.ev_bit); }
  }
  // the entries' Zip CRC-32 (k_inf_crc)
  std::vector<uint64_t> optr(E), olen(E);
  std::vector<uint32_t> regs(E);
  for (uint32_t i = 0; i < E; i++) { optr[i] = jobs[i].out; olen[i] = ent[i].status == 1 ? ent[i].out_off : 0; regs[i] = crc_in ? crc_in[i] : 0u; }
  rc = inflate_crc_entries(c, E, optr.data(), olen.data(), regs.data());
  if (rc) return rc;
  c->tmark("bunzip2:k_inf_crc");
  for (uint32_t i = 0; i < E; i++) {
    const BzdEnt &e = ent[i];
    BzdResult &Q = res[i];
    Q.rc = e.status == 1 ? 0 : BZD_E_DATA; Q.rule = e.status == 1 ? 0u : e.rule;
    Q.out_len = e.status == 1 ? e.out_off : 0; Q.in_used = e.status == 1 ? e.in_used : 0;
    Q.bitpos = e.fail_bit; Q.block = e.block; Q.crc = regs[i];
    for (uint64_t v : {(uint64_t)Q.rule, (uint64_t)e.block, e.fail_bit, (uint64_t)0}) S->last_entries.push_back(v);
  }
  return 0;
}

static void bzd_describe(Ctx *c, const BzdResult &R, int entry) {
  char buf[240];
  snprintf(buf, sizeof buf, "bunzip2: entry %d: %s in block %u at bit %llu", entry, bzd_rule_name(R.rule), R.block, (unsigned long long)R.bitpos);
  c->err = buf;
}

struct BzdReader : ReaderTraits<BzdJob, BzdResult, BzdState> {
  static constexpr const char *word = "bunzip2";
  static BzdState *state(Ctx *c) { return bzd_state(c); }
  static void begin(BzdState *S) { S->last_entries.clear(); S->last_blocks.clear(); }
  // streams and outputs of a group: half of the knob; the rounds' work arrays: the rest
  static uint64_t limit(const Ctx *c) { return ((uint64_t)c->knob_bunzip_batch_mib << 20) / 2; }
  static int run(Ctx *c, BzdState *S, std::vector<BzdJob> &jobs, const uint32_t *crc_in, std::vector<BzdResult> &res, uint32_t entry0) { return bzd_run(c, S, jobs, crc_in, res, entry0); }
  static void describe(Ctx *c, const BzdResult &R, int entry) { bzd_describe(c, R, entry); }
};

// bzd_run for zada_unzip_device (zada_internal.h)
int bunzip2_run_jobs(Ctx *c, uint32_t E, const ReaderJob *rj, ReaderRes *rr, bool *described) {
  return reader_run_jobs<BzdReader>(c, E, rj, rr, described, [](const ReaderJob &J) { return BzdJob{J.in, J.out, J.n_in, J.cap}; });
}

}  // namespace zada

using namespace zada;

static constexpr uint64_t BZD_MAX_BYTES = 1ull << 40;      // (as Inflate: a stream or an output of 1 TiB and more is beyond any device)

int zada_bunzip2_device(zada_ctx *z, const void *d_in, uint64_t n_in, void *d_out, uint64_t cap, uint64_t *out_len, uint64_t *in_used, uint32_t *crc_inout) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if ((n_in && !d_in) || (cap && !d_out)) { c->err = "zada_bunzip2_device: null buffer"; return ZADA_E_INVALID; }
  if (n_in >= BZD_MAX_BYTES || cap >= BZD_MAX_BYTES) { c->err = "zada_bunzip2_device: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  return reader_device_one<BzdReader>(c, out_len, in_used, crc_inout, [&](BzdJob &J) {
    J = BzdJob{(uint64_t)(uintptr_t)d_in, (uint64_t)(uintptr_t)d_out, n_in, cap};
    return 0;
  });
}

int zada_bunzip2_batch(zada_ctx *z, int count, const uint8_t *const *in, const uint64_t *n_in, uint8_t *const *out, const uint64_t *cap, uint64_t *out_len,
                       uint64_t *in_used, uint32_t *crc, int *rc_out) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (count && (!in || !n_in || !cap || !rc_out)) { c->err = "zada_bunzip2_batch: null argument"; return ZADA_E_INVALID; }
  for (int i = 0; i < count; i++) {
    if ((n_in[i] && !in[i]) || (out && cap[i] && !out[i])) { c->err = "zada_bunzip2_batch: null buffer"; return ZADA_E_INVALID; }
    if (n_in[i] >= BZD_MAX_BYTES || cap[i] >= BZD_MAX_BYTES) { c->err = "zada_bunzip2_batch: a stream or an output of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  }
  if (count == 0) return ZADA_OK;
  return reader_batch<BzdReader>(c, count, in, n_in, out, cap, out_len, in_used, crc, rc_out,
                                 [&](int i, uint64_t d_in, uint64_t d_out) { return BzdJob{d_in, d_out, n_in[i], cap[i]}; });
}

int zada_bunzip2(zada_ctx *z, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used, uint32_t *crc_inout) {
  if (!z) return ZADA_E_INVALID;
  z->c.lz_stopped = false;
  if ((n_in && !in) || (cap && !out)) { z->c.err = "zada_bunzip2: null buffer"; return ZADA_E_INVALID; }
  return reader_single(out_len, in_used, crc_inout, [&](uint64_t *ol, uint64_t *iu, uint32_t *reg, int *erc) {
    return zada_bunzip2_batch(z, 1, &in, &n_in, &out, &cap, ol, iu, reg, erc);
  });
}

uint64_t zada_bunzip2_last_records(zada_ctx *z, int what, uint64_t *dst, uint64_t cap_items) {
  if (!z || !z->c.bzd || (cap_items && !dst)) return 0;
  const BzdState *S = (const BzdState *)z->c.bzd;
  return reader_last_records(what == 0 ? S->last_entries : S->last_blocks, dst, cap_items);
}
