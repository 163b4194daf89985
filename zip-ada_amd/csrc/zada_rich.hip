// zada_rich.hip -- Deflate_R's LZ77 front end on gfx950: LZ77.Rich (Rich Geldreich's PROG2.C, lz77.adb:1829-2143).
//
// The reference parses the input in sectors of 8 KiB (SECTORLEN, counted from the entry's start) held in a ring of four;
// Dict_Search starts afresh at every sector (:2039-2040) and no match crosses a sector's end.  Read as a closed form
// (DESIGN.md 11):
//   * h (p) = (b [p] << 10 ^ b [p+1] << 5 ^ b [p+2]) & 0x1FFF for every p with 3 bytes left in its sector (Hash_Data :1947-1981);
//   * the walk from position i of sector S visits the positions q with h (q) = h (i), max (entry, (S-3) * 8 KiB) <= q < i,
//     newest first, at most 4 096 of them (Find_Match :1989-2023, Delete_Data :1927-1942); it keeps the longest match
//     (first reached among equals), stopping at 258;
//   * a comparison that reads stream offset x at or beyond the sector's loaded end sees what the ring still holds there:
//     the byte x - 32 768, or -- where the ring was never written -- 0 (zada.h: the convention for unwritten bytes);
//   * one (L, P) pair per position, searched from length 2, is all the non-greedy parse (:2042-2082) needs.
// So every sector is an independent job over a window of at most 32 KiB + 258 bytes:
//   k_rich_links   one wave per 32 KiB run: the link of every hashed position to the nearest earlier one with its hash
//                  (u16 distance), by a 13-bit head table in LDS, 64 positions at a time;
//   k_rich_match   one workgroup per sector: window bytes and links in LDS, (L, P) of every position; the lanes take
//                  positions from an LDS counter whenever their walk ends (the walks are very uneven);
//   k_rich_parse   one lane per sector: the parse over (L, P), tokens and their positions into the sector's slots;
//   k_rich_compact the sectors' tokens into the atom array (exclusive_scan_u32 over the per-sector counts).
#include "../../include/zada.h"
#include "zada_internal.h"

namespace zada {

constexpr uint32_t RS = 8192;                       // SECTORLEN (SECTORBIT 13)
constexpr uint32_t R_HASH = 8192;                   // HASHSIZE (HASHBITS 13)
constexpr uint32_t R_MAXCMP = 4096;                 // MAXCOMPARES
constexpr uint32_t R_MAXMATCH = 258;                // MAXMATCH
constexpr uint32_t R_BACK = 3 * RS;                 // a sector's window reaches three sectors back
constexpr uint32_t R_WBYTES = 4 * RS + R_MAXMATCH;  // window bytes, the view past the loaded end included
constexpr uint32_t R_WPAD = (R_WBYTES + 255) & ~255u;
constexpr uint32_t R_LDS = R_WPAD + 4 * RS * 2 + 64;   // window, links of its positions, the work counter
constexpr uint32_t R_MATCH_THREADS = 1024;
static_assert(RS % PCHUNK == 0 && 32768 % RS == 0, "sectors: whole parse chunks, four to a 32 KiB segment");
static_assert(R_LDS <= 160 * 1024, "LDS of one CU");

// Where the sectors lie.  One stream: the buffer holds stream bytes from offset `gpos` on, `es` = -gpos is where the stream
// starts in buffer coordinates, `end` where it ends (~0: behind the buffer).  A batch: `segend` (Layout, zada_lz.hip).
struct RichGeo {
  const uint8_t *in;
  const uint32_t *segend;
  int64_t es;
  uint64_t end;
  uint64_t s_first;                                  // the first sector the call parses
};

// The entry's first byte for the sector holding p.  An entry that began in an earlier 32 KiB segment began at least 32 KiB
// before p's sector: any value that far back says the same (every look back stays inside the entry).
__device__ __forceinline__ int64_t r_entry_start(const RichGeo &g, uint64_t p) {
  if (!g.segend) return g.es;
  const uint64_t seg = p >> 15;
  return (g.segend[seg] >> 31) ? (int64_t)(seg << 15) : (int64_t)(p & ~(uint64_t)(RS - 1)) - 32768;
}
__device__ __forceinline__ uint64_t r_sector_end(const RichGeo &g, uint64_t s0) {        // loaded end of the sector at s0
  const uint64_t e = g.segend ? (uint64_t)(g.segend[s0 >> 15] & 0x7FFFFFFFu) : g.end, f = s0 + RS;
  return e < f ? e : f;
}
__device__ __forceinline__ uint32_t r_hash(const uint8_t *b) { return (((uint32_t)b[0] << 10) ^ ((uint32_t)b[1] << 5) ^ b[2]) & (R_HASH - 1); }

// One wave per run of four sectors: links [q] = q - q' for the nearest earlier hashed q' with h (q') = h (q), no further back
// than the first sector's window (0 = none).  The run is scanned from its first sector's window start, 64 positions at a
// time: a lane finds the nearest lower lane with its hash itself, else takes the head table's entry; the last lane of each
// hash then moves the head.  The first run also writes the links of the window in front of it.
__global__ void __launch_bounds__(64) k_rich_links(RichGeo g, uint32_t nruns, uint64_t hi, uint16_t *__restrict__ links) {
  __shared__ uint16_t head[R_HASH];                  // position - lo + 1 of the newest member, 0 = none
  const uint32_t r = blockIdx.x;
  const int lane = threadIdx.x;
  if (r >= nruns) return;
  const uint64_t R0 = g.s_first + (uint64_t)r * 4 * RS;
  const uint64_t rend = R0 + 4 * RS < hi ? R0 + 4 * RS : hi;
  const int64_t es = r_entry_start(g, R0), wb = (int64_t)R0 - (int64_t)R_BACK;
  const uint64_t lo = (uint64_t)(es > wb ? es : wb);
  const uint64_t wlo = r == 0 ? lo : R0;
  for (int i = lane; i < (int)R_HASH; i += 64) head[i] = 0;
  __syncthreads();
  for (uint64_t c = lo; c < rend; c += 64) {
    const uint64_t q = c + lane;
    bool hashed = false;
    uint32_t h = 0x10000u + lane;                    // (unhashed lanes: a value no other lane has)
    if (q < rend && q + 2 < r_sector_end(g, q & ~(uint64_t)(RS - 1))) { hashed = true; h = r_hash(g.in + q); }
    int prevlane = -1;
    bool later = false;
    for (int j = 0; j < 64; j++) {
      const uint32_t hj = __builtin_amdgcn_readlane(h, j);
      if (hj == h) { if (j < lane) prevlane = j; else if (j > lane) later = true; }
    }
    uint32_t link = 0;
    if (hashed) link = prevlane >= 0 ? (uint32_t)(c - lo) + (uint32_t)prevlane + 1u : (uint32_t)head[h];
    __syncthreads();                                 // (every lane has read the table before it changes)
    if (hashed && !later) head[h] = (uint16_t)(q - lo + 1);
    __syncthreads();
    if (q >= wlo && q < rend) links[q] = (hashed && link) ? (uint16_t)((uint32_t)(q - lo + 1) - link) : (uint16_t)0;
  }
}

// One workgroup per sector: lp [p] = L << 16 | (p - P) for every position p of the sector (0 where L <= 2).
__global__ void __launch_bounds__(R_MATCH_THREADS) k_rich_match(RichGeo g, const uint16_t *__restrict__ links, uint32_t *__restrict__ lp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t *win = lds;
  uint16_t *lnk = (uint16_t *)(lds + R_WPAD);
  uint32_t *ctr = (uint32_t *)(lds + R_WPAD + 4 * RS * 2);
  const int tid = threadIdx.x;
  const uint64_t s0 = g.s_first + (uint64_t)blockIdx.x * RS;
  const uint64_t e = r_sector_end(g, s0);
  if (e <= s0) return;                               // (a batch slot's room behind its entry)
  const int64_t es = r_entry_start(g, s0), wb = (int64_t)s0 - (int64_t)R_BACK;
  const uint64_t ws = (uint64_t)(es > wb ? es : wb);
  const uint32_t wlen = (uint32_t)(s0 + RS + R_MAXMATCH - ws);
  for (uint32_t v = tid; v < wlen; v += R_MATCH_THREADS) {
    const uint64_t x = ws + v;
    uint8_t b = 0;                                   // never written: 0
    if (x < e) b = g.in[x];
    else if (x >= 32768 && (int64_t)x - 32768 >= es) b = g.in[x - 32768];   // what the ring still holds there
    win[v] = b;
  }
  const uint32_t nl = (uint32_t)(e - ws);
  for (uint32_t v = tid; v < nl; v += R_MATCH_THREADS) lnk[v] = links[ws + v];
  if (tid == 0) *ctr = 0;
  __syncthreads();
  const uint32_t cnt = (uint32_t)(e - s0), base = (uint32_t)(s0 - ws);
  uint32_t i = 0, q = 0, best = 0, bd = 0, steps = 0;
  uint8_t mb = 0;
  bool active = false, live = true;
  for (;;) {
    if (!active && live) {                           // this lane's walk has ended: the next position
      const uint32_t k = atomicAdd(ctr, 1u);
      if (k >= cnt) live = false;
      else if (s0 + k + 2 < e) { i = base + k; q = i; best = 2; bd = 0; steps = 0; mb = win[i + 2]; active = true; }
      else lp[s0 + k] = 0;                           // (the last two positions of a sector have no link)
    }
    if (__ballot(live) == 0) break;
    if (!active) continue;
    const uint32_t d = lnk[q];
    bool stop = d == 0 || d > q;                     // no older member, or one before the window
    if (!stop) {
      q -= d;
      if (win[q + best] == mb) {
        uint32_t len = 0;
        while (len < R_MAXMATCH && win[i + len] == win[q + len]) len++;
        if (len > best) {
          best = len; bd = i - q;
          if (best == R_MAXMATCH) stop = true;
          else mb = win[i + best];
        }
      }
      if (++steps == R_MAXCMP) stop = true;
    }
    if (stop) {
      lp[s0 + (i - base)] = best > 2 ? (best << 16) | bd : 0u;
      active = false;
    }
  }
}

// One lane per sector: Dict_Search's non-greedy loop over (L, P).  Tokens and their buffer positions go to the sector's
// RS slots of tok / tpos, the count to counts.
__global__ void __launch_bounds__(64) k_rich_parse(RichGeo g, uint32_t nsec, const uint32_t *__restrict__ lp, uint32_t *__restrict__ tok,
                                                   uint32_t *__restrict__ tpos, uint32_t *__restrict__ counts) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsec) return;
  const uint64_t s0 = g.s_first + (uint64_t)s * RS, e = r_sector_end(g, s0);
  uint32_t *t = tok + (uint64_t)s * RS, *tp = tpos + (uint64_t)s * RS;
  uint32_t k = 0;
  uint64_t i = s0;
  uint32_t j = e > s0 ? (uint32_t)(e - s0) : 0u;
  while (j > 0) {
    const uint32_t v = lp[i];
    uint32_t m = v >> 16, d = v & 0xFFFFu;
    if (m > 2) {
      for (;;) {                                     // a longer match one further on: this byte as a literal
        const uint32_t v1 = lp[i + 1];
        if ((v1 >> 16) <= m) break;
        t[k] = g.in[i]; tp[k] = (uint32_t)i; k++; i++; j--;
        m = v1 >> 16; d = v1 & 0xFFFFu;
      }
      if (m > j) m = j;                              // clamped to the sector's end
    }
    if (m <= 2) { t[k] = g.in[i]; tp[k] = (uint32_t)i; k++; i++; j--; continue; }
    t[k] = tok_match(m, d); tp[k] = (uint32_t)i; k++;
    i += m; j -= m;
  }
  counts[s] = k;
}

// one wave per sector: its tokens to their place in the atom array
__global__ void __launch_bounds__(256) k_rich_compact(uint32_t nsec, const uint32_t *__restrict__ tok, const uint32_t *__restrict__ tpos,
                                                      const uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                      uint32_t *__restrict__ atoms, uint32_t *__restrict__ apos, uint32_t apos_bias) {
  const uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (s >= nsec) return;
  const uint32_t cnt = counts[s], o = offsets[s];
  const uint32_t *t = tok + (uint64_t)s * RS, *tp = tpos + (uint64_t)s * RS;
  for (uint32_t k = lane; k < cnt; k += 64) { atoms[o + k] = t[k]; apos[o + k] = tp[k] + apos_bias; }
}

// a batch: the atom offset of every parse chunk (batch_geometry reads it at the entries' first chunks)
__global__ void k_rich_chunk_offsets(uint32_t nch, const uint32_t *__restrict__ sec_off, uint32_t *__restrict__ offsets) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nch) offsets[k] = sec_off[k / (RS / PCHUNK)];
}

int rich_shard(Ctx *c, const ShardJob &job, ShardResult *res) {
  hipStream_t st = c->stream;
  Workspace &W = c->ws;
  const uint64_t n = job.nbuf;
  if (job.need) { if (int rn = job.need(n)) return rn; }
  RichGeo g;
  g.in = W.in; g.segend = job.segend; g.es = -(int64_t)job.gpos; g.end = job.final ? n : ~0ull;
  g.s_first = job.segend ? 0 : job.tok_lo;
  const uint64_t hi = job.segend || job.final ? n : job.tok_hi;
  if ((g.s_first % RS) != 0) { c->err = "Deflate_R: a shard must start on an 8 KiB sector"; return ZADA_E_INVALID; }
  res->ntok = 0; res->exit = ExitState{(uint32_t)hi, SYNC_F}; res->warm = ExitState{(uint32_t)g.s_first, SYNC_F};
  if (hi <= g.s_first) return 0;
  const uint32_t nsec = (uint32_t)((hi - g.s_first + RS - 1) / RS), nruns = (nsec + 3) / 4;
  // the sectors' token and position slots share the speculative-token block (2.25 words per byte of the workspace)
  uint32_t *tok = W.spec_tok, *tpos = W.spec_tok + (uint64_t)nsec * RS;
  uint32_t *lp = (uint32_t *)W.M;
  c->tmark("rich:begin");
  hipFuncSetAttribute((const void *)k_rich_match, hipFuncAttributeMaxDynamicSharedMemorySize, R_LDS);
  hipLaunchKernelGGL(k_rich_links, dim3(nruns), dim3(64), 0, st, g, nruns, hi, W.lprev[0]);
  c->tmark("rich:links");
  hipLaunchKernelGGL(k_rich_match, dim3(nsec), dim3(R_MATCH_THREADS), R_LDS, st, g, (const uint16_t *)W.lprev[0], lp);
  c->tmark("rich:match");
  hipLaunchKernelGGL(k_rich_parse, dim3((nsec + 63) / 64), dim3(64), 0, st, g, nsec, (const uint32_t *)lp, tok, tpos, W.counts);
  exclusive_scan_u32(st, W.counts, W.take_from, W.scan_sums, W.n_changed, nsec);
  uint32_t total = 0;
  hipMemcpyAsync(&total, W.n_changed, 4, hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipStreamSynchronize(st), "Deflate_R parse")) return ZADA_E_HIP_;
  c->tmark("rich:parse");
  uint32_t *dst_atoms = job.dst_atoms, *dst_apos = job.dst_apos;
  if (total > job.cap_atoms) {
    if (!job.grow_atoms) { c->err = "atom array overflow"; return -2; }
    if (int rg = job.grow_atoms(total, &dst_atoms, &dst_apos)) return rg;
  }
  hipLaunchKernelGGL(k_rich_compact, dim3((nsec + 3) / 4), dim3(256), 0, st, nsec, (const uint32_t *)tok, (const uint32_t *)tpos, (const uint32_t *)W.counts,
                     (const uint32_t *)W.take_from, dst_atoms, dst_apos, job.apos_bias);
  if (job.segend) {
    const uint32_t nch = nsec * (RS / PCHUNK);
    hipLaunchKernelGGL(k_rich_chunk_offsets, dim3((nch + 255) / 256), dim3(256), 0, st, nch, (const uint32_t *)W.take_from, W.offsets);
  }
  c->tmark("rich:compact");
  res->ntok = total;
  return hip_check(c, hipGetLastError(), "Deflate_R compact");
}

}  // namespace zada
