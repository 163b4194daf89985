// zada_rezip.hip -- the tools on top of the archive reader and writer.  ReZip (tools/rezip_lib.adb): zada_rezip_device, at the end of
// this file, is host code around zada_unzip_device, zada_zip_device_ex and the writer's table-driven copy.  Comp_Zip (tools/comp_zip_prc.adb):
// zada_compare_device, the first offset at which two device buffers differ, and zada_compzip_device, two archives in device memory compared entry
// by entry.  The host side is a plan (zada_rezip_plan.h: the verdict, argument checks, groups) around zada_unzip_device, whose launches extract both
// sides of a group into workspace; what is new here:
// k_cz_compare: one wave per piece of 16 KiB of a pair of buffers, four pieces per workgroup.  Side a is read with 16-byte loads from its word
//   boundary on (up to 15 head bytes and 15 tail bytes one per lane).  Where side b has the same 16-byte phase it is read the same way; where not,
//   every lane loads the two aligned words that hold its sixteen bytes (its neighbour's load of the same word hits in L1) and funnels them into one
//   with v_alignbyte -- no load is unaligned, and none touches a 16-byte word without a byte of the buffer in it.  The lane xors, takes the first set
//   bit's byte (trailing-zero count >> 3) and keeps the smallest offset it has seen; the wave leaves its loop of four-strip groups behind the first group in which any
//   lane saw a difference (the words that are left still run through the word-by-word loop; what they find lies further on), takes the minimum across its lanes and lane 0 sends it to the pair's 64-bit word with one atomic minimum.  A piece that
//   begins behind the value the word already holds ends at once: the word only falls, and only to offsets at which the buffers do differ.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <new>
#include <string>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_rezip_plan.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {

constexpr uint32_t CZ_WAVE = 64, CZ_NONE = 0xFFFFFFFFu;
constexpr uint32_t CZ_UNROLL = 4;                      // 16-byte words per lane between two looks at "did any lane see a difference"
typedef __attribute__((address_space(1))) const uint8_t cz_gcu8;
typedef uint32_t cz_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const cz_u32x4 cz_gcu4;

struct CzPair { uint64_t a, b, n; };                   // device addresses; n: the bytes that count

// the byte offset of the first set bit of x (16: none)
__device__ __forceinline__ uint32_t cz_first(cz_u32x4 x) {
  uint32_t r = 16;
  if (x.w) r = 12u + ((uint32_t)__builtin_ctz(x.w) >> 3);
  if (x.z) r = 8u + ((uint32_t)__builtin_ctz(x.z) >> 3);
  if (x.y) r = 4u + ((uint32_t)__builtin_ctz(x.y) >> 3);
  if (x.x) r = (uint32_t)__builtin_ctz(x.x) >> 3;
  return r;
}
// the sixteen bytes that begin s = 4 q + r bytes (1 .. 15) into the aligned words lo, hi
__device__ __forceinline__ cz_u32x4 cz_funnel(cz_u32x4 lo, cz_u32x4 hi, uint32_t q, uint32_t r) {
  uint32_t x0 = lo.x, x1 = lo.y, x2 = lo.z, x3 = lo.w, x4 = hi.x, x5 = hi.y, x6 = hi.z, x7 = hi.w;
  if (q & 2u) { x0 = x2; x1 = x3; x2 = x4; x3 = x5; x4 = x6; x5 = x7; }
  if (q & 1u) { x0 = x1; x1 = x2; x2 = x3; x3 = x4; x4 = x5; }
  cz_u32x4 o;
  o.x = __builtin_amdgcn_alignbyte(x1, x0, r); o.y = __builtin_amdgcn_alignbyte(x2, x1, r);
  o.z = __builtin_amdgcn_alignbyte(x3, x2, r); o.w = __builtin_amdgcn_alignbyte(x4, x3, r);
  return o;
}

// pieces = nullptr: one pair, piece k at k << CZ_PIECE_LOG.  first [pair] holds n of the pair, or a smaller offset, when the kernel starts.
__global__ void __launch_bounds__(CZ_WAVE * CZ_WAVES) k_cz_compare(const CzPair *__restrict__ pairs, const UzPiece *__restrict__ pieces, uint64_t npieces,
                                                                   unsigned long long *first) {
  const uint32_t lane = threadIdx.x & (CZ_WAVE - 1);
  const uint64_t pi = (uint64_t)blockIdx.x * CZ_WAVES + (threadIdx.x >> 6);
  if (pi >= npieces) return;
  uint64_t off;
  uint32_t pair, len;
  if (pieces) { const UzPiece P = pieces[pi]; off = P.off; pair = P.entry; len = P.len; }
  else {
    pair = 0; off = pi << CZ_PIECE_LOG;
    const uint64_t rest = pairs[0].n - off;
    len = (uint32_t)(rest < CZ_PIECE ? rest : CZ_PIECE);
  }
  const CzPair Q = pairs[pair];
  if (__hip_atomic_load(&first[pair], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < off) return;      // (every lane asks for the same word: one request, and the exit is the wave's)
  cz_gcu8 *a = (cz_gcu8 *)(Q.a + off);
  cz_gcu8 *b = (cz_gcu8 *)(Q.b + off);
  uint32_t m = CZ_NONE;                                   // the smallest offset in the piece at which this lane saw a difference
  uint32_t h = (16u - (uint32_t)((uintptr_t)a & 15u)) & 15u;
  if (h > len) h = len;
  if (lane < h && a[lane] != b[lane]) m = lane;
  const uint32_t words = (len - h) >> 4;
  const uint32_t s = (uint32_t)((uintptr_t)(b + h) & 15u);
  cz_gcu4 *a4 = (cz_gcu4 *)(a + h);
  cz_gcu4 *b4 = (cz_gcu4 *)(b + h - s);                   // s > 0: word w of side a lies in words w and w + 1 from here, each with a byte of the piece in it
  // whole groups of CZ_UNROLL kilobyte strips: every load of a group is issued before the first comparison; then the strips that are left, word by word
  uint32_t w0 = 0;
  if (s == 0) {
    for (; w0 + CZ_WAVE * CZ_UNROLL <= words && !__any(m != CZ_NONE); w0 += CZ_WAVE * CZ_UNROLL) {
      cz_u32x4 va[CZ_UNROLL], vb[CZ_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < CZ_UNROLL; u++) { va[u] = a4[w0 + u * CZ_WAVE + lane]; vb[u] = b4[w0 + u * CZ_WAVE + lane]; }
#pragma unroll
      for (uint32_t u = 0; u < CZ_UNROLL; u++) {
        const uint32_t r = cz_first(va[u] ^ vb[u]);
        if (r < 16u && m == CZ_NONE) m = h + 16u * (w0 + u * CZ_WAVE + lane) + r;
      }
    }
    for (uint32_t w = w0 + lane; w < words; w += CZ_WAVE) {
      const uint32_t r = cz_first(a4[w] ^ b4[w]);
      if (r < 16u && m == CZ_NONE) m = h + 16u * w + r;
    }
  } else {
    const uint32_t q = s >> 2, r8 = s & 3u;
    for (; w0 + CZ_WAVE * CZ_UNROLL <= words && !__any(m != CZ_NONE); w0 += CZ_WAVE * CZ_UNROLL) {
      cz_u32x4 va[CZ_UNROLL], lo[CZ_UNROLL], hi[CZ_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < CZ_UNROLL; u++) { const uint32_t w = w0 + u * CZ_WAVE + lane; va[u] = a4[w]; lo[u] = b4[w]; hi[u] = b4[w + 1]; }
#pragma unroll
      for (uint32_t u = 0; u < CZ_UNROLL; u++) {
        const uint32_t r = cz_first(va[u] ^ cz_funnel(lo[u], hi[u], q, r8));
        if (r < 16u && m == CZ_NONE) m = h + 16u * (w0 + u * CZ_WAVE + lane) + r;
      }
    }
    for (uint32_t w = w0 + lane; w < words; w += CZ_WAVE) {
      const uint32_t r = cz_first(a4[w] ^ cz_funnel(b4[w], b4[w + 1], q, r8));
      if (r < 16u && m == CZ_NONE) m = h + 16u * w + r;
    }
  }
  // (a lane's words ascend, so its first hit is its smallest; the head lies in front of every word and the tail behind)
  const uint32_t t = h + words * 16u + lane;
  if (t < len && m == CZ_NONE && a[t] != b[t]) m = t;
#pragma unroll
  for (int j = 1; j < (int)CZ_WAVE; j <<= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)m, j, CZ_WAVE);
    m = o < m ? o : m;
  }
  if (lane == 0 && m != CZ_NONE) atomicMin(&first[pair], (unsigned long long)(off + m));
}

// ---- host side ----
struct RzState { DevBuf tabs, arena_a, arena_b, hold; };      // hold: the streams of a ReZip group, method after method, until the group is placed

static RzState *rz_state(Ctx *c) {
  if (!c->rz) c->rz = new (std::nothrow) RzState();
  return (RzState *)c->rz;
}
void rezip_destroy(Ctx *c) {
  RzState *S = (RzState *)c->rz;
  if (!S) return;
  for (DevBuf *b : {&S->tabs, &S->arena_a, &S->arena_b, &S->hold}) dev_free(*b);
  delete S;
  c->rz = nullptr;
}

#define RZ_HIP(call, what) do { if (hip_check(c, (call), what)) return ZADA_E_HIP_; } while (0)

// pairs [0 .. np) through one launch of k_cz_compare: over `pieces`, or (pieces empty, np = 1) over the pieces of the one pair.  first [k]: the first
// offset below pairs [k].n at which the pair differs, or pairs [k].n.  Synchronises.
static int cz_run(Ctx *c, RzState *S, const std::vector<CzPair> &pairs, const std::vector<UzPiece> &pieces, std::vector<uint64_t> &first, const char *mark) {
  hipStream_t st = c->stream;
  const uint32_t np = (uint32_t)pairs.size();
  const uint64_t NP = pieces.empty() ? cz_piece_count(pairs[0].n) : pieces.size();
  first.resize(np);
  for (uint32_t k = 0; k < np; k++) first[k] = pairs[k].n;
  if (!NP) return 0;
  const uint64_t o_pairs = 0, o_first = (o_pairs + (uint64_t)np * sizeof(CzPair) + 255) & ~255ull, o_pieces = (o_first + (uint64_t)np * 8 + 255) & ~255ull;
  const int rc = dev_grow(c, S->tabs, o_pieces + pieces.size() * sizeof(UzPiece) + 256, "hipMalloc (compare tables)");
  if (rc) return rc;
  uint8_t *T = S->tabs.p;
  hipMemcpyAsync(T + o_pairs, pairs.data(), (size_t)np * sizeof(CzPair), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(T + o_first, first.data(), (size_t)np * 8, hipMemcpyHostToDevice, st);
  if (!pieces.empty()) hipMemcpyAsync(T + o_pieces, pieces.data(), pieces.size() * sizeof(UzPiece), hipMemcpyHostToDevice, st);
  hipLaunchKernelGGL(k_cz_compare, dim3((uint32_t)((NP + CZ_WAVES - 1) / CZ_WAVES)), dim3(CZ_WAVE * CZ_WAVES), 0, st, (const CzPair *)(T + o_pairs),
                     pieces.empty() ? (const UzPiece *)nullptr : (const UzPiece *)(T + o_pieces), NP, (unsigned long long *)(T + o_first));
  c->tmark(mark);
  hipMemcpyAsync(first.data(), T + o_first, (size_t)np * 8, hipMemcpyDeviceToHost, st);
  RZ_HIP(hipGetLastError(), "compare launch");
  RZ_HIP(hipStreamSynchronize(st), "compare");
  return 0;
}

int zip_place_pieces(Ctx *c, const std::vector<uint8_t> &blob, std::vector<ZwPiece> &pieces, const char *mark);      // zada_zip.hip

}  // namespace zada

using namespace zada;

int zada_compare_device(zada_ctx *z, const void *d_a, const void *d_b, uint64_t n, uint64_t *first_diff) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;                                            // (as every entry point: zada_lzma_export_state)
  if (!first_diff || (n && (!d_a || !d_b))) { c->err = "zada_compare_device: null argument"; return ZADA_E_INVALID; }
  if (n >= UZ_MAX_BYTES) { c->err = "zada_compare_device: buffers of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  *first_diff = 0;
  if (n == 0) { hipStreamSynchronize(c->stream); return ZADA_OK; }
  RzState *S = rz_state(c);
  if (!S) { c->err = "compare: no memory for the tables"; return ZADA_E_NOMEM; }
  std::vector<CzPair> pairs(1, CzPair{(uint64_t)(uintptr_t)d_a, (uint64_t)(uintptr_t)d_b, n});
  std::vector<UzPiece> none;
  std::vector<uint64_t> first;
  c->tbegin();
  c->tmark("compare:begin");
  const int rc = cz_run(c, S, pairs, none, first, "compare:k_cz_compare");
  c->tend();
  if (rc) { hipStreamSynchronize(c->stream); (void)hipGetLastError(); return rc; }
  *first_diff = first[0];
  return ZADA_OK;
}

int zada_compzip_device(zada_ctx *z, const void *d_archive_a, uint64_t len_a, const void *d_archive_b, uint64_t len_b, int count,
                        const zada_unzip_entry *a, const zada_unzip_entry *b, const uint32_t keys0[3], zada_compzip_result *res) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (count && (!a || !b || !res)) { c->err = "zada_compzip_device: null argument"; return ZADA_E_INVALID; }
  if ((len_a && !d_archive_a) || (len_b && !d_archive_b)) { c->err = "zada_compzip_device: null archive"; return ZADA_E_INVALID; }
  int bad = -1, side = 0, why = 0;
  int rc = cz_check(a, b, count, len_a, len_b, keys0 != nullptr, &bad, &side, &why, c->knob_unzip_legacy);
  if (rc) {
    char buf[200];
    snprintf(buf, sizeof buf, "zada_compzip_device: pair %d, archive %d: %s", bad, side, uz_why_text(why, c->knob_unzip_legacy));
    c->err = buf;
    return rc;
  }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  if (count == 0) { hipStreamSynchronize(c->stream); return ZADA_OK; }
  RzState *S = rz_state(c);
  if (!S) { c->err = "compzip: no memory for the tables"; return ZADA_E_NOMEM; }
  std::vector<std::pair<const char *, float>> times;               // last_timing: the launches of every group and side of the call, equal names added up
  auto gather = [&]() {
    for (const auto &t : c->timing) {
      size_t k = 0;
      while (k < times.size() && strcmp(times[k].first, t.first)) k++;
      if (k < times.size()) times[k].second += t.second; else times.push_back(t);
    }
    c->timing.clear();
  };
  std::vector<int> ends;
  cz_groups(a, b, count, (uint64_t)c->knob_batch_mib << 20, ends);
  std::vector<zada_unzip_entry> ea, eb;
  std::vector<zada_unzip_result> ra, rb;
  std::vector<int> idx;
  std::vector<CzPair> pairs;
  std::vector<uint64_t> plen, first;
  std::vector<uint32_t> pid, pk;
  std::vector<UzPiece> pieces;
  std::vector<uint64_t> pfirst;
  int g0 = 0;
  for (int g1 : ends) {
    ea.clear(); eb.clear(); idx.clear();
    uint64_t bytes = 0;
    for (int i = g0; i < g1; i++) {
      zada_compzip_result &R = res[i];
      R = zada_compzip_result{ZADA_CZ_OK, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0, 0};
      if (cz_absent(b[i])) { R.verdict = ZADA_CZ_MISSING; continue; }
      zada_unzip_entry x = a[i], y = b[i];
      x.out_off = y.out_off = bytes;
      x.flags &= x.method == 6 ? 7u : 3u; y.flags &= y.method == 6 ? 7u : 3u;   // (an Implode row keeps its general-purpose bit 2)
      bytes += cz_slot(a[i], b[i]);
      ea.push_back(x); eb.push_back(y); idx.push_back(i);
    }
    g0 = g1;
    const int n = (int)idx.size();
    if (!n) continue;
    rc = dev_grow(c, S->arena_a, bytes + 16, "hipMalloc (compzip arena 1)");
    if (!rc) rc = dev_grow(c, S->arena_b, bytes + 16, "hipMalloc (compzip arena 2)");
    if (rc) return rc;
    ra.assign(n, zada_unzip_result{0, 0xFFFFFFFFu, 0, 0}); rb = ra;
    // both sides through the reader's launches; a return value that no entry carries is what stopped the call
    for (int s = 0; s < 2; s++) {
      std::vector<zada_unzip_result> &r = s ? rb : ra;
      rc = zada_unzip_device(z, s ? d_archive_b : d_archive_a, s ? len_b : len_a, s ? S->arena_b.p : S->arena_a.p, bytes, n, s ? eb.data() : ea.data(), keys0, r.data());
      gather();
      bool entrys = false;
      for (int k = 0; k < n && rc; k++) entrys = entrys || r[k].rc == rc;
      if (rc && !entrys) return rc;
    }
    pairs.clear(); plen.clear(); pid.clear(); pk.clear();
    for (int k = 0; k < n; k++) {
      zada_compzip_result &R = res[idx[k]];
      R.rc_a = ra[k].rc; R.rc_b = rb[k].rc; R.crc_a = ra[k].crc; R.crc_b = rb[k].crc; R.len_a = ra[k].out_len; R.len_b = rb[k].out_len;
      if (R.rc_a || R.rc_b) { R.verdict = ZADA_CZ_DAMAGED; continue; }
      const uint64_t m = R.len_a < R.len_b ? R.len_a : R.len_b;
      pid.push_back((uint32_t)pairs.size()); pk.push_back((uint32_t)k); plen.push_back(m);
      pairs.push_back(CzPair{(uint64_t)(uintptr_t)S->arena_a.p + ea[k].out_off, (uint64_t)(uintptr_t)S->arena_b.p + eb[k].out_off, m});
    }
    if (pairs.empty()) continue;
    uz_pieces(plen.data(), pid.data(), (uint32_t)pairs.size(), CZ_PIECE_LOG, pieces, pfirst);
    if (pieces.empty()) first.assign(plen.begin(), plen.end());      // (every pair of the group is empty on one side)
    else {
      c->tbegin();
      c->tmark("compzip:begin");
      rc = cz_run(c, S, pairs, pieces, first, "compzip:k_cz_compare");
      c->tend();
      gather();
      if (rc) { hipStreamSynchronize(c->stream); (void)hipGetLastError(); return rc; }
    }
    for (size_t p = 0; p < pairs.size(); p++) {
      zada_compzip_result &R = res[idx[pk[p]]];
      R.verdict = cz_verdict(R.len_a, R.len_b, first[p], &R.position, &R.compared);
    }
  }
  hipStreamSynchronize(c->stream);
  c->timing = times;
  return ZADA_OK;
}

// ---- ReZip ----
uint64_t zada_rezip_bound(int count, const zada_rezip_entry *ent, uint64_t comment_len) { return rz_bound(count < 0 || !ent ? 0 : count, ent, comment_len); }

namespace {
struct RzWinner { uint64_t src, csize; uint16_t zip_type; bool eos; };
struct RzRun {
  zada_ctx *z; Ctx *c; RzState *S; const uint8_t *src; uint64_t src_len; const zada_rezip_entry *ent; uint32_t considered, formats;
  uint8_t *archive; uint64_t cap; RzArchive A; zada_rezip_result *res; uint64_t *sizes;
  std::vector<int> p2, p1;
  std::vector<std::pair<const char *, float>> times;
  void gather() {                                                    // last_timing: the launches of every call below, equal names added up
    for (const auto &t : c->timing) {
      size_t k = 0;
      while (k < times.size() && strcmp(times[k].first, t.first)) k++;
      if (k < times.size()) times[k].second += t.second; else times.push_back(t);
    }
    c->timing.clear();
  }
};
int rz_fail(RzRun &R, int rc, int i, const char *what) {
  char buf[200];
  snprintf(buf, sizeof buf, "zada_rezip_device: entry %d: %s", i, what);
  R.c->err = buf;
  return rc;
}
// the kept entries idx of one group: extracted, every distinct method run once over the entries that need it, the winners placed
int rz_group(RzRun &R, const std::vector<int> &idx) {
  Ctx *c = R.c;
  const int n = (int)idx.size();
  // 1. extract, and hold size and CRC-32 against the directory (UnZip.Extract raises there)
  std::vector<zada_unzip_entry> ue(n);
  std::vector<zada_unzip_result> ur(n, zada_unzip_result{0, 0xFFFFFFFFu, 0, 0});
  uint64_t bytes = 0;
  for (int k = 0; k < n; k++) {
    const zada_rezip_entry &e = R.ent[idx[k]];
    ue[k] = zada_unzip_entry{e.in_off, e.n_in, bytes, e.method == 0 ? e.n_in : e.usize, e.method, (uint8_t)(e.flags & (e.method == 6 ? 6u : 2u)), 0, 0};   // (Implode: bits 1 and 2 say how it is read)
    bytes += uz_slot(ue[k].cap);
  }
  int rc = dev_grow(c, R.S->arena_a, bytes + 16, "hipMalloc (rezip extraction arena)");
  if (rc) return rc;
  uint8_t *arena = R.S->arena_a.p;
  rc = zada_unzip_device(R.z, R.src, R.src_len, arena, bytes, n, ue.data(), nullptr, ur.data());
  R.gather();
  if (rc) {                                                          // a return value that no entry carries is what stopped the call
    bool entrys = false;
    for (int k = 0; k < n; k++) entrys = entrys || ur[k].rc == rc;
    if (!entrys) return rc;
  }
  for (int k = 0; k < n; k++) {
    const zada_rezip_entry &e = R.ent[idx[k]];
    if (ur[k].rc) return rz_fail(R, ZADA_E_DATA, idx[k], "its data do not decode");
    if (ur[k].out_len != e.usize) return rz_fail(R, ZADA_E_DATA, idx[k], "its decoded length is not what the directory promises");
    if ((ur[k].crc ^ 0xFFFFFFFFu) != e.crc) return rz_fail(R, ZADA_E_DATA, idx[k], "its CRC-32 is not the directory's");
  }
  // 2. sizes of original; the methods to run
  std::vector<uint64_t> size((size_t)n * RZ_NA, RZ_NOT_TRIED);
  std::vector<RzWinner> best(n);
  std::vector<std::vector<int>> need(n);
  std::vector<int> methods;
  for (int k = 0; k < n; k++) {
    const zada_rezip_entry &e = R.ent[idx[k]];
    size[(size_t)k * RZ_NA] = e.n_in;
    best[k] = RzWinner{(uint64_t)(uintptr_t)R.src + e.in_off, e.n_in, e.method, e.method == 14 && (e.flags & 2u)};
    rz_methods(R.considered, R.p2[idx[k]], R.p1[idx[k]], need[k], e.usize);
    methods.insert(methods.end(), need[k].begin(), need[k].end());
  }
  std::sort(methods.begin(), methods.end());
  methods.erase(std::unique(methods.begin(), methods.end()), methods.end());
  // the holding buffer: per method the bound of a zada_zip_device_ex archive of its entries (nameless: 30 + 46 bytes of headers each, 98 of end records)
  std::vector<uint64_t> hold_at(methods.size() + 1, 0);
  std::vector<std::vector<int>> users(methods.size());
  std::vector<std::vector<zada_zip_entry>> tabs(methods.size());
  for (size_t m = 0; m < methods.size(); m++) {
    for (int k = 0; k < n; k++)
      if (std::find(need[k].begin(), need[k].end(), methods[m]) != need[k].end()) {
        users[m].push_back(k);
        tabs[m].push_back(zada_zip_entry{R.ent[idx[k]].usize ? arena + ue[k].out_off : nullptr, R.ent[idx[k]].usize, nullptr, 0, 0, 0});
      }
    hold_at[m + 1] = hold_at[m] + ((zada_zip_bound_ex((int)tabs[m].size(), tabs[m].data(), 0, 0) + 255) & ~255ull);
  }
  if ((rc = dev_grow(c, R.S->hold, hold_at.back() + 16, "hipMalloc (rezip holding buffer)"))) return rc;
  // 3. every distinct method once, ascending; the (size, rank) leaders of an entry are read off when all have run (nothing in the buffer moves)
  for (size_t m = 0; m < methods.size(); m++) {
    const int cnt = (int)tabs[m].size();
    uint8_t *at = R.S->hold.p + hold_at[m];
    std::vector<zada_zip_result> zr(cnt);
    std::vector<uint8_t> refused(cnt, 0);
    uint64_t alen = 0;
    rc = zada_zip_device_ex(R.z, methods[m], cnt, tabs[m].data(), at, hold_at[m + 1] - hold_at[m], 0, nullptr, &alen, zr.data());
    R.gather();
    if (rc == ZADA_E_REFERENCE) {
      // LZMA_3: the coder refuses an entry.  One by one: the refused entries lose this approach, the others keep their streams
      uint64_t pos = 0;
      for (int j = 0; j < cnt; j++) {
        rc = zada_zip_device_ex(R.z, methods[m], 1, &tabs[m][j], at + pos, hold_at[m + 1] - hold_at[m] - pos, 0, nullptr, &alen, &zr[j]);
        R.gather();
        if (rc == ZADA_E_REFERENCE) { refused[j] = 1; continue; }
        if (rc) return rc;
        zr[j].offset += pos;
        pos += (30 + zr[j].csize + 15) & ~15ull;                     // (the next one overwrites this one's directory)
      }
      rc = 0;
    }
    if (rc) return rc;
    for (int j = 0; j < cnt; j++) {
      const int k = users[m][j];
      if (refused[j]) { R.res[idx[k]].flags |= 2u; continue; }
      const uint64_t stream = (uint64_t)(uintptr_t)at + zr[j].offset + zw_local_len(tabs[m][j], zr[j].offset);
      for (int a = 1; a < RZ_NA; a++) {
        if (!((rz_considered_entry(R.considered, R.ent[idx[k]].usize) >> a) & 1u) || rz_method_of(a, R.p2[idx[k]], R.p1[idx[k]]) != methods[m]) continue;
        uint64_t *sz = &size[(size_t)k * RZ_NA];
        sz[a] = zr[j].csize;
        bool lead = true;                                             // smallest (size, rank) among the approaches other than original so far
        for (int b = 1; b < RZ_NA; b++) if (b != a && sz[b] != RZ_NOT_TRIED && (sz[b] < sz[a] || (sz[b] == sz[a] && b < a))) lead = false;
        if (lead) best[k] = RzWinner{stream, zr[j].csize, zr[j].zip_type, zr[j].zip_type == 14};
      }
    }
  }
  // 4. the choice, the headers, one placement
  std::vector<uint8_t> blob;
  std::vector<ZwPiece> pieces;
  for (int k = 0; k < n; k++) {
    const int i = idx[k];
    const zada_rezip_entry &e = R.ent[i];
    const uint64_t *sz = &size[(size_t)k * RZ_NA];
    const int a = rz_choose(sz, rz_original_allowed(R.formats, e.method));
    if (a == RZ_ORIGINAL) best[k] = RzWinner{(uint64_t)(uintptr_t)R.src + e.in_off, e.n_in, e.method, e.method == 14 && (e.flags & 2u)};
    const RzWinner &W = best[k];
    const uint64_t dst = R.A.pos, hat = blob.size();
    const uint32_t hl = rz_add(R.A, e, W.csize, W.zip_type, W.eos, blob, a == RZ_ORIGINAL);
    if (R.A.pos > R.cap) { c->err = "zada_rezip_device: archive buffer too small"; return ZADA_E_INVALID; }
    zw_cut(hat, (uint64_t)(uintptr_t)R.archive + dst, hl, pieces);
    for (size_t q = pieces.size() - zw_piece_count(hl); q < pieces.size(); q++) pieces[q].pad = 1;
    zw_cut(W.src, (uint64_t)(uintptr_t)R.archive + dst + hl, W.csize, pieces);
    R.res[i].rc = ZADA_OK; R.res[i].approach = a; R.res[i].zip_type = W.zip_type; R.res[i].crc = e.crc; R.res[i].csize = W.csize; R.res[i].offset = R.A.base + dst;
    if (R.sizes) memcpy(R.sizes + (size_t)i * RZ_NA, sz, sizeof(uint64_t) * RZ_NA);
  }
  c->tbegin(); c->tmark("begin");
  rc = zip_place_pieces(c, blob, pieces, "rezip:k_zw_place");
  c->tend();
  R.gather();
  return rc;
}
}  // namespace

int zada_rezip_device(zada_ctx *z, const void *d_src, uint64_t src_len, int count, const zada_rezip_entry *ent, uint32_t approaches, uint32_t formats,
                      void *d_archive, uint64_t cap, uint64_t archive_base, const uint8_t *comment, uint32_t comment_len, uint64_t *archive_len,
                      zada_rezip_result *res, uint64_t *sizes) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (!archive_len || (count && (!ent || !res)) || (comment_len && !comment)) { c->err = "zada_rezip_device: null argument"; return ZADA_E_INVALID; }
  if (!d_archive || (src_len && !d_src)) { c->err = "zada_rezip_device: null archive"; return ZADA_E_INVALID; }
  if ((approaches & RZ_UNBUILT) && !c->knob_zip_legacy) {
    c->err = std::string("zada_rezip_device: approach ") + ((approaches >> RZ_SHRINK) & 1u ? "shrink (Shrink_1)" : "reduce_4 (Reduce_4)") + " is not taken by the device writer";
    return ZADA_E_INVALID;
  }
  if (approaches >> RZ_NA || formats >> 5 || comment_len > 65535u) { c->err = "zada_rezip_device: approaches, formats or comment length out of range"; return ZADA_E_INVALID; }
  int bad = -1, why = 0;
  int rc = rz_check(ent, count, (uint64_t)(uintptr_t)d_src, src_len, (uint64_t)(uintptr_t)d_archive, cap, &bad, &why, c->knob_unzip_legacy);
  if (rc) {
    char buf[240];
    if (bad >= 0) snprintf(buf, sizeof buf, "zada_rezip_device: entry %d: %s", bad, rz_why_text(why, c->knob_unzip_legacy));
    else snprintf(buf, sizeof buf, "zada_rezip_device: %s", rz_why_text(why));
    c->err = buf;
    return rc;
  }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  RzState *S = rz_state(c);
  if (!S) { c->err = "rezip: no memory for the tables"; return ZADA_E_NOMEM; }
  RzRun R;
  R.z = z; R.c = c; R.S = S; R.src = (const uint8_t *)d_src; R.src_len = src_len; R.ent = ent; R.formats = formats;
  R.considered = rz_considered(approaches | 1u, formats, c->knob_zip_legacy);
  R.archive = (uint8_t *)d_archive; R.cap = cap; R.A.base = archive_base; R.res = res; R.sizes = sizes;
  R.p2.assign(count, 0); R.p1.assign(count, 0);
  for (int i = 0; i < count; i++) {
    res[i] = zada_rezip_result{ZADA_OK, 0, 0, (uint16_t)(rz_dropped(ent[i]) ? 1 : 0), ent[i].crc, 0, 0};
    if (sizes) for (int a = 0; a < RZ_NA; a++) sizes[(size_t)i * RZ_NA + a] = RZ_NOT_TRIED;
    // Process_Internal_Raw passes content_hint = Guess_Type_from_Name (name) and the known size (the name's bytes copied: not NUL-terminated there)
    const std::string nm(ent[i].name_len ? (const char *)ent[i].name : "", ent[i].name_len);
    const int hint = zada_guess_type_from_name(nm.c_str());
    R.p2[i] = zada_preselect(ZADA_PRESELECTION_2, hint, 1, ent[i].usize);
    R.p1[i] = zada_preselect(ZADA_PRESELECTION_1, hint, 1, ent[i].usize);
  }
  auto stop = [&](int r) { hipStreamSynchronize(c->stream); hipStreamSynchronize(c->stream2); (void)hipGetLastError(); c->rg.open = false; return r == ZADA_E_HIP_ ? ZADA_E_HIP : r; };
  std::vector<int> ends, idx;
  rz_groups(ent, count, (uint64_t)c->knob_batch_mib << 20, ends);
  int g0 = 0;
  for (int g1 : ends) {
    idx.clear();
    for (int i = g0; i < g1; i++) if (!rz_dropped(ent[i])) idx.push_back(i);
    g0 = g1;
    if (idx.empty()) continue;
    if ((rc = rz_group(R, idx))) return stop(rc);
  }
  const uint64_t at = R.A.pos;
  std::vector<uint8_t> tail;
  rz_finish(R.A, comment, comment_len, tail);
  if (R.A.pos > cap) { c->err = "zada_rezip_device: archive buffer too small"; return stop(ZADA_E_INVALID); }
  hipMemcpyAsync(R.archive + at, tail.data(), tail.size(), hipMemcpyHostToDevice, c->stream);
  if (hip_check(c, hipStreamSynchronize(c->stream), "rezip directory")) return ZADA_E_HIP;
  c->timing = R.times;
  *archive_len = R.A.pos;
  return ZADA_OK;
}
