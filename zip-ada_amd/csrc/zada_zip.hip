// zada_zip.hip -- zada_zip_device: the entries of an archive where they lie in device memory, written as one Zip archive into device memory.
//
// The host side is a plan (zada_zip_plan.h: argument checks, groups, every header byte, the copy jobs) and a sequence of launches per group of
// consecutive entries; no entry byte crosses the host.  A group of small entries goes through the launches of zada_deflate_batch (batch_layout /
// batch_launch, zada_api.hip), a large entry or a group of one through those of zada_deflate_device (deflate_device_one: only an entry longer than
// "span_mib" at a 16-byte-aligned address is compressed straight to its place; every other one into the workspace and from there by one copy of the
// runtime's, an unaligned one after a copy of its own into the workspace), method Store through the archive reader's k_uz_store / k_uz_fold
// (unzip_store_entries).  last_timing holds the launches of all groups of a call, the times of equal names added up.  What is new here:
// k_zw_pack: every entry of a group gathered from its address, at any alignment, into its 32 KiB-aligned slot of the LZ buffer: one wave per piece of
//   16 KiB stages the piece through LDS with aligned 16-byte loads and stores it with 16-byte stores.  The slots' tails stay as they are.
// k_zw_place: a table-driven copy, one wave per piece of at most 16 KiB from any alignment to any alignment: the local headers out of the blob the
//   host uploads, the Deflate streams out of the workspace, a stored entry's bytes from where they lie.  It writes only the bytes of its piece: head
//   and tail byte-wise, the middle in 16-byte stores whose words are put together from the staged piece's 4-byte words.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <new>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_zip_plan.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {

constexpr uint32_t ZW_WAVE = 64;
typedef __attribute__((address_space(1))) uint8_t zw_gu8;
typedef __attribute__((address_space(1))) const uint8_t zw_gcu8;
typedef uint32_t zw_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) zw_u32x4 zw_gu4;
typedef __attribute__((address_space(1))) const zw_u32x4 zw_gcu4;

struct ZwPackEnt { uint64_t src; uint32_t start, pad; };           // an entry's bytes; its slot's offset in the LZ buffer
struct ZwPackPiece { uint32_t entry, off, len, pad; };             // bytes [off, off + len) of the entry, 1 <= len <= ZW_PIECE

// len bytes (1 .. ZW_PIECE) from src to dst by one wave, through `lds` (ZW_PIECE + 32 bytes, 16-byte aligned): the piece lies there behind sh bytes,
// sh = the source's offset in its 16-byte word, so that the aligned loads land on aligned LDS words.
__device__ __forceinline__ void zw_copy(zw_gcu8 *src, zw_gu8 *dst, uint32_t len, uint8_t *lds) {
  const uint32_t lane = threadIdx.x;
  const uint32_t sh = (uint32_t)((uintptr_t)src & 15u);
  uint32_t h = (16u - sh) & 15u;
  if (h > len) h = len;
  if (lane < h) lds[sh + lane] = src[lane];
  const uint32_t words = (len - h) / 16u;
  {
    zw_gcu4 *s4 = (zw_gcu4 *)(src + h);
    uint8_t *l0 = lds + sh + h;                          // (a multiple of 16 whenever there is a word)
#pragma unroll 4
    for (uint32_t w = lane; w < words; w += ZW_WAVE) *(zw_u32x4 *)(l0 + 16u * w) = s4[w];
  }
  for (uint32_t i = h + words * 16u + lane; i < len; i += ZW_WAVE) lds[sh + i] = src[i];
  __syncthreads();
  const uint32_t da = (uint32_t)((uintptr_t)dst & 15u);
  uint32_t hd = (16u - da) & 15u;
  if (hd > len) hd = len;
  if (lane < hd) dst[lane] = lds[sh + lane];
  const uint32_t dwords = (len - hd) / 16u, qb = sh + hd;
  zw_gu4 *d4 = (zw_gu4 *)(dst + hd);
  if ((qb & 15u) == 0) {
#pragma unroll 4
    for (uint32_t w = lane; w < dwords; w += ZW_WAVE) d4[w] = *(const zw_u32x4 *)(lds + qb + 16u * w);
  } else {
    // five aligned 4-byte words hold the sixteen bytes; each output word is the funnel shift of two neighbours (the fifth word may lie up to four
    // bytes behind the piece, inside the buffer; its bytes are shifted out)
    const uint32_t r = (qb & 3u) * 8u;
    const uint32_t *lw = (const uint32_t *)(lds + (qb & ~3u));
#pragma unroll 2
    for (uint32_t w = lane; w < dwords; w += ZW_WAVE) {
      const uint32_t *p = lw + 4u * w;
      const uint32_t a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3], a4 = p[4];
      zw_u32x4 x;
      x.x = (uint32_t)((((uint64_t)a1 << 32) | a0) >> r); x.y = (uint32_t)((((uint64_t)a2 << 32) | a1) >> r);
      x.z = (uint32_t)((((uint64_t)a3 << 32) | a2) >> r); x.w = (uint32_t)((((uint64_t)a4 << 32) | a3) >> r);
      d4[w] = x;
    }
  }
  for (uint32_t i = hd + dwords * 16u + lane; i < len; i += ZW_WAVE) dst[i] = lds[sh + i];
}

__global__ void __launch_bounds__(ZW_WAVE) k_zw_pack(const ZwPackPiece *__restrict__ pieces, const ZwPackEnt *__restrict__ ents, uint8_t *in) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[ZW_PIECE + 32];
  const ZwPackPiece P = pieces[blockIdx.x];
  const ZwPackEnt E = ents[P.entry];
  zw_copy((zw_gcu8 *)(E.src + P.off), (zw_gu8 *)(in + E.start + P.off), P.len, lds);
}

__global__ void __launch_bounds__(ZW_WAVE) k_zw_place(const ZwPiece *__restrict__ pieces) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[ZW_PIECE + 32];
  const ZwPiece P = pieces[blockIdx.x];
  zw_copy((zw_gcu8 *)P.src, (zw_gu8 *)P.dst, P.len, lds);
}

// ---- host side ----
struct ZwState { uint8_t *tab = nullptr; uint64_t cap = 0; };      // device: the tables of k_zw_pack, then the header blob and the pieces of k_zw_place

void zip_destroy(Ctx *c) {
  ZwState *S = (ZwState *)c->zw;
  if (!S) return;
  if (S->tab) hipFree(S->tab);
  delete S;
  c->zw = nullptr;
}
static int zw_grow(Ctx *c, ZwState *S, uint64_t bytes) {
  if (S->tab && S->cap >= bytes) return 0;
  hipStreamSynchronize(c->stream);
  if (S->tab) hipFree(S->tab);
  S->tab = nullptr; S->cap = 0;
  const uint64_t want = ((bytes < (1u << 20) ? (1u << 20) : bytes + bytes / 4) + 65535) & ~65535ull;
  if (hipMalloc((void **)&S->tab, want) != hipSuccess) { (void)hipGetLastError(); c->err = "hipMalloc (zip tables)"; return ZADA_E_NOMEM; }
  S->cap = want;
  return 0;
}
static uint64_t zw_up256(uint64_t v) { return (v + 255) & ~255ull; }

#define ZW_HIP(call, what) do { if (hip_check(c, (call), what)) return ZADA_E_HIP_; } while (0)

struct ZwCall {                      // what one zada_zip_device call works on
  Ctx *c; ZwState *S; int method; const zada_zip_entry *ent; zada_zip_result *res; uint8_t *archive; uint64_t cap; ZwArchive A;
};
static int zw_too_small(Ctx *c) { c->err = "zada_zip_device: archive buffer too small"; return ZADA_E_INVALID; }

// the blob and the pieces of the jobs go up; k_zw_place
static int zw_place(ZwCall &Z, const std::vector<uint8_t> &blob, const std::vector<ZwJob> &jobs, bool with_payloads) {
  Ctx *c = Z.c;
  const uint64_t o_pieces = zw_up256(blob.size());
  std::vector<ZwPiece> pieces;
  // (the blob's address is known once the table has its size: cut with offsets first)
  for (const ZwJob &J : jobs) {
    if (J.kind != ZW_SRC_BLOB && !with_payloads) continue;
    const uint64_t src = J.kind == ZW_SRC_BLOB ? J.src : J.kind == ZW_SRC_STREAM ? (uint64_t)(uintptr_t)c->ws.out + J.src : (uint64_t)(uintptr_t)Z.ent[J.entry].d_data;
    zw_cut(src, (uint64_t)(uintptr_t)Z.archive + J.dst, J.len, pieces);
    if (J.kind == ZW_SRC_BLOB) for (size_t k = pieces.size() - zw_piece_count(J.len); k < pieces.size(); k++) pieces[k].pad = 1;
  }
  if (pieces.empty()) return 0;
  if (pieces.size() >= (1ull << 31)) { c->err = "zada_zip_device: more pieces to place than 2 ** 31"; return ZADA_E_TOO_LARGE; }
  const int rc = zw_grow(c, Z.S, o_pieces + pieces.size() * sizeof(ZwPiece));
  if (rc) return rc;
  for (ZwPiece &P : pieces) if (P.pad) { P.src += (uint64_t)(uintptr_t)Z.S->tab; P.pad = 0; }
  hipMemcpyAsync(Z.S->tab, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream);
  hipMemcpyAsync(Z.S->tab + o_pieces, pieces.data(), pieces.size() * sizeof(ZwPiece), hipMemcpyHostToDevice, c->stream);
  hipLaunchKernelGGL(k_zw_place, dim3((uint32_t)pieces.size()), dim3(ZW_WAVE), 0, c->stream, (const ZwPiece *)(Z.S->tab + o_pieces));
  c->tmark("zip:k_zw_place");
  ZW_HIP(hipGetLastError(), "zip place launch");
  ZW_HIP(hipStreamSynchronize(c->stream), "zip place");              // (the tables are the host's until then)
  return 0;
}

// a group of small entries: gathered, through the launches of a batch, placed (between tbegin and tend of zw_batch_group)
static int zw_batch_body(ZwCall &Z, int g0, int g1, const BatchLayout &L, const std::vector<uint64_t> &lens) {
  Ctx *c = Z.c;
  const uint32_t E = (uint32_t)(g1 - g0);
  std::vector<ZwPackEnt> pe(E);
  std::vector<ZwPackPiece> pp;
  for (uint32_t e = 0; e < E; e++) {
    pe[e] = ZwPackEnt{(uint64_t)(uintptr_t)Z.ent[g0 + e].d_data, L.start[e], 0};
    for (uint64_t o = 0; o < lens[e]; o += ZW_PIECE) pp.push_back(ZwPackPiece{e, (uint32_t)o, (uint32_t)(lens[e] - o < ZW_PIECE ? lens[e] - o : ZW_PIECE), 0});
  }
  const uint64_t o_pp = zw_up256((uint64_t)E * sizeof(ZwPackEnt));
  int rc = zw_grow(c, Z.S, o_pp + pp.size() * sizeof(ZwPackPiece));
  if (rc) return rc;
  if (!pp.empty()) {
    hipMemcpyAsync(Z.S->tab, pe.data(), (size_t)E * sizeof(ZwPackEnt), hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(Z.S->tab + o_pp, pp.data(), pp.size() * sizeof(ZwPackPiece), hipMemcpyHostToDevice, c->stream);
    hipLaunchKernelGGL(k_zw_pack, dim3((uint32_t)pp.size()), dim3(ZW_WAVE), 0, c->stream, (const ZwPackPiece *)(Z.S->tab + o_pp), (const ZwPackEnt *)Z.S->tab, c->ws.in);
    c->tmark("zip:k_zw_pack");
  }
  uint64_t obytes = 0;
  uint32_t *h_bytes, *h_base, *h_crc;
  rc = batch_launch(c, Z.method, L, &obytes, &h_bytes, &h_base, &h_crc);
  if (rc) return rc;
  ZW_HIP(hipGetLastError(), "zip batch launch");
  ZW_HIP(hipStreamSynchronize(c->stream), "zip batch");
  // the verdicts: offsets, Store fallbacks, headers, jobs
  std::vector<uint8_t> blob;
  std::vector<ZwJob> jobs;
  zw_group_place(Z.A, Z.ent, g0, g1, h_bytes, h_base, h_crc, blob, jobs, Z.res);
  if (Z.A.pos > Z.cap) return zw_too_small(c);
  return zw_place(Z, blob, jobs, true);
}
static int zw_batch_group(ZwCall &Z, int g0, int g1) {
  Ctx *c = Z.c;
  const uint32_t E = (uint32_t)(g1 - g0);
  std::vector<uint64_t> lens(E);
  for (uint32_t e = 0; e < E; e++) lens[e] = Z.ent[g0 + e].n;
  BatchLayout L;
  int rc = batch_layout(c, E, lens.data(), nullptr, L);
  if (rc) return rc;
  batch_segends_all(c, L);
  c->tbegin(); c->tmark("begin");
  rc = zw_batch_body(Z, g0, g1, L, lens);
  c->tmark("end"); c->tend();                            // (on every way out: a tbegin has its tend)
  return rc;
}

// one entry through the single-stream path (deflate_device_one), its stream written behind its local header: straight to its place where the entry is
// longer than "span_mib" and lies at a 16-byte-aligned address, otherwise into the workspace and from there by one device-to-device copy (an
// unaligned entry is first copied into the workspace itself).  The header, which holds the CRC and the sizes, is written afterwards.
static int zw_single(ZwCall &Z, int i) {
  Ctx *c = Z.c;
  const zada_zip_entry &e = Z.ent[i];
  const uint64_t off = Z.A.pos, payoff = off + zw_local_len(e, Z.A.base + off);
  if (payoff > Z.cap) return zw_too_small(c);
  uint32_t reg = 0xFFFFFFFFu;
  uint64_t ol = 0;
  bool stored = true;                                    // (an empty entry: any stream is longer)
  if (e.n) {
    const int rc = deflate_device_one(c, Z.method, e.d_data, e.n, Z.archive + payoff, Z.cap - payoff, &ol, &reg);
    if (rc == ZADA_E_INVALID && c->err == ERR_OUTPUT_TOO_SMALL) return zw_too_small(c);    // (the stream alone is beyond the buffer; any other refusal keeps its text)
    if (rc < 0) return rc;
    stored = rc == ZADA_INEFFICIENT;
  }
  if (payoff + (stored ? e.n : ol) > Z.cap) return zw_too_small(c);
  std::vector<uint8_t> blob;
  std::vector<ZwJob> jobs;
  zw_single_place(Z.A, Z.ent, i, stored, ol, reg, blob, jobs, Z.res);
  for (const ZwJob &J : jobs) {                          // (the runtime's copies: a header of some tens of bytes, or millions of bytes at once)
    if (J.kind == ZW_SRC_BLOB) hipMemcpyAsync(Z.archive + J.dst, blob.data() + J.src, J.len, hipMemcpyHostToDevice, c->stream);
    else if (J.kind == ZW_SRC_DATA) hipMemcpyAsync(Z.archive + J.dst, e.d_data, J.len, hipMemcpyDeviceToDevice, c->stream);
  }
  ZW_HIP(hipStreamSynchronize(c->stream), "zip entry");
  return 0;
}

// method Store: the payloads copied and summed by the archive reader's kernels, then the headers
static int zw_store_group(ZwCall &Z, int g0, int g1) {
  Ctx *c = Z.c;
  std::vector<uint64_t> src, dst, len;
  std::vector<uint32_t> crc, who, reg((size_t)(g1 - g0), 0xFFFFFFFFu);
  uint64_t pos = Z.A.pos;
  for (int i = g0; i < g1; i++) {
    const zada_zip_entry &e = Z.ent[i];
    pos += zw_local_len(e, Z.A.base + pos);
    if (e.n) { src.push_back((uint64_t)(uintptr_t)e.d_data); dst.push_back((uint64_t)(uintptr_t)Z.archive + pos); len.push_back(e.n); crc.push_back(0xFFFFFFFFu); who.push_back((uint32_t)(i - g0)); }
    pos += e.n;
  }
  if (pos > Z.cap) return zw_too_small(c);
  c->tbegin(); c->tmark("begin");
  int rc = unzip_store_entries(c, (uint32_t)src.size(), src.data(), dst.data(), len.data(), crc.data());
  if (!rc) {
    for (size_t s = 0; s < who.size(); s++) reg[who[s]] = crc[s];
    std::vector<uint8_t> blob;
    std::vector<ZwJob> jobs;
    zw_group_place(Z.A, Z.ent, g0, g1, nullptr, nullptr, reg.data(), blob, jobs, Z.res);
    rc = zw_place(Z, blob, jobs, false);
  }
  c->tmark("end"); c->tend();                            // (on every way out: a tbegin has its tend)
  return rc;
}

}  // namespace zada

using namespace zada;

uint64_t zada_zip_bound(int count, const zada_zip_entry *ent, uint64_t archive_base) { return zw_bound(count < 0 || !ent ? 0 : count, ent, archive_base); }

int zada_zip_device(zada_ctx *z, int method, int count, const zada_zip_entry *ent, void *d_archive, uint64_t cap, uint64_t archive_base,
                    uint64_t *archive_len, zada_zip_result *res) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = c->lz_run_stopped = false;                       // (as every entry point: zada_lzma_export_state)
  char buf[240];
  if (!zw_method_ok(method)) {
    snprintf(buf, sizeof buf, "zada_zip_device: method %d (%s) is not one it takes: Store (0), Deflate_Fixed .. Deflate_R (6 .. 11)", method, zw_method_name(method));
    c->err = buf;
    return ZADA_E_INVALID;
  }
  if (!archive_len || (count && (!ent || !res))) { c->err = "zada_zip_device: null argument"; return ZADA_E_INVALID; }
  if (!d_archive) { c->err = "zada_zip_device: null archive buffer"; return ZADA_E_INVALID; }
  if (count == 0 && archive_base > ZW_M32) {             // (Finish promotes an archive to Zip64 only when it has entries)
    c->err = "zada_zip_device: an empty archive behind more than 4 GiB - 1 bytes has no end record";
    return ZADA_E_INVALID;
  }
  int bad = -1, why = 0;
  int rc = zw_check(ent, count, (uint64_t)(uintptr_t)d_archive, cap, &bad, &why);
  if (rc) {
    snprintf(buf, sizeof buf, "zada_zip_device: entry %d: %s", bad, zw_why_text(why));
    c->err = buf;
    return rc;
  }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  if (!c->zw) c->zw = new (std::nothrow) ZwState();
  if (!c->zw) { c->err = "zip: no memory for the tables"; return ZADA_E_NOMEM; }
  ZwCall Z{c, (ZwState *)c->zw, method, ent, res, (uint8_t *)d_archive, cap, ZwArchive()};
  Z.A.base = archive_base;
  std::vector<ZwGroup> groups;
  zw_groups(ent, count, method, (uint64_t)c->knob_batch_mib << 20, groups);
  auto stop = [&](int r) {                                         // a call that ends early must not leave work in flight on the context's streams
    hipStreamSynchronize(c->stream); hipStreamSynchronize(c->stream2); (void)hipGetLastError(); c->rg.open = false;
    return r;
  };
  std::vector<std::pair<const char *, float>> times;               // last_timing: the launches of every group of the call, equal names added up
  auto gather = [&]() {
    for (const auto &t : c->timing) {
      size_t k = 0;
      while (k < times.size() && strcmp(times[k].first, t.first)) k++;
      if (k < times.size()) times[k].second += t.second; else times.push_back(t);
    }
    c->timing.clear();
  };
  for (const ZwGroup &g : groups) {
    if (g.kind == ZW_G_STORE) rc = zw_store_group(Z, g.g0, g.g1);
    else if (g.kind == ZW_G_SINGLE) rc = zw_single(Z, g.g0);
    else {
      const ZwArchive keep = Z.A;
      rc = zw_batch_group(Z, g.g0, g.g1);
      if (rc == ZADA_E_NOMEM) {                                    // no room for the batch's tables: one by one
        stop(rc);
        Z.A = keep; rc = 0; c->timing.clear();
        for (int i = g.g0; i < g.g1 && !rc; i++) { rc = zw_single(Z, i); gather(); }
      }
    }
    gather();
    if (rc) return stop(rc == ZADA_E_HIP_ ? ZADA_E_HIP : rc);
  }
  // the central directory and the end records: one copy
  const uint64_t at = Z.A.pos;
  std::vector<uint8_t> tail;
  zw_finish(Z.A, tail);
  if (Z.A.pos > cap) return stop(zw_too_small(c));
  hipMemcpyAsync(Z.archive + at, tail.data(), tail.size(), hipMemcpyHostToDevice, c->stream);
  if (hip_check(c, hipStreamSynchronize(c->stream), "zip directory")) return ZADA_E_HIP;
  c->timing = times;
  *archive_len = Z.A.pos;
  return ZADA_OK;
}
