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
// zada_zip_device_ex is the same walk with a method per entry -- BZip2 and LZMA batches on entries gathered by k_zw_pack
// (bzip2_batch_layout / _launch, lzma_batch_layout / _launch, zada_api.hip), Preselection, one launch sequence per distinct method of a group with
// the streams kept in a holding buffer until the group is placed once -- and with passwords: the payloads then go to their place through
// k_zc_place (zada_crypt.hip), an out-of-place Encode.  With the knob "zip_legacy" Shrink_1 and Reduce_1 .. _4 are methods as well: the
// launch group of zada_shrink_batch / zada_reduce_batch (legacy_batch_layout / _launch, zada_api.hip) on entries gathered by k_zw_pack.  Both entry points run the host code below: zada_zip_device is the case of one Store or Deflate
// method for all entries and no password, with its own texts and the launches, marks and bytes it always had.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <new>
#include <vector>
#include <string>
#include <algorithm>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_zip_plan.h"
#include "zada_legacy.h"

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
struct ZwState {
  uint8_t *tab = nullptr; uint64_t cap = 0;        // device: the tables of k_zw_pack, then the header blob and the pieces of k_zw_place
  uint8_t *hold = nullptr; uint64_t hold_cap = 0;  // device: the streams of a group with several methods until the group is placed (zada_zip_device_ex)
};

void zip_destroy(Ctx *c) {
  ZwState *S = (ZwState *)c->zw;
  if (!S) return;
  if (S->tab) hipFree(S->tab);
  if (S->hold) hipFree(S->hold);
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

// ---- the one writer behind zada_zip_device and zada_zip_device_ex: a method per entry, Deflate, BZip2 and LZMA batches on gathered entries, groups
//      with several methods, passwords (zada_zip_device: one method, Store or Deflate, and no password) ----
struct ZxCall {
  const char *who = ""; bool ex = false;   // the entry point's name, for the error texts; it is zada_zip_device_ex
  zada_ctx *z = nullptr; Ctx *c; ZwState *S; const zada_zip_entry *ent; zada_zip_result *res; uint8_t *archive; uint64_t cap; ZwArchive A;
  std::vector<int> m;                  // the method of every entry (Preselection: zada_preselect on its name and size)
  bool enc = false;                    // a password: k0 are its keys, random11 eleven bytes per entry
  uint32_t k0[3] = {0, 0, 0}; const uint8_t *random11 = nullptr;
};
static int zx_too_small(const ZxCall &Z) { Z.c->err = std::string(Z.who) + ": archive buffer too small"; return ZADA_E_INVALID; }
static int zx_hold_grow(Ctx *c, ZwState *S, uint64_t bytes) {
  if (S->hold && S->hold_cap >= bytes) return 0;
  hipStreamSynchronize(c->stream);
  if (S->hold) hipFree(S->hold);
  S->hold = nullptr; S->hold_cap = 0;
  const uint64_t want = ((bytes < (1u << 20) ? (1u << 20) : bytes + bytes / 4) + 65535) & ~65535ull;
  if (hipMalloc((void **)&S->hold, want) != hipSuccess) { (void)hipGetLastError(); c->err = "hipMalloc (zip holding buffer)"; return ZADA_E_NOMEM; }
  S->hold_cap = want;
  return 0;
}
// the encryption header of entry i and the keys behind it, from the entry's final CRC-32 (zip-compress.adb:153-166)
static void zx_header(const ZxCall &Z, int i, uint32_t crc, uint8_t out12[12], uint32_t keys[3]) {
  memcpy(keys, Z.k0, 12);
  zada_crypt_header(keys, Z.random11 + 11 * (size_t)i, crc, out12);
}
// pieces on the context's stream: the tables go up, k_zw_place, and the stream is synchronised (the tables are the host's until then)
static int zx_pieces(ZxCall &Z, const std::vector<uint8_t> &blob, std::vector<ZwPiece> &pieces, const char *mark) {
  Ctx *c = Z.c;
  if (pieces.empty()) return 0;
  if (pieces.size() >= (1ull << 31)) { c->err = std::string(Z.who) + ": more pieces to place than 2 ** 31"; return ZADA_E_TOO_LARGE; }
  const uint64_t o_pieces = zw_up256(blob.size());
  const int rc = zw_grow(c, Z.S, o_pieces + pieces.size() * sizeof(ZwPiece));
  if (rc) return rc;
  for (ZwPiece &P : pieces) if (P.pad) { P.src += (uint64_t)(uintptr_t)Z.S->tab; P.pad = 0; }      // (pad = 1: src counts from the blob)
  if (!blob.empty()) hipMemcpyAsync(Z.S->tab, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream);
  hipMemcpyAsync(Z.S->tab + o_pieces, pieces.data(), pieces.size() * sizeof(ZwPiece), hipMemcpyHostToDevice, c->stream);
  hipLaunchKernelGGL(k_zw_place, dim3((uint32_t)pieces.size()), dim3(ZW_WAVE), 0, c->stream, (const ZwPiece *)(Z.S->tab + o_pieces));
  c->tmark(mark);
  ZW_HIP(hipGetLastError(), "zip place launch");
  ZW_HIP(hipStreamSynchronize(c->stream), "zip place");
  return 0;
}
// the jobs of a group: headers out of the blob, and the payloads (with_payloads) -- plain by k_zw_place, with a password through the out-of-place Encode
// from keys [k], k counted from g0
static int zx_place(ZxCall &Z, int g0, const std::vector<uint8_t> &blob, const std::vector<ZwJob> &jobs, bool with_payloads, const std::vector<uint32_t> &keys) {
  Ctx *c = Z.c;
  std::vector<ZwPiece> pieces;
  std::vector<ZcPlaceJob> coded, large;            // large: a stored entry above ZW_ENTRY_MAX whose copy lies in its place already is encoded there, all waves on it
  for (const ZwJob &J : jobs) {
    const uint64_t dst = (uint64_t)(uintptr_t)Z.archive + J.dst;
    if (J.kind == ZW_SRC_BLOB) {
      zw_cut(J.src, dst, J.len, pieces);
      for (size_t k = pieces.size() - zw_piece_count(J.len); k < pieces.size(); k++) pieces[k].pad = 1;
      continue;
    }
    const uint64_t src = J.kind == ZW_SRC_STREAM ? J.src : (uint64_t)(uintptr_t)Z.ent[J.entry].d_data;
    if (Z.enc) {
      ZcPlaceJob P{src, dst, J.len, {0, 0, 0}, 0};
      memcpy(P.keys, &keys[3 * (size_t)((int)J.entry - g0)], 12);
      if (!with_payloads && J.len > ZW_ENTRY_MAX) large.push_back(P); else coded.push_back(P);
    } else if (with_payloads) zw_cut(src, dst, J.len, pieces);
  }
  int rc = zx_pieces(Z, blob, pieces, "zip:k_zw_place");
  if (rc) return rc;
  if (!coded.empty()) {
    if ((rc = crypt_encode_place(c, (uint32_t)coded.size(), coded.data()))) return rc;
    ZW_HIP(hipStreamSynchronize(c->stream), "zip encode");
  }
  for (ZcPlaceJob &P : large) if ((rc = crypt_encode_device(c, P.keys, (uint8_t *)(uintptr_t)P.dst, P.len))) return rc;
  return 0;
}
// entries idx [k] gathered into their slots base + start [k]
static int zx_pack(ZxCall &Z, const std::vector<int> &idx, const uint64_t *start, uint8_t *base) {
  Ctx *c = Z.c;
  const uint32_t E = (uint32_t)idx.size();
  std::vector<ZwPackEnt> pe(E);
  std::vector<ZwPackPiece> pp;
  for (uint32_t e = 0; e < E; e++) {
    const zada_zip_entry &en = Z.ent[idx[e]];
    pe[e] = ZwPackEnt{(uint64_t)(uintptr_t)en.d_data, (uint32_t)start[e], 0};
    for (uint64_t o = 0; o < en.n; o += ZW_PIECE) pp.push_back(ZwPackPiece{e, (uint32_t)o, (uint32_t)(en.n - o < ZW_PIECE ? en.n - o : ZW_PIECE), 0});
  }
  if (pp.empty()) return 0;
  const uint64_t o_pp = zw_up256((uint64_t)E * sizeof(ZwPackEnt));
  const int rc = zw_grow(c, Z.S, o_pp + pp.size() * sizeof(ZwPackPiece));
  if (rc) return rc;
  // (blocking copies: pe and pp are locals, and the caller goes on to enqueue the method's launches without waiting for the stream)
  ZW_HIP(hipMemcpy(Z.S->tab, pe.data(), (size_t)E * sizeof(ZwPackEnt), hipMemcpyHostToDevice), "zip pack table");
  ZW_HIP(hipMemcpy(Z.S->tab + o_pp, pp.data(), pp.size() * sizeof(ZwPackPiece), hipMemcpyHostToDevice), "zip pack pieces");
  hipLaunchKernelGGL(k_zw_pack, dim3((uint32_t)pp.size()), dim3(ZW_WAVE), 0, c->stream, (const ZwPackPiece *)(Z.S->tab + o_pp), (const ZwPackEnt *)Z.S->tab, base);
  c->tmark("zip:k_zw_pack");
  return 0;
}
// ONE launch sequence for the entries idx of a group that share `method`: V [i - g0] says where entry i's stream lies (until the next launches on the
// context) and how long it is
static int zx_method_run(ZxCall &Z, int method, const std::vector<int> &idx, int g0, std::vector<ZwVerdict> &V) {
  Ctx *c = Z.c;
  const uint32_t E = (uint32_t)idx.size();
  std::vector<uint64_t> lens(E);
  for (uint32_t e = 0; e < E; e++) lens[e] = Z.ent[idx[e]].n;
  int rc;
  char buf[160];
  if (zw_is_bzip2(method) || zw_is_lzma(method)) {
    const bool bz = zw_is_bzip2(method);
    DevBatch D;
    if ((rc = bz ? bzip2_batch_layout(c, method, E, lens.data(), nullptr, D) : lzma_batch_layout(c, method, E, lens.data(), nullptr, D))) return rc;
    if ((rc = zx_pack(Z, idx, D.start.data(), D.d_in))) return rc;
    if ((rc = bz ? bzip2_batch_launch(c, method, D, nullptr, 0) : lzma_batch_launch(c, method, D))) return rc;
    c->tmark(bz ? "bz:end" : "lzma:end");                   // (as in the host-pointer batches: lzma:end is the coder's launch)
    for (uint32_t e = 0; e < E; e++) {
      if (!bz && D.refused[e]) {
        snprintf(buf, sizeof buf, "%s: entry %d: LZMA_3: the reference's matcher reports a match that is none on this entry", Z.who, idx[e]);
        c->err = buf;
        return ZADA_E_REFERENCE;
      }
      V[idx[e] - g0] = ZwVerdict{(uint64_t)(uintptr_t)D.d_out + D.off[e], D.bytes[e], D.reg[e], (uint16_t)(bz ? 12 : 14), 0};
    }
    return 0;
  }
  if (zw_is_legacy(method)) {
    // Shrink_1 / Reduce_1 .. _4: the launch group of zada_shrink_batch / zada_reduce_batch on gathered entries; a stream that does not fit its slot
    // is cut there and stored by the rule of zw_group_place_ex (its length is not below the entry's)
    DevBatch D;
    if ((rc = legacy_batch_layout(c, E, lens.data(), nullptr, D))) return rc;
    if ((rc = zx_pack(Z, idx, D.start.data(), D.d_in))) return rc;
    if ((rc = legacy_batch_launch(c, method, D))) return rc;
    for (uint32_t e = 0; e < E; e++) V[idx[e] - g0] = ZwVerdict{(uint64_t)(uintptr_t)D.d_out + D.off[e], D.bytes[e], D.reg[e], zw_zip_type(method), 0};
    return 0;
  }
  BatchLayout L;
  if ((rc = batch_layout(c, E, lens.data(), nullptr, L))) return rc;
  batch_segends_all(c, L);
  std::vector<uint64_t> start(L.start.begin(), L.start.end());
  if ((rc = zx_pack(Z, idx, start.data(), c->ws.in))) return rc;
  uint64_t obytes = 0;
  uint32_t *h_bytes, *h_base, *h_crc;
  if ((rc = batch_launch(c, method, L, &obytes, &h_bytes, &h_base, &h_crc))) return rc;
  ZW_HIP(hipGetLastError(), "zip batch launch");
  ZW_HIP(hipStreamSynchronize(c->stream), "zip batch");
  for (uint32_t e = 0; e < E; e++) V[idx[e] - g0] = ZwVerdict{(uint64_t)(uintptr_t)c->ws.out + h_base[e], h_bytes[e], h_crc[e], 8, 0};
  return 0;
}
// A group of small entries: per distinct method one launch sequence, in ascending method order; with several methods the streams that beat their input
// move to the holding buffer before the next method reuses the workspace; then the whole group is placed once.
static int zx_batch_body(ZxCall &Z, int g0, int g1) {
  Ctx *c = Z.c;
  std::vector<int> methods(Z.m.begin() + g0, Z.m.begin() + g1);
  std::sort(methods.begin(), methods.end());
  methods.erase(std::unique(methods.begin(), methods.end()), methods.end());
  std::vector<ZwVerdict> V((size_t)(g1 - g0));
  const bool hold = methods.size() > 1;
  uint64_t held = 0;
  int rc;
  if (hold) {
    uint64_t sum = 0;
    for (int i = g0; i < g1; i++) sum += Z.ent[i].n;
    if ((rc = zx_hold_grow(c, Z.S, sum + 16))) return rc;
  }
  for (int method : methods) {
    std::vector<int> idx;
    for (int i = g0; i < g1; i++) if (Z.m[i] == method) idx.push_back(i);
    if ((rc = zx_method_run(Z, method, idx, g0, V))) return rc;
    if (!hold) continue;
    std::vector<ZwPiece> pieces;
    for (int i : idx) {
      ZwVerdict &v = V[i - g0];
      if (v.bytes >= Z.ent[i].n) continue;                           // (it will be stored: nothing to keep)
      const uint64_t to = (uint64_t)(uintptr_t)Z.S->hold + held;
      zw_cut(v.src, to, v.bytes, pieces);
      v.src = to; held += v.bytes;
    }
    if ((rc = zx_pieces(Z, std::vector<uint8_t>(), pieces, "zip:k_zw_place (hold)"))) return rc;
  }
  // the verdicts: encryption headers, offsets, Store fallbacks, local headers, jobs
  std::vector<uint8_t> hdr12, blob;
  std::vector<uint32_t> keys;
  if (Z.enc) {
    hdr12.resize(12 * (size_t)(g1 - g0)); keys.resize(3 * (size_t)(g1 - g0));
    for (int i = g0; i < g1; i++) zx_header(Z, i, V[i - g0].reg ^ 0xFFFFFFFFu, &hdr12[12 * (size_t)(i - g0)], &keys[3 * (size_t)(i - g0)]);
  }
  std::vector<ZwJob> jobs;
  zw_group_place_ex(Z.A, Z.ent, g0, g1, V.data(), Z.enc ? hdr12.data() : nullptr, blob, jobs, Z.res);
  if (Z.A.pos > Z.cap) return zx_too_small(Z);
  return zx_place(Z, g0, blob, jobs, true, keys);
}
static int zx_batch_group(ZxCall &Z, int g0, int g1) {
  Ctx *c = Z.c;
  c->tbegin(); c->tmark("begin");
  const int rc = zx_batch_body(Z, g0, g1);
  c->tmark("end"); c->tend();                            // (on every way out: a tbegin has its tend)
  return rc;
}
// One entry through the single-stream path of its method, its stream written behind its local header (and the 12 bytes of an encryption header), a
// stored one copied there; with a password the payload is then encoded where it lies.  The headers, which hold the CRC and the sizes, come last.
static int zx_single(ZxCall &Z, int i) {
  Ctx *c = Z.c;
  const zada_zip_entry &e = Z.ent[i];
  const int method = Z.m[i];
  const uint64_t off = Z.A.pos, payoff = off + zw_local_len(e, Z.A.base + off) + (Z.enc ? 12 : 0);
  if (payoff > Z.cap) return zx_too_small(Z);
  uint32_t reg = 0xFFFFFFFFu;
  uint64_t ol = 0;
  bool stored = true;                                    // (an empty entry: any stream is longer)
  if (e.n) {
    const int rc = zw_is_legacy(method) ? legacy_device_one(Z.z, method, e.d_data, e.n, Z.archive + payoff, Z.cap - payoff, &ol, &reg, Z.who)
                 : zw_is_bzip2(method) ? bzip2_device_one(c, method, e.d_data, e.n, Z.archive + payoff, Z.cap - payoff, &ol, &reg)
                 : zw_is_lzma(method)  ? lzma_device_one(c, method, e.d_data, e.n, Z.archive + payoff, Z.cap - payoff, &ol, &reg)
                                       : deflate_device_one(c, method, e.d_data, e.n, Z.archive + payoff, Z.cap - payoff, &ol, &reg);
    if (rc == ZADA_E_INVALID && c->err == ERR_OUTPUT_TOO_SMALL) return zx_too_small(Z);    // (the stream alone is beyond the buffer; any other refusal keeps its text)
    if (rc == ZADA_E_REFERENCE) {
      char buf[160];
      snprintf(buf, sizeof buf, "%s: entry %d: LZMA_3: the reference's matcher reports a match that is none on this entry", Z.who, i);
      c->err = buf;
    }
    if (rc < 0) return rc;
    stored = rc == ZADA_INEFFICIENT;
  }
  const uint64_t payload = stored ? e.n : ol;
  if (payoff + payload > Z.cap) return zx_too_small(Z);
  uint8_t hdr12[12];
  uint32_t keys[3];
  if (Z.enc) zx_header(Z, i, reg ^ 0xFFFFFFFFu, hdr12, keys);
  const ZwVerdict v{0, stored ? e.n : ol, reg, zw_zip_type(method), 0};
  std::vector<uint8_t> blob;
  std::vector<ZwJob> jobs;
  zw_group_place_ex(Z.A, Z.ent, i, i + 1, &v, Z.enc ? hdr12 : nullptr, blob, jobs, Z.res);
  for (const ZwJob &J : jobs) {                          // (the runtime's copies; a job of kind ZW_SRC_STREAM lies where it belongs)
    if (J.kind == ZW_SRC_BLOB) hipMemcpyAsync(Z.archive + J.dst, blob.data() + J.src, J.len, hipMemcpyHostToDevice, c->stream);
    else if (J.kind == ZW_SRC_DATA) hipMemcpyAsync(Z.archive + J.dst, e.d_data, J.len, hipMemcpyDeviceToDevice, c->stream);
  }
  ZW_HIP(hipStreamSynchronize(c->stream), "zip entry");
  if (Z.enc && payload) return crypt_encode_device(c, keys, Z.archive + payoff, payload);
  return 0;
}
// method Store: the payloads copied and summed by the archive reader's kernels, then the headers; with a password the cipher text of every entry's own
// bytes then takes the copy's place
static int zx_store_group(ZxCall &Z, int g0, int g1) {
  Ctx *c = Z.c;
  const uint64_t x = Z.enc ? 12 : 0;
  std::vector<uint64_t> src, dst, len;
  std::vector<uint32_t> crc, who;
  std::vector<ZwVerdict> V((size_t)(g1 - g0), ZwVerdict{0, 0, 0xFFFFFFFFu, 0, 0});
  uint64_t pos = Z.A.pos;
  for (int i = g0; i < g1; i++) {
    const zada_zip_entry &e = Z.ent[i];
    pos += zw_local_len(e, Z.A.base + pos) + x;
    if (e.n) { src.push_back((uint64_t)(uintptr_t)e.d_data); dst.push_back((uint64_t)(uintptr_t)Z.archive + pos); len.push_back(e.n); crc.push_back(0xFFFFFFFFu); who.push_back((uint32_t)(i - g0)); }
    pos += e.n;
  }
  if (pos > Z.cap) return zx_too_small(Z);
  c->tbegin(); c->tmark("begin");
  int rc = unzip_store_entries(c, (uint32_t)src.size(), src.data(), dst.data(), len.data(), crc.data());
  if (!rc) {
    for (size_t s = 0; s < who.size(); s++) V[who[s]].reg = crc[s];
    std::vector<uint8_t> hdr12, blob;
    std::vector<uint32_t> keys;
    if (Z.enc) {
      hdr12.resize(12 * (size_t)(g1 - g0)); keys.resize(3 * (size_t)(g1 - g0));
      for (int i = g0; i < g1; i++) zx_header(Z, i, V[i - g0].reg ^ 0xFFFFFFFFu, &hdr12[12 * (size_t)(i - g0)], &keys[3 * (size_t)(i - g0)]);
    }
    std::vector<ZwJob> jobs;
    zw_group_place_ex(Z.A, Z.ent, g0, g1, V.data(), Z.enc ? hdr12.data() : nullptr, blob, jobs, Z.res);
    rc = zx_place(Z, g0, blob, jobs, false, keys);
  }
  c->tmark("end"); c->tend();                            // (on every way out: a tbegin has its tend)
  return rc;
}

// k_zw_place for zada_rezip_device (zada_rezip.hip): the pieces of a group -- pad = 1: src counts from the blob -- placed and waited for
int zip_place_pieces(Ctx *c, const std::vector<uint8_t> &blob, std::vector<ZwPiece> &pieces, const char *mark) {
  if (!c->zw) c->zw = new (std::nothrow) ZwState();
  if (!c->zw) { c->err = "zip: no memory for the tables"; return ZADA_E_NOMEM; }
  ZxCall Z;
  Z.who = "zada_rezip_device"; Z.c = c; Z.S = (ZwState *)c->zw;
  return zx_pieces(Z, blob, pieces, mark);
}

}  // namespace zada

using namespace zada;

// What both entry points do behind their argument checks: the groups one after the other, then the central directory and the end records.
static int zx_run(ZxCall &Z, const std::vector<ZwGroup> &groups, uint64_t *archive_len) {
  Ctx *c = Z.c;
  int rc = 0;
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
    if (g.kind == ZW_G_STORE) rc = zx_store_group(Z, g.g0, g.g1);
    else if (g.kind == ZW_G_SINGLE) rc = zx_single(Z, g.g0);
    else {
      const ZwArchive keep = Z.A;
      rc = zx_batch_group(Z, g.g0, g.g1);
      if (rc == ZADA_E_NOMEM || (rc == ZADA_E_TOO_LARGE && Z.ex)) {   // no room for the batch's tables: one by one
        stop(rc);
        Z.A = keep; rc = 0; c->timing.clear();
        for (int i = g.g0; i < g.g1 && !rc; i++) { rc = zx_single(Z, i); gather(); }
      }
    }
    gather();
    if (rc) return stop(rc == ZADA_E_HIP_ ? ZADA_E_HIP : rc);
  }
  // the central directory and the end records: one copy
  const uint64_t at = Z.A.pos;
  std::vector<uint8_t> tail;
  zw_finish(Z.A, tail);
  if (Z.A.pos > Z.cap) return stop(zx_too_small(Z));
  hipMemcpyAsync(Z.archive + at, tail.data(), tail.size(), hipMemcpyHostToDevice, c->stream);
  if (hip_check(c, hipStreamSynchronize(c->stream), "zip directory")) return ZADA_E_HIP;
  c->timing = times;
  *archive_len = Z.A.pos;
  return ZADA_OK;
}

// the checks both entry points make before anything touches the device, with their texts under the entry point's name; then the writer's state
static int zx_open(zada_ctx *z, ZxCall &Z, bool ex, int method, int count, const zada_zip_entry *ent, void *d_archive, uint64_t cap, uint64_t archive_base,
                   const zada_zip_crypt *crypt, uint64_t *archive_len, zada_zip_result *res) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = c->lz_run_stopped = false;                       // (as every entry point: zada_lzma_export_state)
  const char *who = ex ? "zada_zip_device_ex" : "zada_zip_device";
  char buf[320];
  if (!(ex ? zw_method_ok_ex(method, c->knob_zip_legacy) : zw_method_ok(method))) {
    snprintf(buf, sizeof buf, "%s: method %d (%s) is not one it takes: Store (0), %s", who, method, zw_method_name(method),
             !ex ? "Deflate_Fixed .. Deflate_R (6 .. 11)" : c->knob_zip_legacy ? "Shrink_1 .. Preselection_2 (1 .. 35)" : "Deflate_Fixed .. Preselection_2 (6 .. 35)");
    c->err = buf;
    return ZADA_E_INVALID;
  }
  if (!archive_len || (count && (!ent || !res))) { c->err = std::string(who) + ": null argument"; return ZADA_E_INVALID; }
  if (!d_archive) { c->err = std::string(who) + ": null archive buffer"; return ZADA_E_INVALID; }
  if (crypt && ((count && !crypt->random11) || (crypt->pw_len && !crypt->password))) {
    c->err = std::string(who) + ": a password needs random11 (eleven bytes per entry) and, with pw_len > 0, its bytes";
    return ZADA_E_INVALID;
  }
  if (count == 0 && archive_base > ZW_M32) {             // (Finish promotes an archive to Zip64 only when it has entries)
    c->err = std::string(who) + ": an empty archive behind more than 4 GiB - 1 bytes has no end record";
    return ZADA_E_INVALID;
  }
  int bad = -1, why = 0;
  const int rc = zw_check_ex(ent, count, (uint64_t)(uintptr_t)d_archive, cap, crypt != nullptr, &bad, &why);
  if (rc) {
    snprintf(buf, sizeof buf, "%s: entry %d: %s", who, bad, zw_why_text(why));
    c->err = buf;
    return rc;
  }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  if (!c->zw) c->zw = new (std::nothrow) ZwState();
  if (!c->zw) { c->err = "zip: no memory for the tables"; return ZADA_E_NOMEM; }
  Z.who = who; Z.ex = ex; Z.z = z; Z.c = c; Z.S = (ZwState *)c->zw; Z.ent = ent; Z.res = res; Z.archive = (uint8_t *)d_archive; Z.cap = cap;
  Z.A.base = archive_base;
  Z.m.assign((size_t)count, method);
  return 1;                                              // (go on)
}

uint64_t zada_zip_bound(int count, const zada_zip_entry *ent, uint64_t archive_base) { return zw_bound(count < 0 || !ent ? 0 : count, ent, archive_base); }

int zada_zip_device(zada_ctx *z, int method, int count, const zada_zip_entry *ent, void *d_archive, uint64_t cap, uint64_t archive_base,
                    uint64_t *archive_len, zada_zip_result *res) {
  ZxCall Z;
  const int rc = zx_open(z, Z, false, method, count, ent, d_archive, cap, archive_base, nullptr, archive_len, res);
  if (rc != 1) return rc;
  std::vector<ZwGroup> groups;
  zw_groups(ent, count, method, (uint64_t)Z.c->knob_batch_mib << 20, groups);
  return zx_run(Z, groups, archive_len);
}

uint64_t zada_zip_bound_ex(int count, const zada_zip_entry *ent, uint64_t archive_base, int encrypted) {
  return zw_bound_ex(count < 0 || !ent ? 0 : count, ent, archive_base, encrypted != 0);
}

int zada_zip_device_ex(zada_ctx *z, int method, int count, const zada_zip_entry *ent, void *d_archive, uint64_t cap, uint64_t archive_base,
                       const zada_zip_crypt *crypt, uint64_t *archive_len, zada_zip_result *res) {
  ZxCall Z;
  const int rc = zx_open(z, Z, true, method, count, ent, d_archive, cap, archive_base, crypt, archive_len, res);
  if (rc != 1) return rc;
  Ctx *c = Z.c;
  if (crypt) { Z.enc = true; Z.random11 = crypt->random11; zada_crypt_init_keys(crypt->password, crypt->pw_len, Z.k0); }
  // the method of every entry: Preselection looks at the name (the bytes of the table, copied: they are not NUL-terminated there) and the size
  std::vector<uint64_t> lit((size_t)count, 0);
  for (int i = 0; i < count; i++) {
    if (method >= ZADA_PRESELECTION_1) {
      const std::string nm(ent[i].name_len ? (const char *)ent[i].name : "", ent[i].name_len);
      Z.m[i] = zada_preselect(method, zada_guess_type_from_name(nm.c_str()), 1, ent[i].n);
    }
    lit[i] = zada_lzma_lit_table_bytes(Z.m[i]);
  }
  std::vector<ZwGroup> groups;
  if (method == 0) zw_groups(ent, count, 0, 0, groups);
  else if (zw_is_legacy(method)) {
    const int big = zw_legacy_too_large(ent, count);
    if (big >= 0) {
      char buf[160];
      snprintf(buf, sizeof buf, "zada_zip_device_ex: entry %d: Shrink and Reduce take entries below 1 GiB - 64 KiB", big);
      c->err = buf;
      return ZADA_E_TOO_LARGE;
    }
    zw_groups_legacy(ent, count, method, (uint64_t)c->knob_batch_mib << 20, (uint64_t)c->knob_reduce_group_mib << 20, groups);
  } else {
    const uint64_t mib = (uint64_t)c->knob_batch_mib << 20, limit = mib < (1ull << 30) ? mib : 1ull << 30;
    zw_groups_ex(ent, count, Z.m.data(), lit.data(), limit, (uint64_t)c->knob_bz_batch_mib << 20, (uint64_t)c->knob_lzma_lit_mib << 20, groups);
  }
  return zx_run(Z, groups, archive_len);
}
