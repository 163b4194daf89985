// zada_find.hip -- Find_Zip on the device (tools/find_zip.adb): zada_find_device, a string searched in one device buffer, and
// zada_findzip_device, the same in every entry of an archive that lies in device memory.  The host side is a plan (zada_find_plan.h: the string, the
// argument checks, the groups) around zada_unzip_device, whose launches extract a group into an arena of the context; what is new here:
// k_fz_search: one wave per piece of 16 KiB of an entry, four pieces per workgroup.  The piece's end positions are the bytes of the piece; the wave
//   walks the aligned 16-byte words that hold them, 64 words a strip, four strips between two looks at the candidates.  A lane loads its word (bytes
//   in front of the entry's first byte become spaces), takes the two dwords in front of it from its neighbour (lane 0: from lane 63 of the strip
//   before; for the piece's first strip one more aligned load, from the piece before where the entry has one -- a word in front of the entry is
//   spaces and is not loaded) and keeps the bytes that can be the string's last character and whose eight-byte window, upper-cased in registers, is
//   the string's last eight (fz_filter16).  A string of up to eight bytes is found by that alone.  A longer one is confirmed wave-wide, candidate
//   after candidate: lane L compares the string's bytes [stl - 16 (L + 1), stl - 16 L) -- word 63 - L of the 1024-byte buffer the workgroup staged in
//   LDS -- with the text in front of the candidate, two aligned loads funnelled into one (fz_lane_text), and __all decides.  The wave sums its hits
//   and lane 0 sends one 64-bit atomic add and one atomic minimum per piece that found any.  Nothing is stored to the text.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <new>
#include <string>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_find_plan.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {

constexpr uint32_t FZ_WAVE = 64, FZ_NONE = 0xFFFFFFFFu;
constexpr uint32_t FZ_UNROLL = 4;                      // strips of 64 words whose loads are issued before the first filter
typedef uint32_t fz_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const fz_u32x4 fz_gcu4;

struct FzEntry { uint64_t base, n; };                  // device address and length of an entry's decoded bytes

struct FzLoad {
  __device__ __forceinline__ void operator()(uint64_t a, uint32_t w[4]) const {
    const fz_u32x4 v = *(fz_gcu4 *)a;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  }
};

// pieces = nullptr: one entry, piece k at k << FZ_PIECE_LOG.  occ [entry] is 0 and first [entry] the entry's length when the kernel starts.
__global__ void __launch_bounds__(FZ_WAVE * FZ_WAVES) k_fz_search(const FzEntry *__restrict__ ents, const UzPiece *__restrict__ pieces, uint64_t npieces,
                                                                  const uint32_t *__restrict__ needle, const FzPat P, unsigned long long *occ,
                                                                  unsigned long long *first) {
  const uint32_t stl = P.len, fold = P.fold;
  __shared__ fz_u32x4 s_str[FZ_MAX / 16];
  if (stl > 8u) {                                          // (the same in every thread of the grid)
    ((uint32_t *)s_str)[threadIdx.x] = needle[threadIdx.x];
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & (FZ_WAVE - 1);
  const uint64_t pi = (uint64_t)blockIdx.x * FZ_WAVES + (threadIdx.x >> 6);
  if (pi >= npieces) return;
  uint64_t off;
  uint32_t entry, len;
  if (pieces) { const UzPiece P = pieces[pi]; off = P.off; entry = P.entry; len = P.len; }
  else {
    entry = 0; off = pi << FZ_PIECE_LOG;
    const uint64_t rest = ents[0].n - off;
    len = (uint32_t)(rest < FZ_PIECE ? rest : FZ_PIECE);
  }
  const FzEntry E = ents[entry];
  const uint64_t base = E.base, end = base + E.n, a0 = base + off, a1 = a0 + len;
  const uint64_t k0 = a0 >> 4, k1 = (a1 - 1) >> 4;         // the words that hold the piece's bytes (len > 0)
  const FzLoad ld{};
  uint32_t cnt = 0, mn = FZ_NONE;                          // this lane's hits (stl <= 8) and the smallest offset in the piece among them
  uint32_t ucnt = 0, umn = FZ_NONE;                        // the wave's confirmed hits (the same in every lane)
  uint32_t carry2, carry;                                  // the two dwords in front of the strip to come (the same in every lane): first the piece before's last
  {
    uint32_t p[4];
    fz_word(ld, k0 - 1, base, end, 0, p);
    carry2 = p[2]; carry = p[3];
  }
  for (uint64_t kb = k0; kb <= k1; kb += FZ_WAVE * FZ_UNROLL) {
    uint32_t w[FZ_UNROLL][4], m[FZ_UNROLL];
    // every load of the group is issued before the first filter; a lane behind the piece's last word loads that word again (its bits do not count)
#pragma unroll
    for (uint32_t u = 0; u < FZ_UNROLL; u++) {
      const uint64_t k = kb + u * FZ_WAVE + lane;
      ld((k < k1 ? k : k1) << 4, w[u]);
    }
    if (kb == k0 && lane == 0 && (k0 << 4) < base) fz_spaces_front(w[0], (uint32_t)(base - (k0 << 4)));
#pragma unroll
    for (uint32_t u = 0; u < FZ_UNROLL; u++) {
      const uint64_t k = kb + u * FZ_WAVE + lane;
      const uint32_t up2 = (uint32_t)__shfl_up((int)w[u][2], 1, FZ_WAVE), up = (uint32_t)__shfl_up((int)w[u][3], 1, FZ_WAVE);
      const uint32_t prev2 = lane ? up2 : carry2, prev = lane ? up : carry;
      carry2 = (uint32_t)__shfl((int)w[u][2], 63, FZ_WAVE); carry = (uint32_t)__shfl((int)w[u][3], 63, FZ_WAVE);
      m[u] = k <= k1 ? fz_filter16(w[u], prev2, prev, P) & fz_range_mask(k << 4, a0, a1) : 0u;
    }
    if (stl <= 8u) {
#pragma unroll
      for (uint32_t u = 0; u < FZ_UNROLL; u++)
        if (m[u]) {
          const uint32_t at = (uint32_t)(((kb + u * FZ_WAVE + lane) << 4) + (uint32_t)__builtin_ctz(m[u]) - a0);
          cnt += (uint32_t)__builtin_popcount(m[u]);
          mn = at < mn ? at : mn;
        }
      continue;
    }
    // the survivors, one after the other, by the whole wave
#pragma unroll
    for (uint32_t u = 0; u < FZ_UNROLL; u++) {
      for (uint64_t bal = __ballot(m[u] != 0u); bal; bal &= bal - 1) {
        const uint32_t src = (uint32_t)__builtin_ctzll(bal);
        const uint64_t kk = kb + u * FZ_WAVE + src;
        for (uint32_t mm = (uint32_t)__shfl((int)m[u], (int)src, FZ_WAVE); mm; mm &= mm - 1) {
          const uint64_t e = (kk << 4) + (uint32_t)__builtin_ctz(mm);
          const uint32_t nv = fz_lane_bytes(stl, lane);
          bool ok = true;
          if (nv) {
            uint32_t t[4];
            fz_lane_text(ld, e, lane, base, end, fold, t);
            const fz_u32x4 sv = s_str[63u - lane];
            const uint32_t s[4] = {sv.x, sv.y, sv.z, sv.w};
            ok = fz_same_tail(t, s, nv);
          }
          if (__all(ok)) {
            const uint32_t at = (uint32_t)(e - a0);
            ucnt++;
            umn = at < umn ? at : umn;
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 1; j < (int)FZ_WAVE; j <<= 1) {
    cnt += (uint32_t)__shfl_xor((int)cnt, j, FZ_WAVE);
    const uint32_t o = (uint32_t)__shfl_xor((int)mn, j, FZ_WAVE);
    mn = o < mn ? o : mn;
  }
  cnt += ucnt;
  mn = umn < mn ? umn : mn;
  if (lane == 0 && cnt) {
    atomicAdd(&occ[entry], (unsigned long long)cnt);
    atomicMin(&first[entry], (unsigned long long)(off + mn));
  }
}

// ---- host side ----
struct FzState { DevBuf tabs, arena; };

static FzState *fz_state(Ctx *c) {
  if (!c->fz) c->fz = new (std::nothrow) FzState();
  return (FzState *)c->fz;
}
void find_destroy(Ctx *c) {
  FzState *S = (FzState *)c->fz;
  if (!S) return;
  for (DevBuf *b : {&S->tabs, &S->arena}) dev_free(*b);
  delete S;
  c->fz = nullptr;
}

#define FZ_HIP(call, what) do { if (hip_check(c, (call), what)) return ZADA_E_HIP_; } while (0)

// entries [0 .. ne) through one launch of k_fz_search: over `pieces`, or (pieces empty, ne = 1) over the pieces of the one entry.  occ [k] and
// first [k] as zada_find_device gives them.  Synchronises.
static int fz_run(Ctx *c, FzState *S, const std::vector<FzEntry> &ents, const std::vector<UzPiece> &pieces, const FzNeedle &N, std::vector<uint64_t> &occ,
                  std::vector<uint64_t> &first, const char *mark) {
  hipStream_t st = c->stream;
  const uint32_t ne = (uint32_t)ents.size();
  const uint64_t NP = pieces.empty() ? fz_piece_count(ents[0].n) : pieces.size();
  occ.assign(ne, 0);
  first.resize(ne);
  for (uint32_t k = 0; k < ne; k++) first[k] = ents[k].n;
  if (!NP) return 0;
  const uint64_t o_needle = 0, o_ents = FZ_MAX, o_occ = (o_ents + (uint64_t)ne * sizeof(FzEntry) + 255) & ~255ull, o_first = (o_occ + (uint64_t)ne * 8 + 255) & ~255ull,
                 o_pieces = (o_first + (uint64_t)ne * 8 + 255) & ~255ull;
  const int rc = dev_grow(c, S->tabs, o_pieces + pieces.size() * sizeof(UzPiece) + 256, "hipMalloc (find tables)");
  if (rc) return rc;
  uint8_t *T = S->tabs.p;
  hipMemcpyAsync(T + o_needle, N.buf, FZ_MAX, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(T + o_ents, ents.data(), (size_t)ne * sizeof(FzEntry), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(T + o_occ, occ.data(), (size_t)ne * 8, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(T + o_first, first.data(), (size_t)ne * 8, hipMemcpyHostToDevice, st);
  if (!pieces.empty()) hipMemcpyAsync(T + o_pieces, pieces.data(), pieces.size() * sizeof(UzPiece), hipMemcpyHostToDevice, st);
  hipLaunchKernelGGL(k_fz_search, dim3((uint32_t)((NP + FZ_WAVES - 1) / FZ_WAVES)), dim3(FZ_WAVE * FZ_WAVES), 0, st, (const FzEntry *)(T + o_ents),
                     pieces.empty() ? (const UzPiece *)nullptr : (const UzPiece *)(T + o_pieces), NP, (const uint32_t *)(T + o_needle), N.p,
                     (unsigned long long *)(T + o_occ), (unsigned long long *)(T + o_first));
  c->tmark(mark);
  hipMemcpyAsync(occ.data(), T + o_occ, (size_t)ne * 8, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(first.data(), T + o_first, (size_t)ne * 8, hipMemcpyDeviceToHost, st);
  FZ_HIP(hipGetLastError(), "find launch");
  FZ_HIP(hipStreamSynchronize(st), "find");
  return 0;
}

// the string of a call: its length checked, upper-cased when asked
static int fz_text(Ctx *c, const char *who, const uint8_t *text, uint32_t text_len, uint32_t flags, FzNeedle &N) {
  if (fz_check_len(text_len) != ZADA_OK) {
    char buf[160];
    snprintf(buf, sizeof buf, "%s: a search string of %u bytes (1 .. %u are taken, as find_zip does)", who, text_len, FZ_MAX);
    c->err = buf;
    return ZADA_E_INVALID;
  }
  if (!text) { c->err = std::string(who) + ": null argument"; return ZADA_E_INVALID; }
  return fz_needle(text, text_len, flags, N);
}

}  // namespace zada

using namespace zada;

int zada_find_device(zada_ctx *z, const void *d_buf, uint64_t n, const uint8_t *text, uint32_t text_len, uint32_t flags, uint64_t *occurrences, uint64_t *first) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;                                            // (as every entry point: zada_lzma_export_state)
  if (!occurrences || !first || (n && !d_buf)) { c->err = "zada_find_device: null argument"; return ZADA_E_INVALID; }
  FzNeedle N;
  int rc = fz_text(c, "zada_find_device", text, text_len, flags, N);
  if (rc) return rc;
  if (n >= UZ_MAX_BYTES) { c->err = "zada_find_device: a buffer of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  *occurrences = 0; *first = 0;
  if (n == 0) { hipStreamSynchronize(c->stream); return ZADA_OK; }
  FzState *S = fz_state(c);
  if (!S) { c->err = "find: no memory for the tables"; return ZADA_E_NOMEM; }
  std::vector<FzEntry> ents(1, FzEntry{(uint64_t)(uintptr_t)d_buf, n});
  std::vector<UzPiece> none;
  std::vector<uint64_t> occ, fst;
  c->tbegin();
  c->tmark("find:begin");
  rc = fz_run(c, S, ents, none, N, occ, fst, "find:k_fz_search");
  c->tend();
  if (rc) { hipStreamSynchronize(c->stream); (void)hipGetLastError(); return rc == ZADA_E_HIP_ ? ZADA_E_HIP : rc; }
  *occurrences = occ[0]; *first = fst[0];
  return ZADA_OK;
}

int zada_findzip_device(zada_ctx *z, const void *d_archive, uint64_t archive_len, int count, const zada_unzip_entry *ent, const uint32_t keys0[3],
                        const uint8_t *text, uint32_t text_len, uint32_t flags, zada_findzip_result *res) {
  if (!z || count < 0) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = false;
  if (count && (!ent || !res)) { c->err = "zada_findzip_device: null argument"; return ZADA_E_INVALID; }
  if (archive_len && !d_archive) { c->err = "zada_findzip_device: null archive"; return ZADA_E_INVALID; }
  FzNeedle N;
  int rc = fz_text(c, "zada_findzip_device", text, text_len, flags, N);
  if (rc) return rc;
  int bad = -1, why = 0;
  rc = fz_check(ent, count, archive_len, keys0 != nullptr, &bad, &why, c->knob_unzip_legacy);
  if (rc) {
    char buf[200];
    snprintf(buf, sizeof buf, "zada_findzip_device: entry %d: %s", bad, uz_why_text(why, c->knob_unzip_legacy));
    c->err = buf;
    return rc;
  }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  if (count == 0) { hipStreamSynchronize(c->stream); return ZADA_OK; }
  FzState *S = fz_state(c);
  if (!S) { c->err = "findzip: no memory for the tables"; return ZADA_E_NOMEM; }
  std::vector<std::pair<const char *, float>> times;               // last_timing: the launches of every group of the call, equal names added up
  auto gather = [&]() {
    for (const auto &t : c->timing) {
      size_t k = 0;
      while (k < times.size() && strcmp(times[k].first, t.first)) k++;
      if (k < times.size()) times[k].second += t.second; else times.push_back(t);
    }
    c->timing.clear();
  };
  std::vector<zada_unzip_entry> rows(ent, ent + count);
  for (zada_unzip_entry &e : rows) e.flags &= e.method == 6 ? 7u : 3u;   // (an Implode row keeps its general-purpose bit 2)
  std::vector<int> ends;
  fz_groups(rows.data(), count, (uint64_t)c->knob_batch_mib << 20, ends);
  std::vector<zada_unzip_result> ur;
  std::vector<FzEntry> ents;
  std::vector<uint64_t> plen, occ, fst, pfirst;
  std::vector<uint32_t> pid, pk;
  std::vector<UzPiece> pieces;
  int g0 = 0;
  for (int g1 : ends) {
    const int n = g1 - g0;
    uint64_t bytes = 0;
    for (int i = g0; i < g1; i++) { rows[i].out_off = bytes; bytes += uz_slot(rows[i].cap); }
    rc = dev_grow(c, S->arena, bytes + 16, "hipMalloc (findzip arena)");
    if (rc) return rc;
    ur.assign(n, zada_unzip_result{0, 0xFFFFFFFFu, 0, 0});
    // through the reader's launches; a return value that no entry carries is what stopped the call
    rc = zada_unzip_device(z, d_archive, archive_len, S->arena.p, bytes, n, rows.data() + g0, keys0, ur.data());
    gather();
    bool entrys = false;
    for (int k = 0; k < n && rc; k++) entrys = entrys || ur[k].rc == rc;
    if (rc && !entrys) return rc;
    ents.clear(); plen.clear(); pid.clear(); pk.clear();
    for (int k = 0; k < n; k++) {
      res[g0 + k] = zada_findzip_result{ur[k].rc, ur[k].crc, ur[k].out_len, 0, 0};
      if (ur[k].rc) continue;
      pid.push_back((uint32_t)ents.size()); pk.push_back((uint32_t)k); plen.push_back(ur[k].out_len);
      ents.push_back(FzEntry{(uint64_t)(uintptr_t)S->arena.p + rows[g0 + k].out_off, ur[k].out_len});
    }
    g0 = g1;
    if (ents.empty()) continue;
    uz_pieces(plen.data(), pid.data(), (uint32_t)ents.size(), FZ_PIECE_LOG, pieces, pfirst);
    if (pieces.empty()) continue;                                    // (every entry of the group is empty: nothing occurs in it, first = its length, 0)
    c->tbegin();
    c->tmark("findzip:begin");
    rc = fz_run(c, S, ents, pieces, N, occ, fst, "findzip:k_fz_search");
    c->tend();
    gather();
    if (rc) { hipStreamSynchronize(c->stream); (void)hipGetLastError(); return rc == ZADA_E_HIP_ ? ZADA_E_HIP : rc; }
    for (size_t p = 0; p < ents.size(); p++) {
      zada_findzip_result &R = res[g1 - n + pk[p]];
      R.occurrences = occ[p]; R.first = fst[p];
    }
  }
  hipStreamSynchronize(c->stream);
  c->timing = times;
  return ZADA_OK;
}
