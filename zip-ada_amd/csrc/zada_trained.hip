// zada_trained.hip -- Trained_Compression (trained/trained_compression.ads, .adb) for batches of messages in device memory: every message is the
// tail of one LZMA stream (Level_3, lc 3, lp 0, pb 2, dictionary_size 2 ** 19, 5-byte header, no size field) whose head is training data both sides
// know.  The contract is at the block of include/zada.h, the argument at DESIGN.md 21.
//
// The decoding side.  zada_trained_open_decoder decodes stub [0 .. skip) ONCE, on the device, with the one-wave decoder of zada_unlzma.hip told to
// stop at the first symbol boundary from which fewer than 64 stub bytes remain (k_unlzma_trained <true>; ulz_decode_f, zada_unlzma_logic.h): the
// handle keeps the snapshot it leaves (range, code, state, reps, positions, the probability model), the dec_fork_out bytes of the trainer's text
// decoded so far, and the at most 64 stub bytes behind the snapshot.  zada_trained_decode_device then runs one wave per entry from that snapshot
// (k_unlzma_trained <false>):
//   k_tr_gather   per entry: the input slot = stub [dec_fork_in .. skip) & message, the head of the output slot = the trainer's text so far.  The
//                 window stays "the output slot", so the match copies need no second address space; a slot is t_len + cap bytes;
//   the decoder   writes the slot from dec_fork_out on, bounded by t_len + cap;
//   k_tr_gather   again: the slot's bytes from t_len on go to the caller's buffer.
// With skip < 10 the five header bytes and the range coder's five initial bytes do not lie inside the stub's part: there is no symbol boundary to
// stop at, and every entry decodes stub [0 .. skip) & message from its own header (info.unforked).
//
// The encoding side.  zada_trained_open_encoder codes the trainer alone ONCE, as one LZMA_3 stream stopped TR_FORK_MARGIN positions in front of its
// end (lzma_fork_snapshot: the resumable launch of zada_lzma.hip), and keeps the coder's state of that stop and the stream bytes written so far.
// zada_trained_encode_device lays trainer & data_i into the slots of an LZMA batch (k_tr_gather), runs the BT4 producer over them as for any batch
// (the dictionary fixed at 2 ** 19 in place of the entry's size), fills every entry's save slot from the snapshot (k_lzma_fork_fill: the window's
// bookkeeping is this entry's) and lets k_lzma_encode resume: it codes [fork_pos, t_len + n_i) and the marker.  The Zip prefix and the first `skip`
// bytes are dropped on the way out.  An entry whose stream is longer than one window fill (String_buffer_size = 2 ** 20 bytes) runs unforked in the
// same launch, as every entry does when the trainer is shorter than twice the margin.  The producer still inserts the trainer's positions for every
// entry: sharing its trees is out of scope.
//
// k_tr_gather is a plain streaming kernel: one workgroup per entry, 16-byte loads and stores where source and destination are congruent mod 16,
// bytes otherwise and at both ends.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <new>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_unlzma_logic.h"

struct zada_ctx { zada::Ctx c; };

struct zada_trained {
  zada_ctx *z = nullptr;
  int device = 0;
  int kind = 0;                                     // 1: the encoding side, 2: the decoding side
  uint64_t t_len = 0, skip = 0;
  uint8_t *d_trainer = nullptr;                     // encoder: the trainer
  uint8_t *d_fsnap = nullptr, *d_fout = nullptr;    // encoder: the coder's state at the fork (one LzSave slot) and the stream bytes written there (null: no fork)
  uint64_t fout_len = 0;                            // ... their number, the four bytes of the Zip prefix included
  uint8_t *d_snap = nullptr;                        // decoder: the snapshot (null: none, every entry decodes its whole stream)
  uint8_t *d_text = nullptr;                        // decoder: the trainer's text up to the snapshot
  uint8_t *d_prefix = nullptr; uint64_t prefix_len = 0;   // decoder: stub [dec_fork_in .. skip)
  uint8_t *d_stub = nullptr;                        // decoder: stub [0 .. skip), for entries that decode their whole stream
  zada::DevBuf tabs, arena;
  zada_trained_info_t info{};
};

namespace zada {

constexpr uint32_t TR_DICT = 1u << 19;              // TC_dictionary_size
constexpr uint64_t TR_MAX_BYTES = 1ull << 40;
constexpr uint32_t TR_THREADS = 256;
// How far in front of the trainer's end its stream is stopped: keepSizeAfter = BT4_OPTS + BT4_LOOK (zada_bt4.h), the most a window keeps behind its
// read position.  What the coder and the matcher have looked at when they stop lies below fork_pos + 3 * 273: far inside the trainer.
constexpr uint64_t TR_FORK_MARGIN = 4096 + 273;

struct TrCopy { uint64_t src, dst, n; };
struct TrGather { TrCopy c[3]; };

namespace {
__device__ __forceinline__ void tr_copy(uint8_t *dst, const uint8_t *src, uint64_t n) {       // all threads of the workgroup
  const uint32_t t = threadIdx.x;
  if (((((uintptr_t)dst) ^ ((uintptr_t)src)) & 15u) == 0 && n >= 64) {
    const uint64_t head = (16u - (uint32_t)((uintptr_t)src & 15u)) & 15u;
    for (uint64_t i = t; i < head; i += TR_THREADS) dst[i] = src[i];
    const uint64_t body = (n - head) >> 4;
    const uint4 *s = (const uint4 *)(src + head);
    uint4 *d = (uint4 *)(dst + head);
    for (uint64_t i = t; i < body; i += TR_THREADS) d[i] = s[i];
    for (uint64_t i = head + (body << 4) + t; i < n; i += TR_THREADS) dst[i] = src[i];
  } else {
    for (uint64_t i = t; i < n; i += TR_THREADS) dst[i] = src[i];
  }
}
__global__ void __launch_bounds__(TR_THREADS) k_tr_gather(const TrGather *__restrict__ g) {
  const TrGather G = g[blockIdx.x];
#pragma unroll
  for (int k = 0; k < 3; k++) if (G.c[k].n) tr_copy((uint8_t *)G.c[k].dst, (const uint8_t *)G.c[k].src, G.c[k].n);
}
}  // namespace

static int tr_gather(Ctx *c, const std::vector<TrGather> &g, uint8_t *d_list) {
  if (g.empty()) return 0;
  hipMemcpyAsync(d_list, g.data(), g.size() * sizeof(TrGather), hipMemcpyHostToDevice, c->stream);
  hipLaunchKernelGGL(k_tr_gather, dim3((uint32_t)g.size()), dim3(TR_THREADS), 0, c->stream, (const TrGather *)d_list);
  return hip_check(c, hipGetLastError(), "k_tr_gather") ? ZADA_E_HIP : 0;
}
static void tr_free(zada_trained *h) {
  for (uint8_t *p : {h->d_trainer, h->d_fsnap, h->d_fout, h->d_stub, h->d_snap, h->d_text, h->d_prefix, h->tabs.p, h->arena.p}) if (p) hipFree(p);
  delete h;
}
// the checks every call on a handle makes before it touches the device
static int tr_check(zada_ctx *z, zada_trained *h, int kind, int count, const zada_trained_entry *ent, uint64_t *out_len, int *rc, const char *who) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = c->lz_run_stopped = false;                       // (as every entry point: zada_lzma_export_state)
  if (!h || h->z != z || h->kind != kind) { c->err = std::string(who) + ": not a handle of this context and this side"; return ZADA_E_INVALID; }
  if (count < 0 || (count && (!ent || !out_len || !rc))) { c->err = std::string(who) + ": null argument"; return ZADA_E_INVALID; }
  for (int i = 0; i < count; i++) {
    if ((ent[i].n && !ent[i].d_data) || (ent[i].cap && !ent[i].d_out)) { c->err = std::string(who) + ": null buffer"; return ZADA_E_INVALID; }
    if (ent[i].n >= TR_MAX_BYTES || ent[i].cap >= TR_MAX_BYTES) { c->err = std::string(who) + ": a buffer of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  }
  return 0;
}

// ---- the decoding side ----
static uint64_t a16(uint64_t v) { return (v + 15) & ~15ull; }

// entries g0 .. g1 - 1 of a call: gather, decode, deliver
static int tr_decode_group(Ctx *c, zada_trained *h, int g0, int g1, const zada_trained_entry *ent, uint64_t *out_len, int *rc_out, UlzResult *first_bad, int *first_bad_entry) {
  const uint32_t E = (uint32_t)(g1 - g0);
  const bool fork = h->d_snap && c->knob_trained_fork;
  const uint64_t T = h->t_len, F = fork ? h->info.dec_fork_out : 0, PL = fork ? h->prefix_len : h->skip;
  const uint8_t *d_head = fork ? h->d_prefix : h->d_stub;
  uint64_t in_bytes = 0, out_bytes = 0;
  for (int i = g0; i < g1; i++) { in_bytes += a16(PL + ent[i].n); out_bytes += a16(T + ent[i].cap); }
  int rc = dev_grow(c, h->arena, in_bytes + out_bytes + 16, "hipMalloc (trained arena)");
  if (rc) return rc;
  const uint64_t o_gather = 0, o_jobs = o_gather + (uint64_t)E * sizeof(TrGather), o_order = o_jobs + (uint64_t)E * sizeof(UlzTrainedJob),
                 o_res = (o_order + (uint64_t)E * 4 + 15) & ~15ull, total = o_res + (uint64_t)E * sizeof(UlzResult);
  rc = dev_grow(c, h->tabs, total, "hipMalloc (trained tables)");
  if (rc) return rc;
  std::vector<TrGather> g(E);
  std::vector<UlzTrainedJob> jobs(E);
  std::vector<uint32_t> order(E);
  uint64_t io = 0, oo = in_bytes;
  for (uint32_t k = 0; k < E; k++) {
    const zada_trained_entry &e = ent[g0 + (int)k];
    uint8_t *in_slot = h->arena.p + io, *out_slot = h->arena.p + oo;
    g[k].c[0] = TrCopy{(uint64_t)(uintptr_t)d_head, (uint64_t)(uintptr_t)in_slot, PL};
    g[k].c[1] = TrCopy{(uint64_t)(uintptr_t)e.d_data, (uint64_t)(uintptr_t)(in_slot + PL), e.n};
    g[k].c[2] = TrCopy{(uint64_t)(uintptr_t)h->d_text, (uint64_t)(uintptr_t)out_slot, F};
    jobs[k] = UlzTrainedJob{(uint64_t)(uintptr_t)in_slot, (uint64_t)(uintptr_t)out_slot, PL + e.n, T + e.cap};
    order[k] = k;
    io += a16(PL + e.n); oo += a16(T + e.cap);
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].n_in > jobs[b].n_in; });     // the longest first
  hipStream_t st = c->stream;
  uint8_t *tb = h->tabs.p;
  c->tmark("trained:begin");
  if ((rc = tr_gather(c, g, tb + o_gather))) return rc;
  c->tmark("trained:k_tr_gather");
  hipMemcpyAsync(tb + o_jobs, jobs.data(), (size_t)E * sizeof(UlzTrainedJob), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(tb + o_order, order.data(), (size_t)E * 4, hipMemcpyHostToDevice, st);
  if ((rc = unlzma_trained_launch(c, (const UlzTrainedJob *)(tb + o_jobs), (const uint32_t *)(tb + o_order), E, (UlzResult *)(tb + o_res), fork ? h->d_snap : nullptr, nullptr, 0))) return rc;
  c->tmark("trained:k_unlzma_trained");
  std::vector<UlzResult> res(E);
  hipMemcpyAsync(res.data(), tb + o_res, (size_t)E * sizeof(UlzResult), hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipStreamSynchronize(st), "trained decode")) return ZADA_E_HIP;
  std::vector<TrGather> d;
  for (uint32_t k = 0; k < E; k++) {
    const int i = g0 + (int)k;
    if (res[k].rc) {
      rc_out[i] = ZADA_E_DATA; out_len[i] = 0;
      if (*first_bad_entry < 0) { *first_bad_entry = i; *first_bad = res[k]; first_bad->in_pos = res[k].in_pos > PL ? res[k].in_pos - PL : 0; }
      continue;
    }
    rc_out[i] = ZADA_OK;
    uint64_t n = res[k].out_len > T ? res[k].out_len - T : 0;      // (a stream that ends inside the trainer's text: no data, as Write_Byte discards)
    if (n > ent[i].cap) n = ent[i].cap;                            // (never: the decoder is bounded by t_len + cap)
    out_len[i] = n;
    if (n) { TrGather x{}; x.c[0] = TrCopy{jobs[k].out + T, (uint64_t)(uintptr_t)ent[i].d_out, n}; d.push_back(x); }
  }
  if ((rc = tr_gather(c, d, tb + o_gather))) return rc;
  c->tmark("trained:deliver");
  if (hip_check(c, hipStreamSynchronize(st), "trained deliver")) return ZADA_E_HIP;
  return 0;
}

// ---- the encoding side ----
static int tr_encode_group(Ctx *c, zada_trained *h, const std::vector<int> &group, const zada_trained_entry *ent, uint64_t *out_len, int *rc_out, bool *small, bool *refused) {
  const uint32_t E = (uint32_t)group.size();
  const uint64_t T = h->t_len, drop = 4 + h->skip;                // (the four bytes Zip.Compress.LZMA_E puts in front, then Skip_Compressed)
  std::vector<uint64_t> ln(E);
  for (uint32_t k = 0; k < E; k++) ln[k] = T + ent[group[k]].n;
  DevBatch D;
  int rc = lzma_batch_layout(c, ZADA_LZMA_3, E, ln.data(), nullptr, D);
  if (rc) return rc;
  const uint64_t o_forked = (uint64_t)E * sizeof(TrGather);
  rc = dev_grow(c, h->tabs, o_forked + E, "hipMalloc (trained tables)");
  if (rc) return rc;
  // an entry forks when ONE window fill holds its whole stream (String_buffer_size bytes at most): then the window's bookkeeping at the fork is
  // a function of the stream's length alone (k_lzma_fork_fill)
  const uint64_t one_fill = lzma_string_buffer_size(3, TR_DICT);
  std::vector<uint8_t> forked(E, 0);
  std::vector<TrGather> g(E);
  for (uint32_t k = 0; k < E; k++) {
    const zada_trained_entry &e = ent[group[k]];
    forked[k] = h->d_fsnap && c->knob_trained_fork && ln[k] <= one_fill ? 1 : 0;
    (forked[k] ? h->info.forked : h->info.unforked)++;
    uint8_t *slot = D.d_in + D.start[k];
    g[k].c[0] = TrCopy{(uint64_t)(uintptr_t)h->d_trainer, (uint64_t)(uintptr_t)slot, T};
    g[k].c[1] = TrCopy{(uint64_t)(uintptr_t)e.d_data, (uint64_t)(uintptr_t)(slot + T), e.n};
    g[k].c[2] = TrCopy{0, 0, 0};
  }
  c->tbegin(); c->tmark("lzma:begin");
  if ((rc = tr_gather(c, g, h->tabs.p))) return rc;
  const LzFork fk{h->d_fsnap, h->d_fout, h->fout_len, h->tabs.p + o_forked};
  if (h->d_fsnap && c->knob_trained_fork) {
    hipMemcpyAsync(h->tabs.p + o_forked, forked.data(), E, hipMemcpyHostToDevice, c->stream);
    D.fork = &fk;
  }
  const int dict0 = c->knob_lzma_dict;
  c->knob_lzma_dict = (int)TR_DICT;                                // (dictionary_size => TC_dictionary_size, not the entry's size)
  rc = lzma_batch_launch(c, ZADA_LZMA_3, D);
  c->knob_lzma_dict = dict0;
  if (rc) return rc;
  std::vector<TrGather> d;
  for (uint32_t k = 0; k < E; k++) {
    const int i = group[k];
    if (D.refused[k]) { rc_out[i] = ZADA_E_REFERENCE; out_len[i] = 0; *refused = true; continue; }
    if (D.bytes[k] > D.cap[k]) { c->err = "trained encode: a stream longer than its slot"; return ZADA_E_INVALID; }
    const uint64_t n = D.bytes[k] > drop ? D.bytes[k] - drop : 0;
    out_len[i] = n;
    rc_out[i] = n > ent[i].cap ? ZADA_E_INVALID : ZADA_OK;
    if (rc_out[i]) *small = true;
    const uint64_t w = n < ent[i].cap ? n : ent[i].cap;
    if (w) { TrGather x{}; x.c[0] = TrCopy{(uint64_t)(uintptr_t)(D.d_out + D.off[k] + drop), (uint64_t)(uintptr_t)ent[i].d_out, w}; d.push_back(x); }
  }
  if ((rc = tr_gather(c, d, h->tabs.p))) return rc;
  if (hip_check(c, hipStreamSynchronize(c->stream), "trained encode out")) return ZADA_E_HIP;
  c->tmark("lzma:end"); c->tend();
  if (*refused) lzma_batch_refused(c, D);                          // (the error text)
  return 0;
}

}  // namespace zada

using namespace zada;

int zada_trained_stub(zada_ctx *z, const uint8_t *trainer, uint64_t t_len, uint8_t *out, uint64_t cap, uint64_t *out_len) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = c->lz_run_stopped = false;
  if ((t_len && !trainer) || (cap && !out) || !out_len) { c->err = "zada_trained_stub: null argument"; return ZADA_E_INVALID; }
  *out_len = 0;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  return lzma_plain_stream(c, trainer, t_len, out, cap, out_len, TR_DICT, false);
}

int zada_trained_open_encoder(zada_ctx *z, const void *trainer, uint64_t t_len, int on_device, uint64_t skip, zada_trained **hp) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = c->lz_run_stopped = false;
  if (!hp || (t_len && !trainer)) { c->err = "zada_trained_open_encoder: null argument"; return ZADA_E_INVALID; }
  *hp = nullptr;
  if (t_len >= (2ull << 30) - 65536 || skip >= TR_MAX_BYTES) { c->err = "zada_trained_open_encoder: a trainer of 2 GiB or more"; return ZADA_E_TOO_LARGE; }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  zada_trained *h = new (std::nothrow) zada_trained();
  if (!h) return ZADA_E_NOMEM;
  h->z = z; h->device = c->device; h->kind = 1; h->t_len = t_len; h->skip = skip;
  if (t_len) {
    if (hipMalloc((void **)&h->d_trainer, t_len) != hipSuccess) { (void)hipGetLastError(); tr_free(h); c->err = "hipMalloc (trainer)"; return ZADA_E_NOMEM; }
    hipMemcpyAsync(h->d_trainer, trainer, t_len, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream);
    if (hip_check(c, hipStreamSynchronize(c->stream), "trained: the trainer")) { tr_free(h); return ZADA_E_HIP; }
  }
  // The fork: the trainer alone as one stream, stopped at the first boundary of the coder's main loop at or beyond t_len - TR_FORK_MARGIN.
  // A trainer below twice the margin, or beyond one window fill, is not forked: every entry codes its whole stream.
  if (t_len >= 2 * TR_FORK_MARGIN && t_len <= lzma_string_buffer_size(3, TR_DICT)) {
    const uint64_t cap = t_len + t_len / 8 + 256;
    if (hipMalloc((void **)&h->d_fsnap, lzma_save_stride()) != hipSuccess || hipMalloc((void **)&h->d_fout, cap) != hipSuccess) {
      (void)hipGetLastError(); tr_free(h); c->err = "hipMalloc (trained fork)"; return ZADA_E_NOMEM;
    }
    c->lz_resume.clear();
    uint64_t pos = 0, olen = 0;
    const int rc = lzma_fork_snapshot(c, h->d_trainer, t_len, t_len - TR_FORK_MARGIN, TR_DICT, h->d_fout, cap, h->d_fsnap, &pos, &olen);
    if (rc) { hipStreamSynchronize(c->stream); hipStreamSynchronize(c->stream2); (void)hipGetLastError(); tr_free(h); return rc; }
    h->fout_len = olen;
    h->info.fork_pos = pos; h->info.fork_out = olen - 4;
  }
  *hp = h;
  return ZADA_OK;
}

int zada_trained_open_decoder(zada_ctx *z, const uint8_t *stub, uint64_t stub_len, uint64_t skip, uint64_t t_len, zada_trained **hp) {
  if (!z) return ZADA_E_INVALID;
  Ctx *c = &z->c;
  c->lz_stopped = c->lz_run_stopped = false;
  if (!hp || (stub_len && !stub)) { c->err = "zada_trained_open_decoder: null argument"; return ZADA_E_INVALID; }
  *hp = nullptr;
  if (skip > stub_len) { c->err = "zada_trained_open_decoder: skip beyond the stub"; return ZADA_E_INVALID; }
  if (stub_len >= TR_MAX_BYTES || t_len >= TR_MAX_BYTES) { c->err = "zada_trained_open_decoder: a stub or a trainer of 1 TiB or more"; return ZADA_E_TOO_LARGE; }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  zada_trained *h = new (std::nothrow) zada_trained();
  if (!h) return ZADA_E_NOMEM;
  h->z = z; h->device = c->device; h->kind = 2; h->t_len = t_len; h->skip = skip;
  hipStream_t st = c->stream;
  auto fail = [&](int rc) { hipStreamSynchronize(st); (void)hipGetLastError(); tr_free(h); return rc; };
  // the stub's part of every stream in device memory (16 spare bytes: an empty part still has an address)
  if (hipMalloc((void **)&h->d_stub, skip + 16) != hipSuccess || hipMalloc((void **)&h->d_prefix, ULZ_FORK_MARGIN + 16) != hipSuccess) {
    (void)hipGetLastError(); c->err = "hipMalloc (stub)"; return fail(ZADA_E_NOMEM);
  }
  if (skip) hipMemcpyAsync(h->d_stub, stub, skip, hipMemcpyHostToDevice, st);
  if (skip < 10) {                                                  // header and initial bytes reach into the message: no boundary to stop at
    if (hip_check(c, hipStreamSynchronize(st), "trained: the stub")) return fail(ZADA_E_HIP);
    *hp = h;
    return ZADA_OK;
  }
  const uint64_t snap_bytes = unlzma_snap_bytes();
  if (hipMalloc((void **)&h->d_snap, snap_bytes) != hipSuccess || hipMalloc((void **)&h->d_text, t_len + 16) != hipSuccess) {
    (void)hipGetLastError(); c->err = "hipMalloc (trained snapshot)"; return fail(ZADA_E_NOMEM);
  }
  int rc = dev_grow(c, h->tabs, sizeof(UlzTrainedJob) + 16 + sizeof(UlzResult), "hipMalloc (trained tables)");
  if (rc) return fail(rc);
  const UlzTrainedJob job{(uint64_t)(uintptr_t)h->d_stub, (uint64_t)(uintptr_t)h->d_text, skip, t_len};
  const uint32_t order0 = 0;
  const uint64_t o_order = sizeof(UlzTrainedJob), o_res = o_order + 16;
  hipMemsetAsync(h->d_snap, 0, snap_bytes, st);
  hipMemcpyAsync(h->tabs.p, &job, sizeof job, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(h->tabs.p + o_order, &order0, 4, hipMemcpyHostToDevice, st);
  rc = unlzma_trained_launch(c, (const UlzTrainedJob *)h->tabs.p, (const uint32_t *)(h->tabs.p + o_order), 1, (UlzResult *)(h->tabs.p + o_res), nullptr, h->d_snap, skip);
  if (rc) return fail(rc);
  UlzResult R;
  std::vector<uint8_t> snap(snap_bytes);
  hipMemcpyAsync(&R, h->tabs.p + o_res, sizeof R, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(snap.data(), h->d_snap, snap_bytes, hipMemcpyDeviceToHost, st);
  if (hip_check(c, hipStreamSynchronize(st), "trained: the stub")) return fail(ZADA_E_HIP);
  char buf[240];
  if (R.rc) {
    snprintf(buf, sizeof buf, "zada_trained_open_decoder: the stub: %s at input byte %llu", ulz_rule_name(R.rule), (unsigned long long)R.in_pos);
    c->err = buf;
    return fail(ZADA_E_DATA);
  }
  uint64_t fin = 0, fout = 0, lit = 0;
  if (R.end != ULZ_END_FORK || !unlzma_snap_info(snap.data(), &fin, &fout, &lit) || fin > skip || fout > t_len) {
    c->err = R.end == ULZ_END_MARKER ? "zada_trained_open_decoder: the stub ends on a marker inside its first skip bytes" : "zada_trained_open_decoder: the stub did not stop at a boundary";
    return fail(ZADA_E_DATA);
  }
  if (lit > ULZ_LIT_LDS_MAX) { c->err = "zada_trained_open_decoder: a stub with lc + lp > 3 is not Trained_Compression's"; return fail(ZADA_E_INVALID); }
  // from here on a forked stream's input is the stub from the snapshot on: fewer than 64 bytes
  if (skip - fin >= ULZ_FORK_MARGIN) { c->err = "zada_trained_open_decoder: the stub did not stop at a boundary"; return fail(ZADA_E_DATA); }
  if (skip > fin) hipMemcpyAsync(h->d_prefix, stub + fin, skip - fin, hipMemcpyHostToDevice, st);
  if (hip_check(c, hipStreamSynchronize(st), "trained: the stub")) return fail(ZADA_E_HIP);
  h->prefix_len = skip - fin;
  h->info.dec_fork_in = fin; h->info.dec_fork_out = fout;
  *hp = h;
  return ZADA_OK;
}

int zada_trained_decode_device(zada_ctx *z, zada_trained *h, int count, const zada_trained_entry *ent, uint64_t *out_len, int *rc_out) {
  int rc = tr_check(z, h, 2, count, ent, out_len, rc_out, "zada_trained_decode_device");
  if (rc) return rc;
  Ctx *c = &z->c;
  h->info.forked = h->info.unforked = 0;
  if (count == 0) return ZADA_OK;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  const uint64_t limit = (uint64_t)c->knob_batch_mib << 20;
  UlzResult bad{};
  int bad_entry = -1;
  c->tbegin();
  for (int g0 = 0; g0 < count;) {
    uint64_t bytes = 0;
    int g1 = g0;
    while (g1 < count) {
      const uint64_t b = a16(h->skip + ent[g1].n) + a16(h->t_len + ent[g1].cap);
      if (g1 > g0 && bytes + b > limit) break;
      bytes += b; g1++;
    }
    rc = tr_decode_group(c, h, g0, g1, ent, out_len, rc_out, &bad, &bad_entry);
    if (rc) { hipStreamSynchronize(c->stream); (void)hipGetLastError(); c->tend(); return rc; }
    g0 = g1;
  }
  c->tend();
  (h->d_snap && c->knob_trained_fork ? h->info.forked : h->info.unforked) = (uint64_t)count;
  if (bad_entry >= 0) {
    char buf[240];
    snprintf(buf, sizeof buf, "trained decode: entry %d: %s at message byte %llu", bad_entry, ulz_rule_name(bad.rule), (unsigned long long)bad.in_pos);
    c->err = buf;
    return ZADA_E_DATA;
  }
  return ZADA_OK;
}

int zada_trained_encode_device(zada_ctx *z, zada_trained *h, int count, const zada_trained_entry *ent, uint64_t *out_len, int *rc_out) {
  int rc = tr_check(z, h, 1, count, ent, out_len, rc_out, "zada_trained_encode_device");
  if (rc) return rc;
  Ctx *c = &z->c;
  for (int i = 0; i < count; i++)
    if (h->t_len + ent[i].n >= (2ull << 30) - 65536) { c->err = "zada_trained_encode_device: trainer and data of 2 GiB or more"; return ZADA_E_TOO_LARGE; }
  h->info.forked = h->info.unforked = 0;
  if (count == 0) return ZADA_OK;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  c->lz_resume.clear();                                             // (an imported state is another stream's)
  bool small = false, refused = false;
  std::vector<int> group;
  uint64_t gbytes = 0;
  auto flush_group = [&]() -> int {
    if (group.empty()) return 0;
    const int r = tr_encode_group(c, h, group, ent, out_len, rc_out, &small, &refused);
    if (r) { hipStreamSynchronize(c->stream); hipStreamSynchronize(c->stream2); (void)hipGetLastError(); }
    group.clear(); gbytes = 0;
    return r;
  };
  for (int i = 0; i < count; i++) {
    const uint64_t slot = (h->t_len + ent[i].n + 63) & ~63ull;
    if (gbytes + slot > (1ull << 30) && (rc = flush_group())) return rc;
    group.push_back(i); gbytes += slot;
  }
  if ((rc = flush_group())) return rc;
  if (refused) return ZADA_E_REFERENCE;                             // (its text is lzma_batch_refused's)
  if (small) { c->err = ERR_OUTPUT_TOO_SMALL; return ZADA_E_INVALID; }
  return ZADA_OK;
}

int zada_trained_info(const zada_trained *h, zada_trained_info_t *info) {
  if (!h || !info) return ZADA_E_INVALID;
  *info = h->info;
  return ZADA_OK;
}

void zada_trained_close(zada_trained *h) {
  if (!h) return;
  if (hipSetDevice(h->device) == hipSuccess) hipDeviceSynchronize();   // (the context may be gone already: nothing of it is read here)
  tr_free(h);
}
