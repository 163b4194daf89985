// zada_reader_host.h -- the host side the four stream readers share (zada_inflate.hip, zada_bunzip2.hip, zada_unlzma.hip, zada_unlegacy.hip): what
// follows the argument checks of zada_*_batch, zada_*_device and zada_*, the adapter of zada_unzip_device, zada_*_last_records, and the tables of a
// launch.  The argument checks stay spelled out at each entry point: they differ between the formats and are the ABI's documentation.
//
// A reader describes itself with a traits struct R:
//   Job, Res, State           its job and result records (Res has rc, out_len, in_used, crc) and its state, a ReaderState
//   word                      its name in the error texts
//   state (c)                 the context's state, made on first use; null: no memory
//   begin (S)                 a call begins: the records of the call before go
//   limit (c)                 bytes of streams and outputs one group of a batch may take
//   run (c, S, jobs, crc_in, res, entry0)   the jobs (device addresses) through the launches; entry0: the number of jobs [0] in the call
//   describe (c, R, entry)    the error text of a failed entry
// The HIP errors of this header are ZADA_E_HIP, the ABI's name (ZADA_E_HIP_ of zada_internal.h is the same value for files without zada.h).
#pragma once
#include <string.h>
#include <string>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_reader_plan.h"

namespace zada {

struct ReaderState {
  uint32_t *d_counter = nullptr;                       // the work counters of a call's launches
  DevBuf tabs, arena;                                  // jobs, orders, results of a launch / a group's inputs and outputs (the host-buffer entry points)
  std::vector<uint64_t> last_entries;                  // the last call, four values per entry (zada_*_last_records)
};

// what a reader's traits have unless it says otherwise
template <class J, class Rs, class St> struct ReaderTraits {
  typedef J Job;
  typedef Rs Res;
  typedef St State;
  static void begin(St *S) { S->last_entries.clear(); }
  static uint64_t limit(const Ctx *c) { return (uint64_t)c->knob_batch_mib << 20; }
};

template <class R> static typename R::State *reader_state(Ctx *c) {
  typename R::State *S = R::state(c);
  if (!S) c->err = std::string(R::word) + ": no memory for the tables";
  return S;
}

// ---- the tables of one launch sequence: jobs, order, the registers to start from (crc_in, null: none), results ----
template <class Job, class Res> struct ReaderTables { const Job *jobs; const uint32_t *order, *crc; Res *res; };

// carves them from S->tabs, sends jobs, order and registers on their way and clears `counters` work counters
template <class Job, class Res>
static int reader_tables_send(Ctx *c, ReaderState *S, const char *word, const std::vector<Job> &jobs, const std::vector<uint32_t> &order, const uint32_t *crc_in,
                              uint32_t counters, ReaderTables<Job, Res> &T) {
  const uint64_t E = jobs.size();
  const uint64_t o_jobs = 0, o_order = o_jobs + E * sizeof(Job), o_crc = o_order + E * 4, o_res = (o_crc + (crc_in ? E * 4 : 0) + 15) & ~15ull, total = o_res + E * sizeof(Res);
  const int rc = dev_grow(c, S->tabs, total, (std::string("hipMalloc (") + word + " tables)").c_str());
  if (rc) return rc;
  uint8_t *t = S->tabs.p;
  T = ReaderTables<Job, Res>{(const Job *)(t + o_jobs), (const uint32_t *)(t + o_order), (const uint32_t *)(t + o_crc), (Res *)(t + o_res)};
  hipStream_t st = c->stream;
  hipMemcpyAsync(t + o_jobs, jobs.data(), (size_t)E * sizeof(Job), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(t + o_order, order.data(), (size_t)E * 4, hipMemcpyHostToDevice, st);
  if (crc_in) hipMemcpyAsync(t + o_crc, crc_in, (size_t)E * 4, hipMemcpyHostToDevice, st);
  hipMemsetAsync(S->d_counter, 0, (size_t)counters * 4, st);
  return 0;
}
// ... and behind the launches: the results come back, the launches are checked, the stream is waited for
template <class Job, class Res> static int reader_tables_fetch(Ctx *c, const char *word, const ReaderTables<Job, Res> &T, std::vector<Res> &res) {
  hipMemcpyAsync(res.data(), T.res, res.size() * sizeof(Res), hipMemcpyDeviceToHost, c->stream);
  if (hip_check(c, hipGetLastError(), (std::string(word) + " launch").c_str()) || hip_check(c, hipStreamSynchronize(c->stream), word)) return ZADA_E_HIP;
  return 0;
}

// ---- zada_*_batch behind its argument checks (count > 0).  make_job (i, d_in, d_out): entry i's job from its addresses in the arena ----
template <class R, class MakeJob>
static int reader_batch(Ctx *c, int count, const uint8_t *const *in, const uint64_t *n_in, uint8_t *const *out, const uint64_t *cap, uint64_t *out_len, uint64_t *in_used,
                        uint32_t *crc, int *rc_out, MakeJob make_job) {
  typedef typename R::Job Job;
  typedef typename R::Res Res;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  typename R::State *S = reader_state<R>(c);
  if (!S) return ZADA_E_NOMEM;
  int worst = 0, worst_entry = -1;
  Res worst_rec{};
  const uint64_t limit = R::limit(c);
  const std::string arena_what = std::string("hipMalloc (") + R::word + " arena)", copy_what = std::string(R::word) + " copy out";
  std::vector<uint8_t> host;
  std::vector<Job> jobs;
  std::vector<Res> res;
  std::vector<uint32_t> regs;
  std::vector<uint64_t> ioff, ooff;
  R::begin(S);
  c->tbegin();
  for (int g0 = 0; g0 < count;) {
    const ReaderGroup G = reader_plan_group(g0, count, n_in, cap, limit);
    const uint32_t E = (uint32_t)(G.g1 - g0);
    const uint64_t in_bytes = G.in_bytes;
    int rc = dev_grow(c, S->arena, in_bytes + G.out_bytes + 16, arena_what.c_str());
    if (rc) { c->tend(); return rc; }
    host.resize(in_bytes ? in_bytes : 1);
    jobs.resize(E); regs.resize(E); ioff.resize(E); ooff.resize(E);
    reader_plan_offsets(G, n_in, cap, ioff.data(), ooff.data());
    for (uint32_t k = 0; k < E; k++) {
      const int i = g0 + (int)k;
      if (n_in[i]) memcpy(host.data() + ioff[k], in[i], n_in[i]);
      jobs[k] = make_job(i, (uint64_t)(uintptr_t)(S->arena.p + ioff[k]), (uint64_t)(uintptr_t)(S->arena.p + ooff[k]));
      regs[k] = crc ? crc[i] : 0u;
    }
    if (in_bytes) hipMemcpyAsync(S->arena.p, host.data(), in_bytes, hipMemcpyHostToDevice, c->stream);
    rc = R::run(c, S, jobs, regs.data(), res, (uint32_t)g0);
    if (rc) { hipStreamSynchronize(c->stream); (void)hipGetLastError(); c->tend(); return rc; }
    // the outputs come back in one piece up to the last byte any entry wrote
    const uint64_t hi = out ? reader_plan_extent(G, ooff.data(), [&](int k) { return res[k].rc == 0 ? (uint64_t)res[k].out_len : 0; }) : 0;
    host.resize(hi ? hi : 1);
    if (hi && (hip_check(c, hipMemcpyAsync(host.data(), S->arena.p + in_bytes, hi, hipMemcpyDeviceToHost, c->stream), copy_what.c_str()) ||
               hip_check(c, hipStreamSynchronize(c->stream), copy_what.c_str()))) { c->tend(); return ZADA_E_HIP; }
    for (uint32_t k = 0; k < E; k++) {
      const int i = g0 + (int)k;
      rc_out[i] = res[k].rc ? ZADA_E_DATA : ZADA_OK;
      if (out_len) out_len[i] = res[k].out_len;
      if (in_used) in_used[i] = res[k].in_used;
      if (res[k].rc) { if (worst == 0) { worst = ZADA_E_DATA; worst_entry = i; worst_rec = res[k]; } continue; }
      if (crc) crc[i] = res[k].crc;
      if (out && res[k].out_len) memcpy(out[i], host.data() + (ooff[k] - in_bytes), res[k].out_len);
    }
    g0 = G.g1;
  }
  c->tend();
  if (worst) R::describe(c, worst_rec, worst_entry);
  return worst;
}

// ---- zada_*_device behind its argument checks.  make_job (J): the one job from the call's arguments; what it returns but 0 ends the call ----
template <class R, class MakeJob> static int reader_device_one(Ctx *c, uint64_t *out_len, uint64_t *in_used, uint32_t *crc_inout, MakeJob make_job) {
  if (out_len) *out_len = 0;
  if (in_used) *in_used = 0;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  typename R::State *S = reader_state<R>(c);
  if (!S) return ZADA_E_NOMEM;
  std::vector<typename R::Job> jobs(1);
  int rc = make_job(jobs[0]);
  if (rc) return rc;
  std::vector<typename R::Res> res;
  const uint32_t reg = crc_inout ? *crc_inout : 0u;
  R::begin(S);
  c->tbegin();
  rc = R::run(c, S, jobs, &reg, res, 0u);
  c->tend();
  if (rc) { hipStreamSynchronize(c->stream); (void)hipGetLastError(); return rc; }
  if (res[0].rc) { R::describe(c, res[0], 0); return ZADA_E_DATA; }
  if (out_len) *out_len = res[0].out_len;
  if (in_used) *in_used = res[0].in_used;
  if (crc_inout) *crc_inout = res[0].crc;
  return ZADA_OK;
}

// ---- zada_* on one stream in host memory behind its argument checks: batch (out_len, in_used, crc, rc_out) is the batch call with count = 1 ----
template <class Batch> static int reader_single(uint64_t *out_len, uint64_t *in_used, uint32_t *crc_inout, Batch batch) {
  if (out_len) *out_len = 0;
  if (in_used) *in_used = 0;
  uint64_t ol = 0, iu = 0;
  uint32_t reg = crc_inout ? *crc_inout : 0u;
  int erc = 0;
  const int rc = batch(&ol, &iu, &reg, &erc);
  if (rc) return rc;
  if (out_len) *out_len = ol;
  if (in_used) *in_used = iu;
  if (crc_inout) *crc_inout = reg;
  return ZADA_OK;
}

// ---- R::run for zada_unzip_device (zada_internal.h).  make_job (rj): a ReaderJob as the reader's own ----
template <class R, class MakeJob> static int reader_run_jobs(Ctx *c, uint32_t E, const ReaderJob *rj, ReaderRes *rr, bool *described, MakeJob make_job) {
  if (E == 0) return 0;
  typename R::State *S = reader_state<R>(c);
  if (!S) return ZADA_E_NOMEM;
  std::vector<typename R::Job> jobs(E);
  std::vector<uint32_t> regs(E);
  std::vector<typename R::Res> res;
  for (uint32_t k = 0; k < E; k++) { jobs[k] = make_job(rj[k]); regs[k] = rr[k].crc; }
  R::begin(S);
  const int rc = R::run(c, S, jobs, regs.data(), res, 0u);
  if (rc) return rc;
  for (uint32_t k = 0; k < E; k++) {
    if (res[k].rc) { rr[k] = ReaderRes{ZADA_E_DATA, regs[k], 0, 0}; if (!*described) { R::describe(c, res[k], rj[k].index); *described = true; } }
    else rr[k] = ReaderRes{ZADA_OK, res[k].crc, res[k].out_len, res[k].in_used};
  }
  return 0;
}

// ---- zada_*_last_records: up to cap_items of v's values to dst; how many there are ----
static inline uint64_t reader_last_records(const std::vector<uint64_t> &v, uint64_t *dst, uint64_t cap_items) {
  const uint64_t n = v.size() < cap_items ? v.size() : cap_items;
  if (n) memcpy(dst, v.data(), n * 8);
  return v.size();
}

}  // namespace zada
