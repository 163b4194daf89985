// zada_inflate_par_batch_plan.h -- the host plan of the batched parallel Inflate (zada_inflate_par.hip, "inflate_par_batch"): the
// large entries of one zada_unzip_device group in the same launches.  Plain C++ without HIP, in the manner of zada_unzip_plan.h: the library's
// host side runs it between its launches, tests/inflate_par/inflate_par_batch_host.cpp runs the same text with every kernel as a loop.
//   passes     : the selected entries in table order, cut by the symbol workspace they may take ("inflate_par_batch_mib"): 2 bytes per promised
//                output byte (cap) for format 8, 4 for format 9; an entry that alone exceeds the bound is a pass of its own.
//   sub-passes : inside a pass one per format present, format 8 first: the two symbol widths are two instantiations of every kernel.
//   numbering  : stream s of a sub-pass has nch_s = ceil (n_in_s / chunk) chunks at the global indices [first_s, first_s + nch_s); a stream with
//                fewer than two chunks is not taken ("single chunk").  Bit positions stay the stream's own.
//   rounds     : infp_walk runs per stream on the stream's slice of the records.  A round collects the one pending repair job of every stream
//                whose walk asked for one; a stream that is damaged, passes its repair bound, ends with fewer than two live chunks or promises
//                more than its cap leaves with the reason inflate_par_try gives, and costs no further job.
//   live table : the surviving streams' live chunks, stream after stream, each row with its stream's index; per stream [first_live, n_live),
//                its addresses and its symbol base (the sum of the totals of the streams before it).
//   record     : per stream what inflate_par_try leaves in zada_inflate_par_info; infpb_sum adds them up in table order.
#pragma once
#include <stdint.h>
#include <vector>
#include "zada_inflate_par_logic.h"

namespace zada {

struct InfpbIn { uint64_t in, n_in, out, cap; uint32_t format, crc; };                 // a selected entry: addresses as integers, the register it starts from
struct InfpbRes { uint64_t out_len, in_used, chunks, live_chunks, repairs; uint32_t crc, taken, reason, pad; };   // taken: finished on this path (reason = 0)
// what the kernels read
struct InfpbJob { uint64_t start_bit; uint32_t chunk, stream; };                        // scout: the chunk's GLOBAL index, its stream, the exact start or INFP_SEARCH
struct InfpbStream { uint64_t in, n_in, out, sym; uint32_t first, first_live, n_live, pad; };   // sym: the stream's first symbol in the workspace; n_live = 0: it left
struct InfpbLive { uint64_t start_bit, stop_bits, off, bytes, end_bit; uint32_t rule, final, stream, pad; };   // InfpLive and the stream's index

inline uint64_t infpb_sym_bytes(uint32_t format) { return format == 9 ? sizeof(InfpFmt<9>::sym_t) : sizeof(InfpFmt<8>::sym_t); }
inline uint64_t infpb_chunks(uint64_t n_in, uint64_t chunk_bytes) { return (n_in + chunk_bytes - 1) / chunk_bytes; }

// The passes: ends receives the index behind every pass's last entry.  limit: bytes of symbol workspace one pass may promise.
inline void infpb_passes(const InfpbIn *in, uint32_t n, uint64_t limit, std::vector<uint32_t> &ends) {
  ends.clear();
  for (uint32_t p0 = 0; p0 < n;) {
    uint64_t bytes = 0;
    uint32_t p1 = p0;
    while (p1 < n && (p1 == p0 || bytes + in[p1].cap * infpb_sym_bytes(in[p1].format) <= limit)) { bytes += in[p1].cap * infpb_sym_bytes(in[p1].format); p1++; }
    ends.push_back(p1);
    p0 = p1;
  }
}

enum { INFPB_WALKING = 0, INFPB_CHAINED = 1, INFPB_OUT = 2 };
struct InfpbState {                                    // one stream of a sub-pass
  uint32_t row = 0;                                    // its index among the call's selected entries
  uint32_t first = 0, nch = 0;                         // its chunks: [first, first + nch) of the sub-pass
  uint32_t state = INFPB_WALKING, reason = INFP_NONE;
  uint32_t slot = 0;                                   // its row of the stream table the decode sees
  uint64_t bound = 0;
  InfpWalk W;
};
struct InfpbSub {
  uint32_t format = 8, pct = 0;
  uint64_t chunk_bytes = 0, nchunks = 0;
  uint32_t launches = 0;                               // scout launches made: the first and one per round that had a job
  std::vector<InfpbState> st;
  std::vector<InfpRec> recs;                           // by global chunk index
  std::vector<uint8_t> is_live;
  std::vector<uint64_t> off;
  std::vector<uint32_t> live_chunk;                    // live row -> global chunk index
  void leave(InfpbState &s, uint32_t why) { s.state = INFPB_OUT; s.reason = why; }
};

// The streams rows [k] (k in idx, all of `format`, each of two chunks or more) numbered, and the first launch's jobs: every chunk of every stream,
// a stream's chunk 0 exact at bit 0.  false: more chunks than 2 ** 31 (every stream leaves with "memory").
inline bool infpb_begin(InfpbSub &B, const InfpbIn *rows, const std::vector<uint32_t> &idx, uint32_t format, uint64_t chunk_bytes, uint32_t pct, std::vector<InfpbJob> &jobs) {
  B = InfpbSub();
  B.format = format; B.pct = pct; B.chunk_bytes = chunk_bytes;
  B.st.resize(idx.size());
  uint64_t at = 0;
  bool fits = true;
  for (size_t s = 0; s < idx.size(); s++) {
    InfpbState &S = B.st[s];
    const uint64_t nch = infpb_chunks(rows[idx[s]].n_in, chunk_bytes);
    S.row = idx[s];
    if (at + nch >= (1ull << 31)) fits = false;
    if (!fits) { S.nch = (uint32_t)(nch < 0xFFFFFFFFu ? nch : 0xFFFFFFFFu); B.leave(S, INFP_MEMORY); continue; }
    S.first = (uint32_t)at; S.nch = (uint32_t)nch; S.bound = infp_repair_bound(nch, pct);
    at += nch;
  }
  B.nchunks = at;
  jobs.clear();
  if (!fits) { for (InfpbState &S : B.st) if (S.state != INFPB_OUT) B.leave(S, INFP_MEMORY); B.nchunks = 0; return false; }
  jobs.reserve((size_t)at);
  for (size_t s = 0; s < B.st.size(); s++)
    for (uint32_t k = 0; k < B.st[s].nch; k++) jobs.push_back(InfpbJob{k ? INFP_SEARCH : 0ull, B.st[s].first + k, (uint32_t)s});
  B.recs.assign((size_t)at, InfpRec{0, 0, 0, 0, 0});
  B.is_live.assign((size_t)at, 0);
  B.off.assign((size_t)at, 0);
  return true;
}

// One round of the chain: every stream that is still walking goes on from where it stood (the records of the last launch are in B.recs).  jobs
// receives the repair jobs of this round, one per stream at the most; none: the chain is over for every stream.
inline void infpb_round(InfpbSub &B, const InfpbIn *rows, std::vector<InfpbJob> &jobs) {
  jobs.clear();
  for (size_t s = 0; s < B.st.size(); s++) {
    InfpbState &S = B.st[s];
    if (S.state != INFPB_WALKING) continue;
    const int w = infp_walk(S.W, B.recs.data() + S.first, S.nch, B.chunk_bytes * 8, B.is_live.data() + S.first, B.off.data() + S.first);
    if (w == INFP_W_DAMAGED) { B.leave(S, INFP_DAMAGED); continue; }
    if (w == INFP_W_REPAIR) {
      if (S.W.repairs > S.bound) B.leave(S, INFP_REPAIRS);
      else jobs.push_back(InfpbJob{S.W.expect, S.first + S.W.cur, (uint32_t)s});
      continue;
    }
    if (S.W.total > rows[S.row].cap) B.leave(S, INFP_DAMAGED);
    else if (S.W.live < 2) B.leave(S, INFP_SINGLE_CHUNK);
    else S.state = INFPB_CHAINED;
  }
}

// The tables of the decode: the chained streams in order (streams), their live chunks stream after stream (lives).  Returns the symbols of the
// sub-pass: the workspace is that many times infpb_sym_bytes.
inline uint64_t infpb_tables(InfpbSub &B, const InfpbIn *rows, std::vector<InfpbStream> &streams, std::vector<InfpbLive> &lives) {
  streams.clear(); lives.clear(); B.live_chunk.clear();
  uint64_t sym = 0;
  for (InfpbState &S : B.st) {
    if (S.state != INFPB_CHAINED) continue;
    const InfpbIn &R = rows[S.row];
    S.slot = (uint32_t)streams.size();
    InfpbStream T{R.in, R.n_in, R.out, sym, S.first, (uint32_t)lives.size(), 0, 0};
    for (uint32_t k = 0; k < S.nch; k++) {
      if (!B.is_live[S.first + k]) continue;
      const InfpRec &C = B.recs[S.first + k];
      lives.push_back(InfpbLive{C.start_bit, ((uint64_t)k + 1) * B.chunk_bytes * 8, B.off[S.first + k], C.bytes, 0, 0, 0, S.slot, 0});
      B.live_chunk.push_back(S.first + k);
    }
    T.n_live = (uint32_t)lives.size() - T.first_live;
    streams.push_back(T);
    sym += S.W.total;
  }
  return sym;
}

// What the decode found (back: the live table as the kernel left it) against the count: a stream with any row that broke a rule, ended at another
// bit or disagrees about the final block leaves ("damaged"), its row of the stream table with n_live = 0.  Returns how many left.
inline uint32_t infpb_compare(InfpbSub &B, const std::vector<InfpbLive> &back, std::vector<InfpbStream> &streams) {
  uint32_t left = 0;
  for (InfpbState &S : B.st) {
    if (S.state != INFPB_CHAINED) continue;
    const InfpbStream &T = streams[S.slot];
    bool bad = false;
    for (uint32_t j = T.first_live; j < T.first_live + T.n_live; j++) {
      const InfpRec &C = B.recs[B.live_chunk[j]];
      if (back[j].rule || back[j].end_bit != C.end_bit || (back[j].final != 0) != ((C.flags & INFP_F_FINAL) != 0)) bad = true;
    }
    if (bad) { B.leave(S, INFP_DAMAGED); streams[S.slot].n_live = 0; left++; }
  }
  return left;
}

// every stream that is still in leaves (the workspace could not be had: "memory")
inline void infpb_drop(InfpbSub &B, uint32_t why) { for (InfpbState &S : B.st) if (S.state != INFPB_OUT) B.leave(S, why); }

// what the sub-pass leaves per entry (res [row]; the register is the caller's to fill for the entries that were taken)
inline void infpb_results(const InfpbSub &B, InfpbRes *res) {
  for (const InfpbState &S : B.st) {
    InfpbRes &R = res[S.row];
    R.chunks = S.nch; R.live_chunks = S.W.live; R.repairs = S.W.repairs; R.reason = S.reason; R.taken = S.state == INFPB_CHAINED;
    if (R.taken) { R.out_len = S.W.total; R.in_used = (B.recs[S.first + S.W.last].end_bit + 7) / 8; }
  }
}

// the summed record of a call: res [0 .. n) in table order; sum6 = chunks, live chunks, repairs, fell_back, reason (of the last that fell back), streams
inline void infpb_sum(const InfpbRes *res, uint32_t n, uint64_t *sum6) {
  for (int i = 0; i < 6; i++) sum6[i] = 0;
  for (uint32_t k = 0; k < n; k++) {
    sum6[0] += res[k].chunks; sum6[1] += res[k].live_chunks; sum6[2] += res[k].repairs; sum6[5]++;
    if (!res[k].taken) { sum6[3]++; sum6[4] = res[k].reason; }
  }
}

}  // namespace zada
