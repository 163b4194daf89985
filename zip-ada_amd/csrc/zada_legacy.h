// zada_legacy.h -- Shrink_1 and Reduce_1 .. _4 (zada_shrink.hip, zada_reduce.hip): what the entry points in zada_api.hip hand to the kernels.
#pragma once
#include <stdint.h>
#include <vector>
#include "zada_internal.h"
#include "zada_legacy_plan.h"

namespace zada {

// one entry of a launch group: its bytes in the input arena, its slot in the output arena
struct LegacyJob { uint32_t in_off, n, out_off, cap; };

// E entries of d_in (jobs [e].in_off, .n) into their slots of d_out, one wave per entry; bytes [e] = the stream's length (a stream that is longer
// than its slot of jobs [e].cap bytes is cut there, never written beyond).  The output arena need not be cleared.  Synchronises the context's stream.
int shrink_encode_group(Ctx *c, uint32_t E, const uint8_t *d_in, const LegacyJob *jobs, uint8_t *d_out, uint64_t *bytes);
// the same for Reduce, factor 1 .. 4; d_out [0, out_bytes) is the output arena (cleared here: the emit kernel ORs bits into it)
int reduce_encode_group(Ctx *c, int factor, uint32_t E, const uint8_t *d_in, const LegacyJob *jobs, uint8_t *d_out, uint64_t out_bytes, uint64_t *bytes);
// what the last reduce_encode_group left on the device, for the tests: what = 0 the raw bytes of `entry`, 1 its Slen (256), 2 its followers (256 x 32)
uint64_t reduce_last_record(Ctx *c, int what, uint32_t entry, uint8_t *dst, uint64_t cap);
void legacy_destroy(Ctx *c);
// one stream from device memory into device memory behind the argument checks (zada_api.hip): ZADA_OK, ZADA_INEFFICIENT (nothing is written: the
// stream does not beat its input), ZADA_E_TOO_LARGE, or ZADA_E_INVALID with ERR_OUTPUT_TOO_SMALL; `who` names the entry point in the other texts
int legacy_device_one(::zada_ctx *z, int method, const void *d_in, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len, uint32_t *crc_inout, const char *who);

// the device buffers of these two methods, made on first use (Ctx::lg)
struct LegacyState {
  void *tab = nullptr; size_t cap_tab = 0;             // a group's jobs, then its stream lengths (and Reduce's raw lengths)
  void *work = nullptr; size_t cap_work = 0;           // Reduce: raw bytes, pair counts, follower positions, followers, Slen of a group's entries
  // the last Reduce group, for reduce_last_record
  uint32_t E = 0;
  uint8_t *d_raw = nullptr, *d_foll = nullptr, *d_slen = nullptr;
  std::vector<uint64_t> raw_start;
  std::vector<uint32_t> raw_len;
};
LegacyState *legacy_state(Ctx *c);
int legacy_grow(Ctx *c, void **p, size_t *cap, size_t bytes, const char *what);

}  // namespace zada
