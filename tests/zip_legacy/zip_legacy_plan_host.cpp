// zip_legacy_plan_host.cpp -- what the knobs "zip_legacy" and "unzip_legacy" add to the host plans of zada_zip_device_ex and zada_rezip_device
// (zip-ada_amd/csrc/zada_zip_plan.h, zada_rezip_plan.h) for the CPU tests: a C interface for ctypes (tests/test_zip_legacy_plan.py).  Every function
// with a `_default` twin makes the call as the call sites from before the knobs make it: without the trailing parameter.
#include <stdint.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_zip_plan.h"
#include "../../zip-ada_amd/csrc/zada_rezip_plan.h"

using namespace zada;

extern "C" {

int zlp_method_ok(int m, int legacy) { return zw_method_ok_ex(m, legacy) ? 1 : 0; }
int zlp_method_ok_default(int m) { return zw_method_ok_ex(m) ? 1 : 0; }
int zlp_zip_type(int m) { return zw_zip_type(m); }
uint64_t zlp_slot(uint64_t n) { return legacy_slot(n); }
uint64_t zlp_footprint(uint64_t n) { return reduce_footprint(n); }
uint64_t zlp_entry_max(void) { return ZW_ENTRY_MAX; }
int zlp_too_large(const zada_zip_entry *ent, int count) { return zw_legacy_too_large(ent, count); }
// the groups: up to cap (g0, g1, kind) triples; returns how many there are
int zlp_groups(const zada_zip_entry *ent, int count, int method, uint64_t limit, uint64_t work_limit, int *groups, int cap) {
  std::vector<ZwGroup> g;
  zw_groups_legacy(ent, count, method, limit, work_limit, g);
  for (size_t k = 0; k < g.size() && (int)k < cap; k++) { groups[3 * k] = g[k].g0; groups[3 * k + 1] = g[k].g1; groups[3 * k + 2] = g[k].kind; }
  return (int)g.size();
}

uint32_t zlp_considered(uint32_t approaches, uint32_t formats, int legacy) { return rz_considered(approaches, formats, legacy); }
uint32_t zlp_considered_default(uint32_t approaches, uint32_t formats) { return rz_considered(approaches, formats); }
int zlp_methods(uint32_t considered, int p2, int p1, uint64_t usize, int *out) {
  std::vector<int> m;
  rz_methods(considered, p2, p1, m, usize);
  for (size_t i = 0; i < m.size(); i++) out[i] = m[i];
  return (int)m.size();
}
int zlp_methods_default(uint32_t considered, int p2, int p1, int *out) {
  std::vector<int> m;
  rz_methods(considered, p2, p1, m);
  for (size_t i = 0; i < m.size(); i++) out[i] = m[i];
  return (int)m.size();
}
uint32_t zlp_considered_entry(uint32_t considered, uint64_t usize) { return rz_considered_entry(considered, usize); }
int zlp_original_allowed(uint32_t formats, int method) { return rz_original_allowed(formats, (uint16_t)method) ? 1 : 0; }
int zlp_choose(const uint64_t *size, int original_allowed) { return rz_choose(size, original_allowed != 0); }
int zlp_rz_check(const zada_rezip_entry *ent, int count, uint64_t src_len, int legacy, int *bad, int *why) { return rz_check(ent, count, 1 << 20, src_len, 1ull << 40, 16, bad, why, legacy); }
int zlp_rz_check_default(const zada_rezip_entry *ent, int count, uint64_t src_len, int *bad, int *why) { return rz_check(ent, count, 1 << 20, src_len, 1ull << 40, 16, bad, why); }
const char *zlp_rz_why_text(int why, int legacy) { return rz_why_text(why, legacy); }
const char *zlp_rz_why_text_default(int why) { return rz_why_text(why); }
// the flag word rz_add writes for one entry
int zlp_flag(int method, int flags, int zip_type, int eos, int kept) {
  zada_rezip_entry e{0, 10, 100, 0, 0, (uint16_t)method, (uint16_t)flags, 20, 0, 1, (const uint8_t *)"x"};
  RzArchive A;
  std::vector<uint8_t> blob;
  rz_add(A, e, 10, (uint16_t)zip_type, eos != 0, blob, kept != 0);
  return A.dir[0].flag;
}
// The archive of made-up winners (payloads as lengths only), kept [i]: the winner is the source's own stream.  As rp_rz_archive
// (tests/rezip/rezip_plan_host.cpp) with that one column more.
uint64_t zlp_rz_archive(const zada_rezip_entry *ent, int count, const uint64_t *csize, const uint16_t *zip_type, const uint8_t *eos, const uint8_t *kept, uint64_t base,
                        const uint8_t *comment, uint32_t comment_len, uint8_t *out, uint64_t cap, uint64_t *archive_len) {
  RzArchive A;
  A.base = base;
  std::vector<uint8_t> blob;
  for (int i = 0; i < count; i++) {
    if (rz_dropped(ent[i])) continue;
    rz_add(A, ent[i], csize[i], zip_type[i], eos[i] != 0, blob, kept[i] != 0);
  }
  rz_finish(A, comment, comment_len, blob);
  *archive_len = A.pos;
  for (size_t j = 0; j < blob.size() && j < cap; j++) out[j] = blob[j];
  return blob.size();
}

}
