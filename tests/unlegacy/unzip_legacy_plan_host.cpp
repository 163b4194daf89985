// unzip_legacy_plan_host.cpp -- the argument checks of zada_unzip_device, zada_compzip_device and zada_findzip_device with and without the knob
// "unzip_legacy" (zip-ada_amd/csrc/zada_unzip_plan.h, zada_rezip_plan.h, zada_find_plan.h) for the CPU tests: a C interface for ctypes
// (tests/test_unzip_legacy_plan.py).
#include <stdint.h>
#include "../../zip-ada_amd/csrc/zada_unzip_plan.h"
#include "../../zip-ada_amd/csrc/zada_rezip_plan.h"
#include "../../zip-ada_amd/csrc/zada_find_plan.h"

using namespace zada;

extern "C" {

int ulp_check(const zada_unzip_entry *ent, int count, uint64_t archive_len, uint64_t out_bytes, int have_out, int have_keys, int legacy, int *bad, int *why) {
  return uz_check(ent, count, archive_len, out_bytes, have_out, have_keys, bad, why, legacy);
}
// the same call as every call site from before the knob makes it: without the trailing parameter
int ulp_check_default(const zada_unzip_entry *ent, int count, uint64_t archive_len, uint64_t out_bytes, int have_out, int have_keys, int *bad, int *why) {
  return uz_check(ent, count, archive_len, out_bytes, have_out, have_keys, bad, why);
}
int ulp_find_check(const zada_unzip_entry *ent, int count, uint64_t archive_len, int have_keys, int legacy, int *bad, int *why) {
  return fz_check(ent, count, archive_len, have_keys, bad, why, legacy);
}
int ulp_comp_check(const zada_unzip_entry *a, const zada_unzip_entry *b, int count, uint64_t len_a, uint64_t len_b, int have_keys, int legacy, int *bad, int *side, int *why) {
  return cz_check(a, b, count, len_a, len_b, have_keys, bad, side, why, legacy);
}
const char *ulp_why_text(int why, int legacy) { return uz_why_text(why, legacy); }
const char *ulp_why_text_default(int why) { return uz_why_text(why); }
// ReZip's plan does not know the knob: 1 if it takes the method as a source
int ulp_rezip_knows(int method) { return uz_method_known((uint16_t)method) ? 1 : 0; }

}
