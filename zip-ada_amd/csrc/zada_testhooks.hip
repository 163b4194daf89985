// zada_testhooks.hip -- test hooks of the C ABI for the three device-only building blocks every byte-exact result rests on:
//   llhc_wave <max_bits>  (zada_llhc_wave.h)  Length_Limited_Coding on one wave,
//   radix_sort_pairs      (zada_sort.hip)     the stable key-value radix sort,
//   exclusive_scan_u32    (zada_lz.hip)       the exclusive prefix sum.
// The product reaches them only through whole streams; here they run on inputs a test chooses (tests/test_gpu_primitives.py).  The hooks
// call the product's own code, unchanged: the header's template and the two host functions.  Host pointers in and out, staged through
// device memory on the context's stream; buffers are made and freed per call (tests, not a hot path).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/zada.h"
#include "zada_internal.h"
#include "zada_llhc_wave.h"

struct zada_ctx { zada::Ctx c; };

namespace zada {
namespace {

constexpr int TH_MAXN = 288;                 // symbols llhc_wave's scratch is laid out for
constexpr size_t TH_GUARD = 256;             // bytes behind a buffer that must come back as they were filled
constexpr uint8_t TH_FILL = 0xA5;

// One wave per vector; WPG waves of a workgroup side by side, each in its own LLHC_WAVE_SCRATCH slice of one LDS array (as in
// k_block_analyze and the BZip2 entropy search).  Where the counts are read from changes from vector to vector, and differs between
// WPG = 1 and WPG = 4 for the same vector, so that a caller who runs both has had every vector read from LDS and from global memory:
//   0, 3  global memory, lengths written straight to global memory           (k_window_descr's histogram in HBM)
//   1     an LDS array of their own, lengths to an LDS array                 (k_block_analyze: st1 / st2 / dtmp -> bl1 / bl2)
//   2     the part of the wave's scratch the procedure uses only after it has read the counts, lengths to an LDS array (BZip2)
template <int max_bits, int WPG>
__global__ void __launch_bounds__(64 * WPG) k_test_llhc(const uint32_t *__restrict__ freq, int n, uint32_t count, uint8_t *__restrict__ bl) {
  __shared__ __attribute__((aligned(16))) uint8_t S[WPG][LLHC_WAVE_SCRATCH];
  __shared__ uint32_t lf[WPG][TH_MAXN];
  __shared__ uint8_t lb[WPG][TH_MAXN];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t v = blockIdx.x * WPG + w;
  if (v >= count) return;                                           // (a whole wave; the kernel has no workgroup barrier)
  const uint32_t mode = (v + (v >> 2) + (WPG == 4 ? 2u : 0u)) & 3u;
  const uint32_t *f = freq + (size_t)v * n;
  uint8_t *out = bl + (size_t)v * n;
  if (mode == 0 || mode == 3) { llhc_wave<max_bits>(f, n, out, S[w], lane); return; }
  uint32_t *dst = mode == 1 ? lf[w] : (uint32_t *)(S[w] + 1728);
  for (int a = lane; a < n; a += 64) { dst[a] = f[a]; lb[w][a] = 0xFF; }
  wave_sync();
  llhc_wave<max_bits>(dst, n, lb[w], S[w], lane);
  wave_sync();
  for (int a = lane; a < n; a += 64) out[a] = lb[w][a];
}

template <int max_bits> void launch_llhc(hipStream_t st, int wpg, const uint32_t *freq, int n, uint32_t count, uint8_t *bl) {
  if (wpg == 4) hipLaunchKernelGGL((k_test_llhc<max_bits, 4>), dim3((count + 3) / 4), dim3(256), 0, st, freq, n, count, bl);
  else hipLaunchKernelGGL((k_test_llhc<max_bits, 1>), dim3(count), dim3(64), 0, st, freq, n, count, bl);
}

// device memory of one call: `bytes` + a guard behind them, filled with TH_FILL
struct Dev {
  uint8_t *p = nullptr; size_t bytes = 0;
  ~Dev() { if (p) hipFree(p); }
  bool make(hipStream_t st, size_t b) {
    bytes = b;
    if (hipMalloc((void **)&p, b + TH_GUARD) != hipSuccess) { p = nullptr; return false; }
    return hipMemsetAsync(p, TH_FILL, b + TH_GUARD, st) == hipSuccess;
  }
  bool put(hipStream_t st, const void *h) { return hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, st) == hipSuccess; }
  bool get(hipStream_t st, void *h) const { return hipMemcpyAsync(h, p, bytes, hipMemcpyDeviceToHost, st) == hipSuccess; }
  // (after the stream has been synchronised)
  bool guard_intact() const {
    uint8_t g[TH_GUARD];
    if (hipMemcpy(g, p + bytes, TH_GUARD, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (size_t i = 0; i < TH_GUARD; i++) if (g[i] != TH_FILL) return false;
    return true;
  }
};

int hook_fail(Ctx *c, hipStream_t st, const char *what) {
  hipStreamSynchronize(st);
  (void)hipGetLastError();
  c->err = what;
  return ZADA_E_HIP;
}

}  // namespace
}  // namespace zada

using namespace zada;

// freq: count vectors of n counts; bl: count x n code lengths.  ZADA_E_INVALID also for what the reference's procedure refuses or the
// product never feeds: more used symbols than 2 ** max_bits can code, a vector whose counts add up to 2 ** 27 or more.
extern "C" int zada_test_llhc(zada_ctx *z, int max_bits, int n, uint32_t count, int waves_per_group, const uint32_t *freq, uint8_t *bl) {
  if (!z || !freq || !bl || n < 1 || n > TH_MAXN || (max_bits != 7 && max_bits != 15 && max_bits != 16 && max_bits != 17) ||
      (waves_per_group != 1 && waves_per_group != 4) || count > (1u << 24))
    return ZADA_E_INVALID;
  Ctx *c = &z->c;
  if (count == 0) return ZADA_OK;
  for (uint32_t v = 0; v < count; v++) {
    uint64_t sum = 0; int ns = 0;
    for (int a = 0; a < n; a++) { const uint32_t f = freq[(size_t)v * n + a]; sum += f; ns += f > 0; }
    if (sum >= (1ull << 27) || ns > (1 << max_bits)) { c->err = "zada_test_llhc: a vector the reference's procedure does not take"; return ZADA_E_INVALID; }
  }
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  hipStream_t st = c->stream;
  const size_t cells = (size_t)count * n;
  Dev d_freq, d_bl;
  if (!d_freq.make(st, cells * 4) || !d_bl.make(st, cells)) return hook_fail(c, st, "zada_test_llhc: device memory");
  if (!d_freq.put(st, freq)) return hook_fail(c, st, "zada_test_llhc: copy in");
  if (max_bits == 7) launch_llhc<7>(st, waves_per_group, (const uint32_t *)d_freq.p, n, count, d_bl.p);
  else if (max_bits == 15) launch_llhc<15>(st, waves_per_group, (const uint32_t *)d_freq.p, n, count, d_bl.p);
  else if (max_bits == 16) launch_llhc<16>(st, waves_per_group, (const uint32_t *)d_freq.p, n, count, d_bl.p);
  else launch_llhc<17>(st, waves_per_group, (const uint32_t *)d_freq.p, n, count, d_bl.p);
  if (hip_check(c, hipGetLastError(), "zada_test_llhc: launch")) return ZADA_E_HIP;
  if (!d_bl.get(st, bl)) return hook_fail(c, st, "zada_test_llhc: copy out");
  if (hip_check(c, hipStreamSynchronize(st), "zada_test_llhc")) return ZADA_E_HIP;
  if (!d_bl.guard_intact() || !d_freq.guard_intact()) { c->err = "zada_test_llhc: bytes behind a buffer were written"; return ZADA_E_HIP; }
  return ZADA_OK;
}

// n (key, value) pairs through radix_sort_pairs with a temporary buffer of exactly radix_sort_tmp_bytes (n, value_bytes).  in_place:
// keys_in == keys_out and vals_in == vals_out on the device.  Otherwise the inputs are read back and compared: ZADA_E_INVALID if the
// sort has changed them.
extern "C" int zada_test_radix_sort(zada_ctx *z, uint64_t n, int value_bytes, unsigned begin_bit, unsigned end_bit, int in_place, const uint32_t *keys,
                                    const void *vals, uint32_t *keys_out, void *vals_out) {
  if (!z || (value_bytes != 4 && value_bytes != 16) || begin_bit > end_bit || end_bit > 32 || n >= (1ull << 32) ||
      (n && (!keys || !vals || !keys_out || !vals_out)))
    return ZADA_E_INVALID;
  Ctx *c = &z->c;
  if (n == 0) return ZADA_OK;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  hipStream_t st = c->stream;
  const size_t kb = (size_t)n * 4, vb = (size_t)n * value_bytes, tb = radix_sort_tmp_bytes(n, value_bytes);
  Dev d_k, d_v, d_ko, d_vo, d_tmp;
  if (!d_k.make(st, kb) || !d_v.make(st, vb) || !d_tmp.make(st, tb) || (!in_place && (!d_ko.make(st, kb) || !d_vo.make(st, vb)))) return hook_fail(c, st, "zada_test_radix_sort: device memory");
  if (!d_k.put(st, keys) || !d_v.put(st, vals)) return hook_fail(c, st, "zada_test_radix_sort: copy in");
  const Dev &ko = in_place ? d_k : d_ko, &vo = in_place ? d_v : d_vo;
  if (radix_sort_pairs(c, st, d_tmp.p, tb, (const uint32_t *)d_k.p, (uint32_t *)ko.p, d_v.p, vo.p, (size_t)value_bytes, n, begin_bit, end_bit)) {
    hipStreamSynchronize(st); (void)hipGetLastError(); return ZADA_E_HIP;
  }
  if (!ko.get(st, keys_out) || !vo.get(st, vals_out)) return hook_fail(c, st, "zada_test_radix_sort: copy out");
  std::vector<uint8_t> back;
  if (!in_place) {
    back.resize(kb + vb);
    if (!d_k.get(st, back.data()) || !d_v.get(st, back.data() + kb)) return hook_fail(c, st, "zada_test_radix_sort: copy back");
  }
  if (hip_check(c, hipStreamSynchronize(st), "zada_test_radix_sort")) return ZADA_E_HIP;
  if (!d_k.guard_intact() || !d_v.guard_intact() || !d_tmp.guard_intact() || (!in_place && (!d_ko.guard_intact() || !d_vo.guard_intact()))) {
    c->err = "zada_test_radix_sort: bytes behind a buffer were written"; return ZADA_E_HIP;
  }
  if (!in_place && (memcmp(back.data(), keys, kb) || memcmp(back.data() + kb, vals, vb))) { c->err = "zada_test_radix_sort: the sort changed its inputs"; return ZADA_E_INVALID; }
  return ZADA_OK;
}

// out [i] = in [0] + ... + in [i - 1] (mod 2 ** 32), *total = the sum of all n, through exclusive_scan_u32.  in_place: d_in == d_out.
extern "C" int zada_test_scan(zada_ctx *z, uint64_t n, int in_place, const uint32_t *in, uint32_t *out, uint32_t *total) {
  if (!z || !in || !out || !total || n == 0 || n > (1ull << 30)) return ZADA_E_INVALID;      // (k_scan_sums: at most 2 ** 20 blocks of 1 024)
  Ctx *c = &z->c;
  if (hipSetDevice(c->device) != hipSuccess) return ZADA_E_HIP;
  hipStream_t st = c->stream;
  const size_t nb = (size_t)((n + 1023) / 1024);
  Dev d_in, d_out, d_sums, d_total;
  if (!d_in.make(st, n * 4) || (!in_place && !d_out.make(st, n * 4)) || !d_sums.make(st, nb * 4) || !d_total.make(st, 4)) return hook_fail(c, st, "zada_test_scan: device memory");
  if (!d_in.put(st, in)) return hook_fail(c, st, "zada_test_scan: copy in");
  const Dev &o = in_place ? d_in : d_out;
  exclusive_scan_u32(st, (const uint32_t *)d_in.p, (uint32_t *)o.p, (uint32_t *)d_sums.p, (uint32_t *)d_total.p, (uint32_t)n);
  if (hip_check(c, hipGetLastError(), "zada_test_scan: launch")) return ZADA_E_HIP;
  if (!o.get(st, out) || !d_total.get(st, total)) return hook_fail(c, st, "zada_test_scan: copy out");
  std::vector<uint32_t> back;
  if (!in_place) { back.resize(n); if (!d_in.get(st, back.data())) return hook_fail(c, st, "zada_test_scan: copy back"); }
  if (hip_check(c, hipStreamSynchronize(st), "zada_test_scan")) return ZADA_E_HIP;
  if (!d_in.guard_intact() || (!in_place && !d_out.guard_intact()) || !d_sums.guard_intact() || !d_total.guard_intact()) {
    c->err = "zada_test_scan: bytes behind a buffer were written"; return ZADA_E_HIP;
  }
  if (!in_place && memcmp(back.data(), in, n * 4)) { c->err = "zada_test_scan: the scan changed its input"; return ZADA_E_INVALID; }
  return ZADA_OK;
}
