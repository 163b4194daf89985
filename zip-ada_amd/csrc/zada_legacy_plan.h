// zada_legacy_plan.h -- Shrink_1 and Reduce_1 .. _4: the sizes a launch group is laid out by.  Plain C++ without HIP: zada_legacy.h hands them to the
// entry points in zada_api.hip, zada_zip_plan.h to the groups of zada_zip_device_ex.
#pragma once
#include <stdint.h>

namespace zada {

constexpr uint64_t LEGACY_ENTRY_MAX = (1ull << 30) - 65536;       // an entry of this many bytes and more is not taken

// A stream that is not shorter than its input is not delivered (Write_Block's rule, zip-compress.adb:468-490), so an entry's slot in the output
// arena holds its n bytes, rounded up to 64: the kernels write nothing beyond the slot and go on counting.
inline uint64_t legacy_slot(uint64_t n) { return n < 64 ? 64 : (n + 63) & ~63ull; }
// Reduce: a literal 144 takes two raw bytes, a pair three or four for at least four input bytes
inline uint64_t reduce_raw_bound(uint64_t n) { return 2 * n + 16; }
// device memory Reduce takes per entry besides its slots: pair counts, follower positions, followers, Slen, raw bytes
inline uint64_t reduce_footprint(uint64_t n) { return 256 * 256 * 4 + 256 * 256 + 256 * 32 + 256 + ((reduce_raw_bound(n) + 63) & ~63ull); }

}  // namespace zada
