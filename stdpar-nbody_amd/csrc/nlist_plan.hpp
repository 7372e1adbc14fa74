// Host plan of the fixed-radius neighbour lists (csrc/nlist.inc, nbody_nlist_* of include/nbody_hip.h): every grid, strip count and
// trip count of a compute, from (n, capacity) alone.  Host arithmetic only, no kernel, no HIP include and nothing of the project's, so
// that tests/nlist_plan_main.cpp can sweep its invariants with the host compiler under the sanitizers.  nbody_nlist_create_on calls
// nlist_plan_for once; nlist_launch (knn.hip) launches what the plan says and the kernels use the same constants.
#pragma once
#include <cstdint>

namespace nbody {

constexpr uint32_t kNlBlock      = 256;         // lanes a block of the walks, the strip sums and the offsets (= kNtBlock)
constexpr uint32_t kNlWave       = 64;          // targets a wave of the walks; lanes a block of the ordering (one wave per body)
constexpr uint32_t kNlScanBlock  = 1024;        // lanes of the one block that scans the strip sums
constexpr uint32_t kNlMaxPerBody = 4096;        // NBODY_NLIST_MAX_PER_BODY: entries of the longest segment the ordering stages
constexpr uint32_t kNlMaxN       = 1u << 28;    // bodies
constexpr uint64_t kNlMaxCapacity = 1ull << 32;  // list entries

struct nlist_plan {
  uint32_t n = 0;
  uint64_t capacity     = 0;
  uint32_t padded       = 0;  // sorted positions: n rounded up to whole blocks; one lane of the walks each
  uint32_t walk_blocks  = 0;  // padded / kNlBlock: count walk, and fill walk if there is a list
  uint32_t strips       = 0;  // strips of kNlBlock bodies in body order: the strip sums, and the offsets' grid
  uint32_t scan_trips   = 0;  // rounds of kNlScanBlock strip sums the one scan block makes
  uint32_t order_blocks = 0;  // one wave per body; 0 for a counts-only handle (capacity 0), which launches neither fill nor ordering
  bool lists            = false;
};

// A count is < n <= 2^28, so a strip's sum is < 2^36 and the total < 2^56: strip sums, offsets and the total are 64-bit.
constexpr uint64_t nlist_strip_sum_max(uint32_t n) { return uint64_t(kNlBlock) * uint64_t(n - 1u); }

// false: n or capacity outside the ABI's range (nbody_nlist_create refuses those before it plans)
inline bool nlist_plan_for(uint32_t n, uint64_t capacity, nlist_plan* out) {
  if (n == 0u || n > kNlMaxN || capacity > kNlMaxCapacity) return false;
  nlist_plan p;
  p.n            = n;
  p.capacity     = capacity;
  p.walk_blocks  = (n + kNlBlock - 1u) / kNlBlock;
  p.padded       = p.walk_blocks * kNlBlock;
  p.strips       = p.walk_blocks;
  p.scan_trips   = (p.strips + kNlScanBlock - 1u) / kNlScanBlock;
  p.lists        = capacity != 0u;
  p.order_blocks = p.lists ? n : 0u;
  *out           = p;
  return true;
}

// Body i belongs to strip i / kNlBlock, lane i % kNlBlock; strip s is scanned in trip s / kNlScanBlock by lane s % kNlScanBlock.
constexpr uint32_t nlist_strip_of(uint32_t i) { return i / kNlBlock; }
constexpr uint32_t nlist_trip_of(uint32_t strip) { return strip / kNlScanBlock; }

}  // namespace nbody
