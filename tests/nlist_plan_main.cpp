// csrc/nlist_plan.hpp on the host: the launch shapes of the fixed-radius neighbour lists for n around every boundary (the bucket of
// 32, the wave of 64, the block / strip of 256, the scan block of 1024 strips, the one-block sort's 2048) and n = 2^28, for a
// counts-only handle and capacities up to 2^32.  Checked: every body belongs to exactly one lane of one strip and to one lane of one
// walk block; every strip is scanned by exactly one lane of one trip; the ordering has one wave per body; the largest strip sum and
// the largest total fit 64 bits with room; no 32-bit quantity of the plan overflows.  A program of its own, built with
// -fsanitize=address,undefined by tests/test_nlist.py; no GPU, nothing of HIP.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nlist_plan.hpp"

using namespace nbody;

static int failures = 0;
#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond)) {                                     \
      std::printf("FAILED %s: ", #cond);               \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
      if (++failures > 20) std::exit(1);               \
    }                                                  \
  } while (0)

// the invariants that need no loop over the bodies
static void check_shape(uint32_t n, uint64_t capacity) {
  nlist_plan p;
  CHECK(nlist_plan_for(n, capacity, &p), "n=%u capacity=%llu", n, (unsigned long long)capacity);
  const uint64_t n64 = n;
  CHECK(p.n == n && p.capacity == capacity, "n=%u", n);
  // sorted positions: whole blocks, at least n, less than one block of padding; nothing wraps 32 bits
  CHECK(uint64_t(p.walk_blocks) * kNlBlock == uint64_t(p.padded), "n=%u", n);
  CHECK(uint64_t(p.padded) >= n64 && uint64_t(p.padded) - n64 < kNlBlock, "n=%u padded=%u", n, p.padded);
  CHECK(uint64_t(p.padded) == (n64 + kNlBlock - 1) / kNlBlock * kNlBlock, "n=%u", n);
  // strips: cover n, the last one not empty
  CHECK(uint64_t(p.strips) * kNlBlock >= n64 && (uint64_t(p.strips) - 1) * kNlBlock < n64, "n=%u strips=%u", n, p.strips);
  CHECK(nlist_strip_of(n - 1) == p.strips - 1, "n=%u", n);
  // the scan's trips: cover the strips, the last one not empty
  CHECK(uint64_t(p.scan_trips) * kNlScanBlock >= p.strips && (uint64_t(p.scan_trips) - 1) * kNlScanBlock < p.strips, "n=%u trips=%u", n, p.scan_trips);
  CHECK(nlist_trip_of(p.strips - 1) == p.scan_trips - 1, "n=%u", n);
  // the ordering: one wave per body, or none
  CHECK(p.lists == (capacity != 0) && p.order_blocks == (p.lists ? n : 0u), "n=%u", n);
  // grids stay below 2^31 blocks
  CHECK(p.walk_blocks < (1u << 31) && p.strips < (1u << 31) && p.order_blocks < (1u << 31), "n=%u", n);
  // a count is <= n - 1: the largest strip sum, the largest in-strip prefix and the largest total, in 64 bits with room
  const uint64_t strip_max = nlist_strip_sum_max(n);
  CHECK(strip_max == uint64_t(kNlBlock) * (n64 - 1), "n=%u", n);
  CHECK(strip_max < (1ull << 36), "n=%u", n);
  const unsigned __int128 total_max = (unsigned __int128)n64 * (n64 - 1);
  CHECK(total_max < ((unsigned __int128)1 << 56), "n=%u", n);
  CHECK((unsigned __int128)p.strips * strip_max >= total_max, "n=%u", n);             // the strips' sums can hold every count
  CHECK((unsigned __int128)p.strips * strip_max < ((unsigned __int128)1 << 63), "n=%u", n);  // ... and their scan does not wrap
  // the summary's key (count << 32) | ~index: the count fits its half
  CHECK(n64 - 1 < (1ull << 32), "n=%u", n);
  // list entries: capacity * 4 bytes fits size_t
  CHECK(capacity <= kNlMaxCapacity && capacity * 4 / 4 == capacity, "capacity=%llu", (unsigned long long)capacity);
}

// every body once: counted per strip lane, per walk lane and per ordering wave; every strip once per scan lane
static void check_cover(uint32_t n) {
  nlist_plan p;
  CHECK(nlist_plan_for(n, 1, &p), "n=%u", n);
  std::vector<unsigned char> strip_lane(size_t(p.strips) * kNlBlock, 0), walk_lane(p.padded, 0), scan_lane(size_t(p.scan_trips) * kNlScanBlock, 0);
  for (uint32_t i = 0; i < n; ++i) {
    const size_t s = size_t(nlist_strip_of(i)) * kNlBlock + i % kNlBlock;  // the lane of nlist_strip_kernel / nlist_offsets_kernel
    CHECK(s == i && s < strip_lane.size(), "n=%u i=%u", n, i);
    ++strip_lane[s];
  }
  for (uint32_t b = 0; b < p.walk_blocks; ++b)      // the walks: wave w of block b takes sorted positions 64 (4 b + w) ...
    for (uint32_t w = 0; w < kNlBlock / kNlWave; ++w) {
      const uint32_t wave = b * (kNlBlock / kNlWave) + w;
      if (uint64_t(wave) * kNlWave >= n) continue;  // the kernel's wave-uniform return
      for (uint32_t l = 0; l < kNlWave; ++l) {
        const uint32_t tp = wave * kNlWave + l;
        CHECK(tp < p.padded, "n=%u tp=%u", n, tp);  // the lane's own record is read: inside the padded array
        if (tp < n) ++walk_lane[tp];
      }
    }
  for (uint32_t s = 0; s < p.strips; ++s) ++scan_lane[size_t(nlist_trip_of(s)) * kNlScanBlock + s % kNlScanBlock];
  size_t bodies = 0, targets = 0, strips = 0;
  bool once = true;  // no lane twice
  for (unsigned char c : strip_lane) once &= c <= 1, bodies += c;
  for (unsigned char c : walk_lane) once &= c <= 1, targets += c;
  for (unsigned char c : scan_lane) once &= c <= 1, strips += c;
  CHECK(once, "n=%u: a lane holds two items", n);
  CHECK(bodies == n && targets == n && strips == p.strips, "n=%u: %zu bodies, %zu targets, %zu strips", n, bodies, targets, strips);
  CHECK(p.order_blocks == n, "n=%u", n);
}

int main() {
  const uint32_t edges[] = {1, 32, 64, 256, 1024, 2048, 4096, 65536, kNlBlock * kNlScanBlock, 2 * kNlBlock * kNlScanBlock, 1u << 24, 1u << 27, kNlMaxN};
  const uint64_t caps[]  = {0, 1, 4096, 1ull << 31, (1ull << 32) - 1, 1ull << 32};
  size_t shapes = 0, covers = 0;
  for (uint32_t e : edges)
    for (int d = -3; d <= 3; ++d) {
      const int64_t n = int64_t(e) + d;
      if (n < 1 || n > int64_t(kNlMaxN)) continue;
      for (uint64_t c : caps) check_shape(uint32_t(n), c), ++shapes;
      if (n <= (int64_t(1) << 24) + 3) check_cover(uint32_t(n)), ++covers;
    }
  check_cover(kNlMaxN);  // 2^28 bodies: 256 MB of counters for a moment
  ++covers;
  for (uint32_t n = 1; n <= 5000; ++n) check_shape(n, n % 3), ++shapes;
  // refusals
  nlist_plan p;
  CHECK(!nlist_plan_for(0, 0, &p), "n = 0");
  CHECK(!nlist_plan_for(kNlMaxN + 1, 0, &p), "n > 2^28");
  CHECK(!nlist_plan_for(1, kNlMaxCapacity + 1, &p), "capacity > 2^32");
  CHECK(nlist_plan_for(kNlMaxN, kNlMaxCapacity, &p) && p.strips == (1u << 20) && p.scan_trips == 1024 && p.padded == kNlMaxN, "the largest plan");
  if (failures) return 1;
  std::printf("%zu shapes, %zu covers\nnlist_plan ok\n", shapes, covers);
  return 0;
}
