// Launch shape and partial-sum bound of the sixth-order block steps (hermite6_block.inc): host code only, in a header of its own so
// that tools/hermite6_block_plan_check.cpp can hold it to hermite_plan_for(sz, 2) without the kernels.
#pragma once
#include "hermite_tile.hpp"

namespace nbody {

constexpr uint32_t kH6SerialChunks = 64;  // up to here `correct` adds the chunks itself, one after the other (hermite_plan_for's most)

// Launch shape of the active-set force + jerk + snap, from (sz, n_act) alone: hermite_block_plan_for's rule (hermite_block.inc: the
// blocks counted over the ACTIVE targets, no cap of 64 on the chunks, down to one tile per chunk, about 2048 blocks in flight
// whatever n_act is) with at least two chunks once there are two tiles, as the sixth order's fixed step has them.  With n_act == sz
// it IS hermite_plan_for(sz, 2) for every sz (the cap of 64 binds below 2048 targets only, where a system has at most 8 tiles), so
// with max_level = 0 a block step adds a body's sums in the order nbody_hermite6_step adds them.
inline hermite_plan hermite6_block_plan_for(uint32_t sz, uint32_t n_act) {
  hermite_plan p;
  p.R      = n_act >= 65536u ? 2u : 1u;
  p.blocks = (n_act + 64u * p.R - 1u) / (64u * p.R);
  p.ntiles = (sz + kHTile - 1u) / kHTile;
  uint32_t want = (2048u + p.blocks - 1u) / p.blocks;
  if (want < 2u) want = 2u;
  if (want > p.ntiles) want = p.ntiles;
  p.tiles_per_chunk = (p.ntiles + want - 1u) / want;
  p.chunks          = (p.ntiles + p.tiles_per_chunk - 1u) / p.tiles_per_chunk;
  return p;
}

// Slots (one slot = 3 D values) the partial sums of any n_act in [1, sz] can need: chunks * n_act.  hermite_block_part_slots' bound
// with the second chunk counted: chunks <= ntiles gives ntiles * sz; chunks <= max(2, ceil(2048 / blocks)) and n_act <= 64 R blocks
// give chunks * n_act <= max(2 n_act, (2048 / blocks + 1) * 64 R blocks) <= max(2 sz, 262144 + sz + 128).
// More than kH6SerialChunks chunks means fewer than 32 blocks, n_act < 2048: their reduced sums take 2048 slots behind the chunks'.
inline uint64_t hermite6_block_part_slots(uint32_t sz) {
  const uint64_t a = uint64_t((sz + kHTile - 1u) / kHTile) * sz;
  uint64_t b       = 262144ull + sz + 128ull;
  if (b < 2ull * sz) b = 2ull * sz;
  return (a < b ? a : b) + 2048ull;
}

}  // namespace nbody
