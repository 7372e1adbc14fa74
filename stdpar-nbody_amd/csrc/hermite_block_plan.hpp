// Launch shape and partial-sum bound of the Hermite block steps (hermite_block.inc, hermite6_block.inc): host code only, in a header
// of its own so that tools/hermite_block_plan_check.cpp can hold it to hermite_plan_for(sz, min_chunks) without the kernels.
// min_chunks is hermite_plan_for's: order 4 passes 1, order 6 passes 2.
#pragma once
#include "hermite_tile.hpp"

namespace nbody {

constexpr uint32_t kSerialChunks = 64;  // up to here `correct` adds the chunks itself, one after the other (hermite_plan_for's most)

// Launch shape of the active-set pair sum, from (sz, n_act) alone.  hermite_plan_for's rule with the blocks counted over the ACTIVE
// targets and no cap of 64 on the chunks: as n_act shrinks the tiles are cut finer over grid.y, down to one tile per chunk, so that
// about 2048 blocks are in flight whatever n_act is.  With n_act == sz it IS hermite_plan_for(sz, min_chunks) for every sz (the cap of
// 64 binds below 2048 targets only, where a system has at most 8 tiles), so with max_level = 0 a block step adds a body's sums in the
// order the fixed step adds them.
inline hermite_plan hermite_block_plan_for(uint32_t sz, uint32_t n_act, uint32_t min_chunks) {
  hermite_plan p;
  p.R      = n_act >= 65536u ? 2u : 1u;
  p.blocks = (n_act + 64u * p.R - 1u) / (64u * p.R);
  p.ntiles = (sz + kHTile - 1u) / kHTile;
  uint32_t want = (2048u + p.blocks - 1u) / p.blocks;
  if (want < min_chunks) want = min_chunks;
  if (want > p.ntiles) want = p.ntiles;
  p.tiles_per_chunk = (p.ntiles + want - 1u) / want;
  p.chunks          = (p.ntiles + p.tiles_per_chunk - 1u) / p.tiles_per_chunk;
  return p;
}

// Slots (one slot = G D values) the partial sums of any n_act in [1, sz] can need: chunks * n_act.  chunks <= ntiles gives
// ntiles * sz; chunks <= max(min_chunks, ceil(2048 / blocks)) and n_act <= 64 R blocks give
// chunks * n_act <= max(min_chunks n_act, (2048 / blocks + 1) * 64 R blocks) <= max(min_chunks sz, 262144 + sz + 128).
// More than kSerialChunks chunks means fewer than 32 blocks, n_act < 2048: their reduced sums take 2048 slots behind the chunks'.
inline uint64_t hermite_block_part_slots(uint32_t sz, uint32_t min_chunks) {
  const uint64_t a = uint64_t((sz + kHTile - 1u) / kHTile) * sz;
  uint64_t b       = 262144ull + sz + 128ull;
  if (b < uint64_t(min_chunks) * sz) b = uint64_t(min_chunks) * sz;
  return (a < b ? a : b) + 2048ull;
}

}  // namespace nbody
