// Host check of csrc/hermite_block_plan.hpp: the launch shape of the Hermite block steps' active-set kernel against the fixed step's,
// and the bound of its partial sums, for both orders (min_chunks = 1: order 4, min_chunks = 2: order 6).  No kernel is launched and no
// device is opened.
//     hipcc -std=c++17 --offload-host-only -I stdpar-nbody_amd/csrc -I include tools/hermite_block_plan_check.cpp -o hermite_block_plan_check
//  1. With every body active the plan IS hermite_plan_for(sz, min_chunks), field for field, for sz in 1 .. 200 000 (and at sizes up to
//     2^28): with max_level = 0 a block step then adds a body's sums in the order the fixed step adds them.
//  2. chunks * n_act (+ n_act where the chunks are reduced by the kernel of their own) never exceeds
//     hermite_block_part_slots(sz, min_chunks), chunks x tiles_per_chunk covers the tiles and no chunk is empty: every n_act for sz up
//     to 3000, a spread of n_act beyond.
#include <cstdio>
#include <cstdlib>

#include "hermite_block_plan.hpp"

using namespace nbody;

static int fail(const char* what, uint32_t sz, uint32_t n_act, uint32_t min_chunks) {
  std::printf("FAILED %s at sz = %u, n_act = %u, min_chunks = %u\n", what, sz, n_act, min_chunks);
  return 1;
}

static int check_bound(uint32_t sz, uint32_t n_act, uint32_t mc) {
  const hermite_plan p = hermite_block_plan_for(sz, n_act, mc);
  const uint64_t need  = uint64_t(p.chunks) * n_act + (p.chunks > kSerialChunks ? n_act : 0u);
  if (need > hermite_block_part_slots(sz, mc)) return fail("slot bound", sz, n_act, mc);
  if (p.chunks > kSerialChunks && n_act >= 2048u) return fail("reduced sums' 2048 slots", sz, n_act, mc);
  if (uint64_t(p.chunks) * p.tiles_per_chunk < p.ntiles || uint64_t(p.chunks - 1u) * p.tiles_per_chunk >= p.ntiles)
    return fail("cover of the tiles", sz, n_act, mc);
  if (uint64_t(p.blocks) * 64u * p.R < n_act || p.chunks > 65535u) return fail("grid", sz, n_act, mc);
  if (p.ntiles >= mc && p.chunks < mc) return fail("min_chunks chunks", sz, n_act, mc);
  return 0;
}

static int check_identity(uint32_t sz, uint32_t mc) {
  const hermite_plan a = hermite_block_plan_for(sz, sz, mc), b = hermite_plan_for(sz, mc);
  if (a.R != b.R || a.blocks != b.blocks || a.ntiles != b.ntiles || a.chunks != b.chunks || a.tiles_per_chunk != b.tiles_per_chunk)
    return fail("identity with hermite_plan_for(sz, min_chunks)", sz, sz, mc);
  return 0;
}

static int check_order(uint32_t mc) {
  for (uint32_t sz = 1; sz <= 200000u; ++sz)
    if (check_identity(sz, mc)) return 1;
  const uint32_t big[] = {262143u, 262144u, 262145u, 524288u, 1u << 20, (1u << 20) + 1u, 1u << 24, (1u << 28) - 1u, 1u << 28};
  for (uint32_t sz : big)
    if (check_identity(sz, mc)) return 1;
  for (uint32_t sz = 1; sz <= 3000u; ++sz)
    for (uint32_t n_act = 1; n_act <= sz; ++n_act)
      if (check_bound(sz, n_act, mc)) return 1;
  const uint32_t sizes[] = {4097u, 20000u, 65535u, 65536u, 65537u, 131072u, 200000u, 262144u, 262400u, 300000u, 1u << 20, 1u << 24, 1u << 28};
  for (uint32_t sz : sizes) {
    for (uint32_t n_act = 1; n_act <= sz && n_act <= 70000u; ++n_act)
      if (check_bound(sz, n_act, mc)) return 1;
    for (uint64_t n_act = 70001u; n_act <= sz; n_act += 997u)
      if (check_bound(sz, uint32_t(n_act), mc)) return 1;
    for (uint32_t back = 0; back < 300u && back < sz; ++back)
      if (check_bound(sz, sz - back, mc)) return 1;
  }
  return 0;
}

int main() {
  if (check_order(1u) || check_order(2u)) return 1;
  std::printf("ok\n");
  return 0;
}
