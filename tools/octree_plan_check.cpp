// Host check of csrc/octree_plan.hpp: the octree's sizes, launches, multipole route, walk form and phase bookkeeping.  No kernel is
// launched and no device is opened.
//     hipcc -std=c++17 --offload-host-only -I stdpar-nbody_amd/csrc -I include tools/octree_plan_check.cpp -o octree_plan_check
// Swept over n = 1 .. 4097, both sides of every boundary below, and a ladder n = 4097 * 1.37^k up to 2^28, for both precisions, both
// dimensions, the shipped build forms (0, 1, 3), the three walk settings and a step budget of 0 and 77:
//  1. every grid is >= 1, grid x block fits 32 bits, and covers what the kernel is to do (bodies, positions 0 .. n, ranks, child slots,
//     the cells a level can hold, the slots of the round);
//  2. every index a launch can produce lies inside the planned buffer: later / later_mask against the chunks, later2 / later2_mask
//     against the blocks of the round (at most chunks * levels cells wait for it), the LDS tables of the round and the crown
//     (kMpMaxBlocks + 1 words), bsum and bhist against lcp_blocks, lcp and plocal against position n, tops against n / 2 cells at the
//     key depth, rankpos, cells and groups against max_cells, the node pool against capacity, lvl_count against slot levels + 6, the
//     sort's scratch against the blocks of the shard window's list, counters and quadrupoles against n and the nodes;
//  3. the one-block kernels only where one block suffices: insert up to kSmallB pairs, multipoles up to kSmallChunks chunks;
//  4. route, sizes and grids are functions of (elem, dim, n, build) alone: walk, budget and NBODY_OT_FORM do not move them;
//  5. the ISA walk exactly when the setting is not 1, max_cells < 2^24 and max_cells * group_bytes < 2^32; the refusals exactly for
//     setting 2; the budget is the step budget, or the capacity;
//  6. ot_level_cap against the width loop it replaced;  7. routes and shapes pinned by hand from the rules (where the GPU tests
//     name a size for a route, that size);  8. the truth table of ot_phases: every event from every state.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "octree_plan.hpp"
#include "radix_sort.hpp"

using namespace nbody;

static ot_request request(uint32_t elem, int dim, uint32_t n, int build = 0, int walk = 0, uint32_t budget = 0) {
  ot_request r;
  r.elem = elem, r.dim = dim, r.n = n, r.build = build, r.walk = walk, r.step_budget = budget;
  r.group_bytes = ot_group_bytes(elem, dim);
  r.sort_words  = radix_sort_scratch_words(n);
  return r;
}

static int fail(const char* what, const ot_request& r) {
  std::printf("FAILED %s at elem = %u, dim = %d, n = %u, build = %d, walk = %d, budget = %u\n", what, r.elem, r.dim, r.n, r.build, r.walk,
              r.step_budget);
  return 1;
}

static bool launch_ok(uint64_t grid, uint64_t block, uint64_t work) {
  return grid >= 1 && grid * block < (uint64_t(1) << 32) && grid * block >= work;
}

static bool same_launches(const ot_plan& a, const ot_plan& b) {
  return a.maxl == b.maxl && a.capacity == b.capacity && a.max_cells == b.max_cells && !std::memcmp(a.bytes, b.bytes, sizeof a.bytes) &&
         a.small_bounds == b.small_bounds && a.bounds_blocks == b.bounds_blocks && a.one_pass == b.one_pass &&
         a.small_insert == b.small_insert && a.keys_grid == b.keys_grid && a.lcp_blocks == b.lcp_blocks && a.scatter_grid == b.scatter_grid &&
         a.build_lcp_grid == b.build_lcp_grid && a.own_levels == b.own_levels &&
         !std::memcmp(a.build_level_grid, b.build_level_grid, sizeof a.build_level_grid) &&
         !std::memcmp(a.level_grid, b.level_grid, sizeof a.level_grid) && a.route == b.route && a.chunks == b.chunks &&
         a.small_threads == b.small_threads && a.round_blocks == b.round_blocks && a.ranks_grid == b.ranks_grid &&
         a.crown_reads_later2 == b.crown_reads_later2;
}

static int check(const ot_request& r) {
  const ot_plan p   = plan_octree(r);
  const uint64_t n  = r.n, nch = uint64_t(1) << r.dim, ML = uint64_t(ot_max_levels(r.dim));
  const size_t* z   = p.bytes;
  const uint64_t mc = p.max_cells;
  if (p.maxl != int(ML) || p.maxl > 32) return fail("levels", r);
  // sizes: the reference's node pool, and a group for every cell the pool can hold
  if (p.capacity != (nch * n < 1000 ? 1000 : nch * n) || mc != p.capacity / nch + 1) return fail("capacity", r);
  if (1 + mc * nch < p.capacity) return fail("groups hold fewer nodes than the pool", r);
  // 1: grids
  if (p.small_bounds != (n <= kSmallN) || p.bounds_blocks > 1024 || !launch_ok(p.bounds_blocks, kOB, 1)) return fail("bounds", r);
  if (!launch_ok(p.keys_grid, kOB, n) || !launch_ok(p.scatter_grid, kOB, n)) return fail("keys / scatter grid", r);
  if (!launch_ok(p.lcp_blocks, kLcpB, n + 1) || p.lcp_blocks > (uint64_t(1) << 20)) return fail("lcp blocks", r);
  if (!launch_ok(p.build_lcp_grid, kLcpBuildB, mc * nch)) return fail("build_lcp grid", r);
  if (!launch_ok(p.ranks_grid, kOB, mc)) return fail("ranks grid", r);
  if (!launch_ok(p.chunks, kMpChunk, mc) || uint64_t(p.chunks - 1) * kMpChunk >= mc) return fail("chunks", r);
  if (!launch_ok(p.round_blocks, kMpCrown, uint64_t(p.chunks) * ML)) return fail("round blocks", r);
  if (!launch_ok(ot_owned_blocks(r.n), kOC, n)) return fail("owned blocks", r);
  for (uint32_t count : {1u, r.n / 3 + 1, r.n})
    if (!launch_ok(ot_walk_grid(r.dim, count), 64, uint64_t(count) * nch) || uint64_t(ot_walk_grid(r.dim, count) - 1) * (64u >> r.dim) >= count)
      return fail("walk grid", r);
  for (int l = 0; l < p.maxl; ++l) {
    const uint64_t cap = ot_level_cap(r.dim, r.n, l);
    if (!launch_ok(p.build_level_grid[l], kOBuild, cap * nch) || !launch_ok(p.level_grid[l], kOB, cap)) return fail("level grids", r);
  }
  // 2: buffers
  if (z[kBufRoot] < r.elem * uint64_t(r.dim + 1) || z[kBufPartials] < uint64_t(2) * r.elem * p.bounds_blocks) return fail("root / partials", r);
  if (z[kBufKeys0] < 8 * n || z[kBufKeys1] < 8 * n || z[kBufIdx0] < 4 * n || z[kBufIdx1] < 4 * n) return fail("keys / idx", r);
  if (z[kBufHist] / 4 < radix_sort_scratch_words(r.n) || z[kBufHist] / 4 < ot_owned_blocks(r.n)) return fail("sort scratch", r);
  if (z[kBufRootrec] < (r.elem == 4 ? 32u : 64u)) return fail("root record", r);
  if (z[kBufGroups] < mc * r.group_bytes || z[kBufCells] < mc * 16 || z[kBufRankpos] < mc * 4) return fail("groups / cells / rankpos", r);
  if (z[kBufLvlCount] / 4 <= ML + 6) return fail("lvl_count", r);
  if (z[kBufTops] < (n / 2) * 16) return fail("tops", r);
  if (z[kBufLcp] <= n || z[kBufPlocal] / 4 <= n) return fail("lcp / plocal", r);
  if (z[kBufBsum] / 4 < p.lcp_blocks || n / kLcpB >= p.lcp_blocks || z[kBufBhist] / 4 < uint64_t(p.lcp_blocks) * (ML + 1)) return fail("bsum / bhist", r);
  if (z[kBufLater] / 4 < uint64_t(p.chunks) * ML || z[kBufLaterMask] / 4 < p.chunks) return fail("later", r);
  if (z[kBufLater2] / 4 < uint64_t(p.round_blocks) * ML || z[kBufLater2Mask] / 4 < p.round_blocks) return fail("later2", r);
  if (z[kBufCounters] < 8 * n) return fail("counters", r);
  if (z[kBufQuad] < uint64_t(r.elem) * (r.dim == 3 ? 9 : 5) * (mc * nch + 1)) return fail("quadrupoles", r);
  for (int b = 0; b < kOtBuffers; ++b)
    if (z[b] == 0) return fail("an empty buffer", r);
  // 3, and the routes
  if (p.one_pass != (r.build != 1) || p.small_insert != (p.one_pass && n <= kSmallN) || (p.small_insert && n > uint64_t(kSmallB))) return fail("insert", r);
  if (p.own_levels != p.maxl) return fail("own levels of a shipped form", r);
  const bool chunked = p.route == ot_mp_route::chunks_crown || p.route == ot_mp_route::chunks_round_crown;
  if ((p.route == ot_mp_route::levels) != !p.one_pass) return fail("levels route", r);
  if (p.one_pass) {
    const bool small = p.chunks == 1 || (r.elem == 4 && p.chunks <= kSmallChunks);
    if ((p.route == ot_mp_route::ranks_per_level) != (p.chunks > kMpMaxBlocks)) return fail("ranks-per-level route", r);
    if ((p.route == ot_mp_route::small_block) != small) return fail("one-block route", r);
    if (p.route == ot_mp_route::small_block && (p.small_threads != (r.elem == 4 ? 1024u : 512u) || p.chunks > kSmallChunks)) return fail("one-block threads", r);
    if (chunked && (p.route == ot_mp_route::chunks_round_crown) != (p.chunks > uint32_t(kMpCrown))) return fail("round", r);
    if (chunked && p.chunks > kMpMaxBlocks) return fail("more chunks than the round's LDS table holds", r);
    if (p.route == ot_mp_route::chunks_crown && p.chunks > uint32_t(kMpCrown)) return fail("more chunks than the crown takes", r);
    if (p.route == ot_mp_route::chunks_round_crown && p.round_blocks > kMpMaxBlocks) return fail("more round blocks than the crown's LDS table holds", r);
    if (p.small_insert && p.route != ot_mp_route::small_block && p.route != ot_mp_route::chunks_crown) return fail("route of a one-block tree", r);
  }
  if (p.crown_reads_later2 != (p.route == ot_mp_route::chunks_round_crown)) return fail("the crown's pair", r);
  // 4
  for (int walk : {0, 1, 2})
    for (uint32_t budget : {0u, 77u})
      for (bool compiled : {false, true}) {
        ot_request q = r;
        q.walk = walk, q.step_budget = budget, q.overrides.compiled_walk = compiled;
        if (!same_launches(p, plan_octree(q))) return fail("the launches follow the walk settings", r);
      }
  // 5
  const bool fits = mc < (uint64_t(1) << 24) && mc * r.group_bytes < (uint64_t(1) << 32);
  if (p.isa != (r.walk != 1 && fits)) return fail("ISA walk", r);
  if ((p.other_refusal != nullptr) != (r.walk == 2) || (p.other_refusal && p.other_refusal != kOtCompiledOnlyRefusal)) return fail("refusal of the other walks", r);
  if ((p.mono_refusal != nullptr) != (r.walk == 2 && !fits) || (p.mono_refusal && p.mono_refusal != kOtIsaRefusal)) return fail("refusal of the ISA walk", r);
  if (p.budget != (r.step_budget ? r.step_budget : p.capacity) || p.budget_set != (r.step_budget != 0)) return fail("budget", r);
  ot_request c = r;
  c.overrides.compiled_walk = true;
  if (plan_octree(c).isa) return fail("NBODY_OT_FORM=1", r);
  return 0;
}

static int check_n(uint32_t n) {
  for (uint32_t elem : {8u, 4u})
    for (int dim : {3, 2}) {
      for (int build : {0, 1, 3})
        for (int walk : {0, 1, 2})
          for (uint32_t budget : {0u, 77u})
            if (check(request(elem, dim, n, build, walk, budget))) return 1;
      // 6: the loop the three runners had
      uint64_t width = 1;
      for (int l = 0; l < ot_max_levels(dim); ++l) {
        const uint64_t cap_l = width < uint64_t(n / 2 + 1) ? width : uint64_t(n / 2 + 1);
        if (ot_level_cap(dim, n, l) != cap_l) return fail("ot_level_cap", request(elem, dim, n));
        if (width < (uint64_t(1) << 40)) width *= uint64_t(1) << dim;
      }
    }
  return 0;
}

// 7.  max_cells = n + 1 once 2^D n >= 1000, so chunks = ceil((n + 1) / 512): 1 up to n = 511, <= 3 up to 1535, <= 512 up to 262143,
// <= 8192 up to 4194303.
struct pin {
  ot_request r;
  ot_mp_route route;
  uint32_t chunks, round_blocks;  // round_blocks = 0: not pinned
  bool small_insert;
};
static int check_pins() {
  const auto d3 = [](uint32_t n, int build = 0) { return request(8, 3, n, build); };
  const auto f3 = [](uint32_t n, int build = 0) { return request(4, 3, n, build); };
  const ot_mp_route small = ot_mp_route::small_block, crown = ot_mp_route::chunks_crown, round = ot_mp_route::chunks_round_crown,
                    ranks = ot_mp_route::ranks_per_level, levels = ot_mp_route::levels;
  const pin pins[] = {
      {d3(1), small, 1, 0, true},
      {d3(511), small, 1, 0, true},
      {d3(512), crown, 2, 0, true},
      {d3(1000), crown, 2, 0, true},
      {d3(1024), crown, 3, 0, true},
      {d3(1025), crown, 3, 0, false},
      {d3(1024, 1), levels, 3, 0, false},
      {f3(511), small, 1, 0, true},
      {f3(1024), small, 3, 0, true},
      {f3(1025), small, 3, 0, false},
      {f3(1535), small, 3, 0, false},
      {f3(1536), crown, 4, 0, false},
      {request(4, 2, 1535), small, 3, 0, false},
      {request(4, 2, 1536), crown, 4, 0, false},
      {request(8, 2, 511), small, 1, 0, true},
      {request(8, 2, 512), crown, 2, 0, true},
      {d3(2049), crown, 5, 0, false},
      {d3(30011), crown, 59, 0, false},
      {d3(100000), crown, 196, 0, false},
      {f3(100000), crown, 196, 0, false},
      {d3(262143), crown, 512, 0, false},
      {d3(262144), round, 513, 22, false},
      {request(8, 2, 262144), round, 513, 33, false},
      {d3(300000), round, 586, 25, false},
      {d3(1000000), round, 1954, 81, false},
      {f3(1000000), round, 1954, 81, false},
      {d3(4194303), round, 8192, 336, false},
      {d3(4194304), ranks, 8193, 0, false},
      {d3(4300000), ranks, 8399, 0, false},
      {d3(4300000, 1), levels, 8399, 0, false},
  };
  for (const pin& q : pins) {
    const ot_plan p = plan_octree(q.r);
    if (p.route != q.route || p.chunks != q.chunks || (q.round_blocks && p.round_blocks != q.round_blocks) || p.small_insert != q.small_insert)
      return fail("pinned route", q.r);
  }
  // the capacity floor of 1000 nodes: up to n = 124 in 3D (8 * 125 = 1000 is the pool's own size), 249 in 2D
  const struct {
    int dim;
    uint32_t n, capacity, max_cells;
  } caps[] = {{3, 1, 1000, 126}, {3, 124, 1000, 126}, {3, 125, 1000, 126}, {3, 126, 1008, 127}, {2, 249, 1000, 251},
              {2, 250, 1000, 251}, {2, 251, 1004, 252}, {3, 1u << 28, 1u << 31, (1u << 28) + 1}};
  for (const auto& c : caps) {
    const ot_plan p = plan_octree(request(8, c.dim, c.n));
    if (p.capacity != c.capacity || p.max_cells != c.max_cells) return fail("pinned capacity", request(8, c.dim, c.n));
  }
  {  // shapes: n = 2049 in double 3D, one pass; n = 100 000, one launch per level; n = 4 300 000, ranks per level
    ot_plan p = plan_octree(d3(2049));
    if (p.small_bounds || p.bounds_blocks != 4 || p.keys_grid != 9 || p.lcp_blocks != 3 || p.scatter_grid != 9 || p.build_lcp_grid != 65 || p.ranks_grid != 9)
      return fail("pinned shape", d3(2049));
    p = plan_octree(d3(1024));
    if (!p.small_bounds || !p.small_insert) return fail("pinned shape", d3(1024));
    p = plan_octree(d3(100000, 1));
    const uint32_t build6[] = {1, 1, 1, 4, 32, 256, 391, 391}, level6[] = {1, 1, 1, 2, 16, 128, 196, 196};
    for (int l = 0; l < 8; ++l)
      if (p.build_level_grid[l] != build6[l] || p.level_grid[l] != level6[l]) return fail("pinned level grids", d3(100000, 1));
    if (p.build_level_grid[20] != 391 || p.own_levels != 21 || plan_octree(request(8, 2, 100000, 1)).own_levels != 32) return fail("pinned levels", d3(100000, 1));
    p = plan_octree(d3(4300000));
    if (p.ranks_grid != 16797 || p.bounds_blocks != 1024) return fail("pinned shape", d3(4300000));
    if (ot_walk_grid(3, 100000) != 12500 || ot_walk_grid(2, 100000) != 6250 || ot_walk_grid(3, 9) != 2 || ot_owned_blocks(100000) != 98) return fail("pinned walk grid", d3(100000));
  }
  {  // what the experiments build contributes: form 2 launches no level on its own, form 4 the hinted ones; one block per CU at most
    ot_request e = d3(100000, 2);
    e.overrides.ncu = 256;
    ot_plan p = plan_octree(e);
    if (p.one_pass || p.route != levels || p.own_levels != 0 || p.all_levels_build_grid != 256 || p.all_levels_mp_grid != 196) return fail("pinned form 2", e);
    e.build = 4, e.overrides.depth_hint = 9, e.overrides.ncu = 8;
    p = plan_octree(e);
    if (p.own_levels != 9 || p.all_levels_build_grid != 8 || p.all_levels_mp_grid != 8 || p.build_level_grid[6] != 391) return fail("pinned form 4", e);
    e.overrides.depth_hint = 64;
    if (plan_octree(e).own_levels != 21) return fail("pinned form 4 without a hint", e);
  }
  // the ISA walk's reach: 320-byte groups leave 32-bit offsets first (max_cells = 13 421 773), 192- and 128-byte groups 24-bit numbers
  if (!plan_octree(d3(13421771)).isa || plan_octree(d3(13421772)).isa) return fail("pinned ISA reach", d3(13421772));
  if (!plan_octree(f3(16777214)).isa || plan_octree(f3(16777215)).isa) return fail("pinned ISA reach", f3(16777215));
  if (!plan_octree(request(8, 2, 16777214)).isa || plan_octree(request(8, 2, 16777215)).isa) return fail("pinned ISA reach", request(8, 2, 16777215));
  return 0;
}

// 8.  States are the four flags (bounds 1, inserted 2, tree 4, quadrupoles 8).  bounds, insert, tree and quadrupoles set their flag; a
// new insert or tree (done or failed) leaves the quadrupoles describing another tree; clear and a change of build form keep the bounds
// alone.  An insert does not withdraw an earlier tree's flag (compute_tree after it rewrites every monopole), and a failed phase sets
// nothing.
static int check_phases() {
  for (unsigned s = 0; s < 16; ++s) {
    const auto from = [&] {
      ot_phases p;
      p.have_bounds = s & 1, p.inserted = s & 2, p.have_tree = s & 4, p.have_quad = s & 8;
      return p;
    };
    const auto bits = [](const ot_phases& p) { return unsigned(p.have_bounds) | p.inserted << 1 | p.have_tree << 2 | p.have_quad << 3; };
    ot_phases p = from();
    if (p.missing(ot_phase::bounds) != !(s & 1) || p.missing(ot_phase::inserted) != !(s & 2) || p.missing(ot_phase::tree) != !(s & 4) ||
        p.missing(ot_phase::quadrupoles) != !(s & 8))
      return 1;
    p.bounds_done();
    if (bits(p) != (s | 1u)) return 1;
    p = from(), p.insert_done();
    if (bits(p) != ((s | 2u) & ~8u)) return 1;
    p = from(), p.insert_failed();
    if (bits(p) != (s & ~8u)) return 1;
    p = from(), p.tree_done();
    if (bits(p) != ((s | 4u) & ~8u)) return 1;
    p = from(), p.tree_failed();
    if (bits(p) != (s & ~8u)) return 1;
    p = from(), p.quadrupoles_done();
    if (bits(p) != (s | 8u)) return 1;
    p = from(), p.cleared();
    if (bits(p) != (s & 1u)) return 1;
    p = from(), p.build_form_changed();
    if (bits(p) != (s & 1u)) return 1;
  }
  char a[256], b[256];
  std::snprintf(a, sizeof a, ot_phase_refusal(ot_phase::tree), "nbody_octree_compute_force");
  std::snprintf(b, sizeof b, ot_phase_refusal(ot_phase::bounds), "nbody_octree_insert");
  if (std::strcmp(a, "nbody_octree_compute_force before nbody_octree_compute_tree") || std::strcmp(b, "nbody_octree_insert before nbody_octree_compute_bounds"))
    return 1;
  return 0;
}

int main() {
  for (uint32_t n = 1; n <= 4097u; ++n)
    if (check_n(n)) return 1;
  for (uint32_t b : {30011u, 100000u, 262143u, 300000u, 1000000u, 4194303u, 4300000u, 13421771u, 16777214u, (1u << 28) - 1u})
    for (uint32_t n = b - 1; n <= b + 2; ++n)
      if (check_n(n)) return 1;
  for (double x = 4097.0; x < double(1u << 28); x *= 1.37)
    if (check_n(uint32_t(x))) return 1;
  if (check_pins()) return 1;
  if (check_phases()) return std::printf("FAILED phase truth table\n"), 1;
  std::printf("ok\n");
  return 0;
}
