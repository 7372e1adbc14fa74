// Host plan of the octree (csrc/octree.hip): what a tree of n bodies allocates, which kernels each phase launches with which grids,
// which form the walk takes, and which phase calls have run.  Host arithmetic only, no kernel and no HIP call, so that
// tools/octree_plan_check.cpp can sweep its invariants and pin its routes without a device.  nbody_octree_create_on fills an ot_request
// and calls plan_octree; nbody_octree_set_build / set_walk / set_step_budget plan again; the phase runners launch what the ot_plan says.
// The shard window's `count` is the only input a call adds (ot_walk_grid).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/nbody_hip.h"

namespace nbody {

// ---- launch shapes the decisions below depend on (the kernels of octree.hip use the same names) ----
constexpr int kOB              = 256;   // bounds, keys, scatter, per-level multipoles and quadrupoles
constexpr int kOBuild          = 1024;  // ot_build_level_kernel
constexpr uint32_t kSmallN     = 1024;  // up to here one block finds the bounds, and one block inserts (ot_insert_small_kernel)
constexpr int kSmallB          = 1024;  // its threads: one (key, body) pair each
constexpr int kLcpB            = 1024;  // positions per block of ot_lcp_kernel
constexpr int kLcpBuildB       = 256;   // ot_build_lcp_kernel: lane groups are independent, small blocks give their slots back early
constexpr int kMpChunk         = 512;   // ot_multipole_chunks_kernel: ranks (= threads) per block (512: a double 3D cell keeps 2^D x 4 values in registers)
constexpr int kMpCrown         = 512;   // ot_multipole_crown_kernel: threads, and cells it finishes out of registers and LDS
constexpr uint32_t kMpMaxBlocks = 8192;  // blocks of the previous round a round can compact (32 KB of LDS): trees of up to 4.2 * 10^6 cells
constexpr uint32_t kSmallChunks = (kSmallN + 1 + kMpChunk - 1) / kMpChunk;  // chunks of the largest tree ot_insert_small_kernel builds
constexpr int kOC              = 1024;  // ot_owned_*_kernel: the shard window's list
template <int D>
constexpr int kMaxLevels = D == 3 ? 21 : 32;  // key depth
template <int D>
constexpr int kOtNQ = D == 3 ? 6 : 3;  // values of Q: xx, xy, xz, yy, yz, zz / xx, xy, yy
template <int D>
constexpr int kOtQS = kOtNQ<D> + D;  // the quadrupole array's stride per node: Q, then the cell's residual dipole
inline int ot_max_levels(int dim) { return dim == 3 ? kMaxLevels<3> : kMaxLevels<2>; }
// sizeof(ot_group<T, D>): the 2^D nodes of a sibling group in 16-byte pieces, 64-byte aligned (octree.hip asserts the four values)
constexpr size_t ot_group_bytes(uint32_t elem, int dim) { return elem == 4 ? (dim == 3 ? 192 : 128) : (dim == 3 ? 320 : 128); }
inline uint32_t ot_small_mp_threads(uint32_t elem) { return elem == 4 ? 1024u : uint32_t(kMpChunk); }  // kSmallMpThreads<T, D>

// Cells level `level` can hold: 2^(D level) of them, and no more than half the bodies (+ 1) — a cell has >= 2.
inline uint64_t ot_level_cap(int dim, uint32_t n, int level) {
  const uint64_t most = uint64_t(n / 2 + 1);
  const int bits      = dim * level;
  return bits < 40 && (uint64_t(1) << bits) < most ? uint64_t(1) << bits : most;
}

// ---- the request ----
// What the -DNBODY_EXPERIMENTS build contributes (experiments/octree_forms.inc); the shipped build leaves it as it stands.
struct ot_overrides {
  bool compiled_walk = false;  // NBODY_OT_FORM=1: the compiler-scheduled walk where auto would take the ISA round
  int depth_hint     = 64;     // build form 4: levels launched one by one (the rest share one launch); from the last nbody_octree_info
  uint32_t ncu       = 1;      // compute units of the device: the all-level kernels of forms 2 and 4 launch at most one block per CU
};
struct ot_request {
  uint32_t elem = 8;  // sizeof(T)
  int dim       = 3;
  uint32_t n    = 0;
  size_t group_bytes = 0;  // sizeof(ot_group<T, D>)
  size_t sort_words  = 0;  // radix_sort_scratch_words(n)
  int build = 0;  // nbody_octree_set_build: 0 auto (= 3), 1 one launch per level, 3 one pass over the sorted keys (experiments: 2 all levels in
                  // one launch behind grid barriers, 4 one launch per level the last tree used and one for the rest)
  int walk  = 0;  // nbody_octree_set_walk: 0 auto, 1 compiler-scheduled kernel, 2 the visit round as ISA
  uint32_t step_budget = 0;  // nbody_octree_set_step_budget: visit rounds a body may make; 0 = the node pool size
  ot_overrides overrides;
};

// ---- the plan ----
// Every buffer of the handle, in the order nbody_octree_create_on allocates them; the last two are allocated by the first
// nbody_octree_enable_counters / nbody_octree_compute_quadrupoles.
enum ot_buffer {
  kBufRoot, kBufPartials, kBufKeys0, kBufKeys1, kBufIdx0, kBufIdx1, kBufHist, kBufRootrec, kBufGroups, kBufCells, kBufLvlCount, kBufTops,
  kBufLcp, kBufPlocal, kBufBsum, kBufBhist, kBufRankpos, kBufLater, kBufLaterMask, kBufLater2, kBufLater2Mask, kOtCreateBuffers,
  kBufCounters = kOtCreateBuffers, kBufQuad, kOtBuffers
};
// The multipole pass (nbody_octree_compute_tree).  One-pass build: one block for the whole tree where that is one chunk's work — a
// single chunk of kMpChunk ranks, or in float up to kSmallChunks chunks, chunk after chunk and then the crown (double trees of two or
// three chunks: their chunks side by side on two CUs + the crown are 22 us, one after the other in one block 30, n = 1000); rank
// chunks, then the cells that span chunk boundaries in one block (the crown); beyond kMpCrown chunks a round of blocks over those
// cells first; beyond kMpMaxBlocks chunks (4.2 * 10^6 bodies) one launch per level over all ranks.  Build form 1: one launch per level
// over that level's cell list.
enum class ot_mp_route { small_block, chunks_crown, chunks_round_crown, ranks_per_level, levels };
struct ot_plan {
  // sizes
  int maxl = 0;  // kMaxLevels<dim>
  uint32_t capacity = 0, max_cells = 0;  // nodes (System::max_tree_node_size, src/system.h:30); sibling groups = cells
  size_t bytes[kOtBuffers] = {};
  // bounds: one block up to kSmallN bodies, else bounds_blocks partial blocks and one final block
  bool small_bounds      = false;
  uint32_t bounds_blocks = 0;
  // build
  bool one_pass     = true;   // form 3, which 0 = auto selects
  bool small_insert = false;  // ot_insert_small_kernel: one block does everything up to the cells
  uint32_t keys_grid = 0, lcp_blocks = 0, scatter_grid = 0, build_lcp_grid = 0;  // lcp_blocks: `nblk`, positions 0 ... n
  int own_levels = 0;  // form 1: levels with a launch of their own (all of them; the experiments' forms 2 and 4: fewer)
  uint32_t build_level_grid[32] = {}, level_grid[32] = {};  // ot_build_level_kernel; the per-level multipole and quadrupole kernels
  uint32_t all_levels_build_grid = 0, all_levels_mp_grid = 0;  // experiments: the one launch of the levels from own_levels on
  // multipoles; quadrupoles take ranks_grid per level after a one-pass build and level_grid otherwise
  ot_mp_route route = ot_mp_route::small_block;
  uint32_t chunks = 0, small_threads = 0, round_blocks = 0, ranks_grid = 0;
  bool crown_reads_later2 = false;  // the crown reads the round's (later2, later2_mask) pair, not the chunks' (later, later_mask)
  // walk
  bool isa = false;  // the plain force walk takes the visit round written as ISA (the other kinds exist compiler-scheduled only)
  const char* mono_refusal  = nullptr;  // why the plain force walk is refused, or NULL
  const char* other_refusal = nullptr;  // why every other walk is refused, or NULL: a format that takes the walk's name
  uint32_t budget = 0;  // visit rounds a body may make: a well-formed tree is left after < capacity
  bool budget_set = false;
};
constexpr const char* kOtIsaRefusal = "octree walk: the ISA visit round needs the tree within 24-bit group numbers and 32-bit group offsets";
constexpr const char* kOtCompiledOnlyRefusal =
    "octree walk: the %s walk exists in the compiler-scheduled form only (walk form 1 or 0 = auto), not as the ISA "
    "visit round set by nbody_octree_set_walk(t, 2)";

// one block per wave of 2^(6 - D) bodies: 2^D lanes examine a group side by side
inline uint32_t ot_walk_grid(int dim, uint32_t count) { return (count + (64u >> dim) - 1u) / (64u >> dim); }
// blocks of ot_owned_*_kernel over the n sorted bodies; their counts use the sort's scratch
inline uint32_t ot_owned_blocks(uint32_t n) { return (n + kOC - 1) / kOC; }

inline ot_plan plan_octree(const ot_request& r) {
  ot_plan p;
  const uint32_t n = r.n, nch = 1u << r.dim;
  const size_t N = n;
  p.maxl = ot_max_levels(r.dim);
  const size_t maxl = size_t(p.maxl);
  // sizes
  const uint64_t cap = uint64_t(nch) * n < 1000 ? 1000 : uint64_t(nch) * n;  // System::max_tree_node_size (src/system.h:30)
  p.capacity         = uint32_t(cap);
  p.max_cells        = p.capacity / nch + 1;
  p.bounds_blocks    = uint32_t((uint64_t(n) * r.dim + kOB * 8 - 1) / (kOB * 8));
  if (p.bounds_blocks > 1024) p.bounds_blocks = 1024;
  p.chunks          = (p.max_cells + kMpChunk - 1) / kMpChunk;
  p.round_blocks    = (p.chunks * uint32_t(p.maxl) + kMpCrown - 1) / kMpCrown;
  p.lcp_blocks      = n / kLcpB + 1;
  size_t* z         = p.bytes;
  z[kBufRoot]       = r.elem * size_t(r.dim + 1);  // root_x (D), root_side_length
  z[kBufPartials]   = r.elem * 2 * size_t(p.bounds_blocks);
  z[kBufKeys0] = z[kBufKeys1] = sizeof(uint64_t) * N;
  z[kBufIdx0] = z[kBufIdx1] = sizeof(uint32_t) * N;
  z[kBufHist]       = sizeof(uint32_t) * r.sort_words;
  z[kBufRootrec]    = 64;  // ot_node<T>
  z[kBufGroups]     = r.group_bytes * size_t(p.max_cells);
  z[kBufCells]      = 16 * size_t(p.max_cells);  // ot_cell
  z[kBufLvlCount]   = sizeof(uint32_t) * (maxl + 8);  // level counts, deep groups, flags, two grid-barrier counters, deep-list cursor, crown count
  z[kBufTops]       = 16 * (N / 2 + 2);  // ot_cell: the cells at the key depth hold >= 2 bodies each
  z[kBufLcp]        = N + 2;              // int8: positions 0 ... n
  z[kBufPlocal]     = sizeof(uint32_t) * (N + 1);
  z[kBufBsum]       = sizeof(uint32_t) * p.lcp_blocks;
  z[kBufBhist]      = sizeof(uint32_t) * p.lcp_blocks * (maxl + 1);
  z[kBufRankpos]    = sizeof(uint32_t) * size_t(p.max_cells);
  z[kBufLater]      = sizeof(uint32_t) * size_t(p.chunks) * maxl;  // slot (chunk, level)
  z[kBufLaterMask]  = sizeof(uint32_t) * size_t(p.chunks);
  z[kBufLater2]     = sizeof(uint32_t) * size_t(p.round_blocks) * maxl;  // slot (block of the round, level)
  z[kBufLater2Mask] = sizeof(uint32_t) * size_t(p.round_blocks);
  z[kBufCounters]   = sizeof(uint32_t) * 2 * N;
  z[kBufQuad]       = r.elem * size_t((r.dim == 3 ? kOtQS<3> : kOtQS<2>)) * (size_t(p.max_cells) * nch + 1);  // every node the groups hold, and the root
  // bounds, build
  p.small_bounds   = n <= kSmallN;
  p.one_pass       = r.build == 0 || r.build == 3;
  p.small_insert   = n <= kSmallN && p.one_pass;
  p.keys_grid      = (n + kOB - 1) / kOB;
  p.scatter_grid   = (n + kOB - 1) / kOB;
  p.build_lcp_grid = uint32_t((uint64_t(p.max_cells) * nch + kLcpBuildB - 1) / kLcpBuildB);
  p.ranks_grid     = (p.max_cells + kOB - 1) / kOB;
  p.own_levels     = r.build == 2 ? 0 : (r.overrides.depth_hint < p.maxl ? r.overrides.depth_hint : p.maxl);
  for (int l = 0; l < p.maxl; ++l) {
    const uint64_t cap_l  = ot_level_cap(r.dim, n, l);
    p.build_level_grid[l] = uint32_t((cap_l * nch + kOBuild - 1) / kOBuild);
    p.level_grid[l]       = uint32_t((cap_l + kOB - 1) / kOB);
  }
  {  // at most one block per CU, and no more blocks than the widest level can use
    const uint64_t widest   = ot_level_cap(r.dim, n, p.maxl - 1);  // the deepest key level is bounded by the bodies alone
    p.all_levels_build_grid = uint32_t((widest * nch + kOBuild - 1) / kOBuild);
    p.all_levels_mp_grid    = uint32_t((widest + kOB - 1) / kOB);
    if (p.all_levels_build_grid > r.overrides.ncu) p.all_levels_build_grid = r.overrides.ncu;
    if (p.all_levels_mp_grid > r.overrides.ncu) p.all_levels_mp_grid = r.overrides.ncu;
  }
  // multipoles (decided by the size the tree was created for: the launches are recorded)
  p.small_threads = ot_small_mp_threads(r.elem);
  if (!p.one_pass) p.route = ot_mp_route::levels;
  else if (p.chunks > kMpMaxBlocks) p.route = ot_mp_route::ranks_per_level;
  else if (p.chunks == 1 || (r.elem == 4 && p.chunks <= kSmallChunks)) p.route = ot_mp_route::small_block;
  else p.route = p.chunks > uint32_t(kMpCrown) ? ot_mp_route::chunks_round_crown : ot_mp_route::chunks_crown;
  p.crown_reads_later2 = p.route == ot_mp_route::chunks_round_crown;
  // walk: the visit round as ISA (2D and 3D, both precisions) while 24-bit group numbers times the group size stay inside 32-bit
  // offsets; nbody_octree_set_walk(t, 1) keeps the compiler-scheduled kernel (tests compare the two bitwise)
  p.isa = r.walk != 1 && !r.overrides.compiled_walk && uint64_t(p.max_cells) * r.group_bytes < (1ull << 32) && p.max_cells < (1u << 24);
  if (r.walk == 2) p.other_refusal = kOtCompiledOnlyRefusal;
  if (r.walk == 2 && !p.isa) p.mono_refusal = kOtIsaRefusal;
  p.budget_set = r.step_budget != 0;
  p.budget     = r.step_budget ? r.step_budget : p.capacity;
  return p;
}

// ---- phases ----
// Host-side phase tracking in call order: a recorded step replays its calls in the order they were recorded, so the checks hold for
// graphs too.  Every node the build allocates is fully rewritten by it, so a clear resets nothing else.
enum class ot_phase { bounds, inserted, tree, quadrupoles };
struct ot_phases {
  bool have_bounds = false, inserted = false, have_tree = false;
  bool have_quad   = false;  // nbody_octree_compute_quadrupoles ran after the latest clear / insert / compute_tree / set_build
  void bounds_done() { have_bounds = true; }
  void insert_done() { inserted = true, have_quad = false; }
  void insert_failed() { have_quad = false; }  // the tree is no longer the one the quadrupoles describe
  void tree_done() { have_tree = true, have_quad = false; }
  void tree_failed() { have_quad = false; }
  void quadrupoles_done() { have_quad = true; }
  void cleared() { inserted = have_tree = have_quad = false; }
  // the forms lay the cell list out differently: a tree inserted by one is not the other's to finish (insert again after a change)
  void build_form_changed() { cleared(); }
  bool missing(ot_phase p) const {
    return !(p == ot_phase::bounds ? have_bounds : p == ot_phase::inserted ? inserted : p == ot_phase::tree ? have_tree : have_quad);
  }
};
// "<call> before <the call that makes the phase>": a format that takes the refused call's name
inline const char* ot_phase_refusal(ot_phase p) {
  switch (p) {
    case ot_phase::bounds: return "%s before nbody_octree_compute_bounds";
    case ot_phase::inserted: return "%s before nbody_octree_insert";
    case ot_phase::tree: return "%s before nbody_octree_compute_tree";
    default:
      return "%s before nbody_octree_compute_quadrupoles (which must follow the latest clear / insert / compute_tree / set_build)";
  }
}

}  // namespace nbody
