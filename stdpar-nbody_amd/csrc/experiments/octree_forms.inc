// Octree build forms that are NOT in the shipped library (included by octree.hip under -DNBODY_EXPERIMENTS only: `make experiments`):
//   build form 2: every level of the breadth-first build / the multipole pass in ONE launch behind grid barriers;
//   build form 4: one launch per level the last tree used, one barrier launch for the rest.
// Same cells, monopoles, forces and counters bit for bit; measured slower on MI355X (an agent-scope barrier writes back and
// invalidates the per-XCD L2s, ~12 us against 4.6 us for a dependent launch: N = 10^5 0.82 against 0.35 ms per step,
// profiles/r04/step_graph.txt).  Included three times: OT_FORMS_PART 1 = the barrier, before the level body; 2 = the kernels, after it;
// 3 = the host side (what the plan is told, the two all-level launches, nbody_octree_info's part), behind the handle.
#if OT_FORMS_PART == 1
// Grid-wide barrier of a kernel whose blocks are all resident (one block per CU at most: ot_grid_blocks).  Every wave reaches an
// exit: a block that has waited kBarrierSpins polls (seconds; e.g. the GPU is shared and its peers never got a slot) raises
// kFlagBarrier, which nbody_octree_info reports, and the kernel's level loop ends on every block at its next check.
constexpr uint32_t kBarrierSpins = 4u << 20;
constexpr uint32_t kFlagBarrier  = 16u;  // beside kFlagDepth ... kFlagWalk in the tree's flags word
__device__ __forceinline__ bool ot_grid_barrier(uint32_t* counter, uint32_t& epoch, uint32_t* flags) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();  // release: this block's writes of the level before the arrival
    const uint32_t target = (epoch + 1u) * gridDim.x;
    atomicAdd(counter, 1u);
    uint32_t spins = 0;
    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > kBarrierSpins) {
        atomicOr(flags, kFlagBarrier);
        break;
      }
    }
    __threadfence();  // acquire: the other blocks' writes (invalidates this CU's vector L1)
  }
  ++epoch;
  __syncthreads();
  return (__hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kFlagBarrier) == 0u;
}
__device__ __forceinline__ uint32_t ot_count(const uint32_t* lvl_count, int level) {  // written by other blocks of this kernel
  return __hip_atomic_load(lvl_count + level, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#elif OT_FORMS_PART == 3
// ---- host side: octree.hip's hooks, behind struct nbody_octree and ot_replan -------------------------------------------------------
// The plan (octree_plan.hpp) takes this build's contributions as t->exp: own_levels = 0 for form 2 and the depth hint for form 4, the
// all-level grids capped at one block per CU, and the compiler-scheduled walk for NBODY_OT_FORM=1 (read when the tree is created).
static int ot_check_build_form(nbody_octree* t, int mode) {
  NB_ARG(mode >= 0 && mode <= 4,
         "build form must be 0 (auto), 1 (one launch per level), 2 (all levels in one launch), 3 (one pass over the sorted keys) or 4 "
         "(one launch per level the last tree used, one for the rest), got %d", mode);
  if (mode != 4) t->exp.depth_hint = 64;  // 1: every level its own launch, whatever earlier trees looked like
  return NBODY_OK;
}

static hipError_t ot_exp_create(nbody_octree* t) {
  const char* fe       = experiment_env("NBODY_OT_FORM");
  t->exp.compiled_walk = fe && fe[0] == '1';
  hipDeviceProp_t prop;
  const hipError_t e = hipGetDeviceProperties(&prop, t->device);
  t->exp.ncu         = e == hipSuccess && prop.multiProcessorCount > 0 ? uint32_t(prop.multiProcessorCount) : 1u;
  return e;
}

// nbody_octree_info, between the reports of the node pool and of the walks: the barrier's flag, and form 4's depth hint from a tree
// that raised no flag
static int ot_exp_info(nbody_octree* t, uint32_t flags, const uint32_t* lv) {
  if (flags & kFlagBarrier) {
    set_error("octree build: a grid barrier of the all-level kernels timed out (the blocks of one launch were not all running "
              "within seconds: is the GPU shared?); nbody_octree_set_build(t, 1) builds with one launch per level");
    return NBODY_ERR_STATE;
  }
  if (t->build == 4 && !(flags & (kFlagStack | kFlagWalk))) {
    const int maxl = t->plan.maxl;
    int deepest    = -1;
    for (int l = 0; l < maxl; ++l)
      if (lv[l] != 0) deepest = l;
    t->exp.depth_hint = deepest + 3 < maxl ? deepest + 3 : maxl;  // the levels the next builds launch one by one
    ot_replan(t);
  }
  return NBODY_OK;
}

// Levels [0, own_levels) get a launch each; the levels behind them — empty unless the tree has grown deeper than the last
// nbody_octree_info saw it (+ 2) — share ONE launch that walks them with a grid barrier and normally returns at once.  (All levels
// behind grid barriers, nbody_octree_set_build(t, 2), is slower on this chip: an agent-scope barrier has to write back and
// invalidate the per-XCD L2s and costs ~12 us, a dependent launch 4.6 us — N = 10^5: 0.87 against 0.55 ms per step.)
template <typename T, int D>
static int ot_exp_build_rest(nbody_octree* t, const nbody_state* s, hipStream_t st) {
  const ot_plan& p = t->plan;
  if (p.own_levels >= kMaxLevels<D>) return NBODY_OK;
  const int fin = t->sorted_buf;
  hipLaunchKernelGGL((ot_build_all_levels_kernel<T, D>), dim3(p.all_levels_build_grid), dim3(kOBuild), 0, st, t->keys[fin], t->idx[fin],
                     static_cast<const T*>(s->m), static_cast<const T*>(s->x), ot_view<T, D>(t), t->cells, t->lvl_count, ot_flags(t),
                     p.capacity, p.max_cells, p.own_levels);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}
// the levels below own_levels, deepest first, in one launch, before the launches of the levels above them
template <typename T, int D>
static int ot_exp_multipole_rest(nbody_octree* t, hipStream_t st) {
  const ot_plan& p = t->plan;
  if (p.own_levels >= kMaxLevels<D>) return NBODY_OK;
  hipLaunchKernelGGL((ot_multipole_all_levels_kernel<T, D>), dim3(p.all_levels_mp_grid), dim3(kOB), 0, st, ot_view<T, D>(t), t->cells,
                     t->lvl_count, t->lvl_count + (kMaxLevels<D> + 4), t->lvl_count + (kMaxLevels<D> + 2), p.own_levels, p.max_cells);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// wall_clock64() stamps (100 MHz) of the last ot_insert_small_kernel launch on the current device: entry, keys, sort, numbering,
// cells, deep cells (tools/time_small_insert_phases.py); C linkage: the name is the same inside the namespace
extern "C" int nbody_exp_octree_small_stamps(uint64_t* out8) {
  NB_HIP(hipDeviceSynchronize());
  NB_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(ot_small_stamps), sizeof(uint64_t) * 8));
  return NBODY_OK;
}

#else
// All levels in ONE launch: the step loop of a small system is bound by its ~75 dependent launches (4.6 us each inside a
// recorded step: half of the octree step at N = 10^5).  A grid of at most one 1024-thread block per CU walks the levels with a
// grid barrier between them and stops at the first level without cells.
template <typename T, int D>
__global__ __launch_bounds__(kOBuild) void ot_build_all_levels_kernel(const uint64_t* __restrict__ skeys,
                                                                      const uint32_t* __restrict__ sidx, const T* __restrict__ m,
                                                                      const T* __restrict__ x, ot_tree<T, D> tree, ot_cell* cells,
                                                                      uint32_t* lvl_count, uint32_t* flags, uint32_t capacity,
                                                                      uint32_t max_cells, int first_level) {
  constexpr uint32_t NCH = 1u << D;
  uint32_t* counter = lvl_count + (kMaxLevels<D> + 3);
  uint32_t epoch = 0, base = 0;
  for (int j = 0; j < first_level; ++j) base += ot_count(lvl_count, j);  // levels built by earlier launches
  for (int level = first_level; level < kMaxLevels<D>; ++level) {
    const uint32_t count = ot_count(lvl_count, level);  // final: every block has passed the barrier behind level - 1
    if (count == 0) break;                              // (the same value on every block: they leave together)
    for (uint32_t vb = blockIdx.x; vb * (kOBuild / NCH) < count; vb += gridDim.x)
      ot_build_level_body<T, D>(level, vb, count, base, skeys, sidx, m, x, tree, cells, lvl_count, flags, capacity, max_cells);
    base += count;
    if (!ot_grid_barrier(counter, epoch, flags)) break;
  }
}

// All levels, deepest first, in ONE launch with a grid barrier between non-empty levels (see ot_build_all_levels_kernel).  The
// cell lists and level counts are final here (the build is an earlier launch); only the tree's monopoles change.
template <typename T, int D>
__global__ __launch_bounds__(kOB) void ot_multipole_all_levels_kernel(ot_tree<T, D> tree, const ot_cell* __restrict__ cells,
                                                                      const uint32_t* __restrict__ lvl_count, uint32_t* counter,
                                                                      uint32_t* flags, int lowest_level, uint32_t max_cells) {
  uint32_t cnt[kMaxLevels<D>], total = 0;
#pragma unroll
  for (int l = 0; l < kMaxLevels<D>; ++l) {
    cnt[l] = lvl_count[l];
    total += cnt[l];
  }
  uint32_t epoch = 0, base = total;
  for (int l = kMaxLevels<D> - 1; l >= lowest_level; --l) {
    const uint32_t count = cnt[l];
    if (count == 0) continue;
    base -= count;
    for (uint32_t k = blockIdx.x * kOB + threadIdx.x; k < count && base + k < max_cells; k += gridDim.x * kOB)
      ot_multipole_cell<T, D>(tree, cells[base + k].node);
    if (l > lowest_level && !ot_grid_barrier(counter, epoch, flags)) break;
  }
}

#endif
