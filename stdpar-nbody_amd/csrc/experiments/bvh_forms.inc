// K9 scheduling forms that are NOT in the shipped library (included by bvh.hip under -DNBODY_EXPERIMENTS only: `make experiments`).
// They make every body perform the same tests in the same order as the shipped forms (bitwise the same results) and were
// measured slower; the measurements are in profiles/ (r02/k9_modes.txt, r03/k9_row_sweep.txt) and DESIGN.md's appendix.
//   traversal mode 3 / 4: the sweep's step program as C++, scheduled by hipcc, with 1 / 2 bodies per lane (config 4: 8.9 / 12.2 ms
//                         against 6.6 for the ISA form);
//   traversal mode 6:     four independent 16-lane row sweeps per wave (16.1 ms).
#pragma once

template <typename T>
struct rec_sgprs;
template <>
struct rec_sgprs<double> {
  typedef uint32_t type __attribute__((ext_vector_type(16)));
  __device__ static __forceinline__ type load(const void* base, uint32_t off) {  // base, off wave-uniform
    type r;
    asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(r) : "s"(base), "s"(off));
    return r;
  }
};
template <>
struct rec_sgprs<float> {
  typedef uint32_t type __attribute__((ext_vector_type(8)));
  __device__ static __forceinline__ type load(const void* base, uint32_t off) {
    type r;
    asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(r) : "s"(base), "s"(off));
    return r;
  }
};
template <typename V>
__device__ __forceinline__ void rec_wait(V& v) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v));
}

// BPL bodies per lane: the wave sweeps the union of 64 * BPL consecutive (Hilbert-adjacent) bodies' walks.  The union
// grows slowly with the group (about 7.4k entries for 64 bodies, 8k for 128 at config 4) while the scalar half of a step —
// load, successors, position update: as many issue slots as the vector half — is paid once per step, and the BPL
// independent per-body chains give the wave instruction-level parallelism.
template <typename T, int D, int BPL, bool COUNT>
__global__ __launch_bounds__(64) void bvh_force_wave_kernel(const tree_rec<T>* __restrict__ node, T* __restrict__ a,
                                                            const T* __restrict__ x, T c, uint32_t sz, uint32_t first,
                                                            uint32_t count, T theta2, uint32_t nlevels,
                                                            uint32_t* __restrict__ counters, const uint32_t* __restrict__ items,
                                                            const uint32_t* __restrict__ nitems, uint32_t stride, uint32_t parts) {
  constexpr uint32_t DONE = 0xffffffffu;
  constexpr uint32_t RB   = uint32_t(sizeof(tree_rec<T>));  // 64 (f64) or 32 (f32) bytes per entry
  // work item of this block: with an item list, the XCD it runs on (block index mod 8) owns one list (bvh_items_kernel)
  uint32_t group = xcd_contiguous_block(blockIdx.x, gridDim.x), lane_lo = 0, lane_hi = 63;
  if (items) {
    const uint32_t xcd = blockIdx.x % 8u, slot = blockIdx.x / 8u;
    if (slot >= nitems[xcd]) return;
    const uint32_t it = items[xcd * stride + slot];
    group   = it & 0xfffffu;
    lane_lo = (it >> 20) & 63u;
    lane_hi = it >> 26;
  } else if (parts > 1u) {  // every group as `parts` equal lane ranges (small systems: k9_parts, bvh_plan.hpp)
    lane_lo = (group % parts) * (64u / parts);
    lane_hi = lane_lo + 64u / parts - 1u;
    group /= parts;
  }
  const uint32_t base = group * (64u * BPL) + threadIdx.x;
  const pair_consts<T> pc;
  T xs[BPL][D], acc[BPL][D];
  uint32_t key[BPL], bi[BPL];
  bool valid[BPL];
  // A lane's key keeps counting past the end (covered >= sz means finished: such keys compare above every live
  // one because `covered` sits in the high bits), so only lanes outside the shard need a sentinel.
#pragma unroll
  for (int b = 0; b < BPL; ++b) {
    const uint32_t local = base + 64u * b;
    valid[b]             = local < count && threadIdx.x >= lane_lo && threadIdx.x <= lane_hi;
    bi[b]                = first + (valid[b] ? local : 0u);
    key[b]               = valid[b] ? 0u : DONE;  // root: covered 0, level 0
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xs[b][k]  = x[uint64_t(bi[b]) * D + k];
      acc[b][k] = T(0);
    }
  }
  uint32_t c_nodes[BPL] = {}, c_leaf[BPL] = {}, c_mono[BPL] = {}, c_body[BPL] = {};

  // wave-uniform position of the sweep, kept incrementally in SGPRs: packed key, levels below, byte offset of the record
  // packed key, 32 << (levels below the entry), byte offset of the record
  uint32_t cur = 0, span = 32u << nlevels, off = 0;
  // cur >= (sz << 5): covered >= sz, every remaining key is >= cur: all lanes are finished.  One less, because an accepted
  // ROOT (theta > 0.58) is left by the ascend rule with covered + 2^nlevels and level - 1 = 31 after the borrow, which is
  // (sz << 5) - 1 when sz is a power of two; no live key has level 31.
  const uint32_t end_key = (sz << 5) - 1u;
#pragma unroll
  for (int b = 0; b < BPL; ++b)
#pragma unroll
    for (int k = 0; k < D; ++k) asm volatile("" : "+v"(xs[b][k]));  // the position loads complete here, not inside the loop

  while (cur < end_key) {
    auto raw = rec_sgprs<T>::load(node, off);  // wave-uniform address: one scalar load of the whole record
    // the two possible successors while the load is in flight
    // left child -> sibling (same level); right child -> parent + 1 (level - 1)   (src/bvh.h:272-281)
    // (an entry is a right child iff its level-order index is even; the root counts as one)
    const uint32_t right = ((off / RB) & 1u) ^ 1u;
    const uint32_t ka    = cur + span - right;  // covered + 2^(levels below), level - right
    const uint32_t kd    = cur + 1u;            // descend: same covered, level + 1  (src/bvh.h:283-286)
    const bool body      = span == 32u;         // (counters only: body records pass the opening test by construction)
    rec_wait(raw);
    const tree_rec<T> rc = __builtin_bit_cast(tree_rec<T>, raw);
    uint64_t m_reject_any = 0ull, waiting = 0ull;
#pragma unroll
    for (int b = 0; b < BPL; ++b) {
      T d[D];
#pragma unroll
      for (int k = 0; k < D; ++k) d[k] = xs[b][k] - rc.v[k];
      const T d2 = dist2_ref<T, D>(d);
      // a body is always taken (src/bvh.h:288-300), a node if it passes the opening test (src/bvh.h:306)
      T scaled;
      {
#pragma clang fp contract(off)
        scaled = theta2 * d2;
      }
      // the conditions as scalar masks from ballots of the two plain compares; lanes read them back for free
      const uint64_t m_active = __builtin_amdgcn_ballot_w64(key[b] == cur);
      const uint64_t m_approx = __builtin_amdgcn_ballot_w64(!(rc.v[D + 2] >= scaled));  // `<` for numbers; NaN accepts
      const uint64_t m_accept = m_active & m_approx;
      const uint64_t m_reject = m_active & ~m_approx;
      const bool accept       = __builtin_amdgcn_inverse_ballot_w64(m_accept);
      const bool reject       = __builtin_amdgcn_inverse_ballot_w64(m_reject);
      if (COUNT) {
        const bool active = __builtin_amdgcn_inverse_ballot_w64(m_active);
        const bool approx = __builtin_amdgcn_inverse_ballot_w64(m_approx);
        if (active) {
          const uint32_t cov = cur >> 5;
          if (body) {
            c_body[b] += (cov != bi[b]);
            c_leaf[b] += !(cov & 1u);  // one leaf visit per body pair, counted at its first body
          } else {
            ++c_nodes[b];
            c_mono[b] += approx;
          }
        }
      }
      if (m_accept != 0ull) tree_accumulate<T, D>(accept, m_accept, acc[b], d, d2, rc.v[D], pc);
      key[b] = accept ? ka : (reject ? kd : key[b]);
      m_reject_any |= m_reject;
      waiting |= __builtin_amdgcn_ballot_w64(key[b] < ka);
    }
    // Next position, branch-free in the common cases (every branch costs the wave an issue slot and a refetch).
    // A lane opened the node: its left child is the smallest key any lane can now hold.  Otherwise follow the ascend rule
    // (parent + 1 = idx / 2 for an even idx; sibling = idx + 1) — unless some lane waits at a smaller key: it jumped there
    // from a deeper subtree, to an entry below the one just accepted by the others (rare; found and decoded below).
    const uint32_t off_down = 2u * off + RB, off_up = right ? (off >> 1) : off + RB;
    const uint32_t sh_down = span >> 1, sh_up = span << right;
    uint64_t behind;
    // four scalar selects on one condition; written out because hipcc turns the equivalent C++ into a diamond of branches
    asm volatile("s_cmp_lg_u64 %[mr], 0\n\t"
                 "s_cselect_b32 %[cur], %[kd], %[ka]\n\t"
                 "s_cselect_b32 %[off], %[od], %[ou]\n\t"
                 "s_cselect_b32 %[sh], %[sd], %[su]\n\t"
                 "s_cselect_b64 %[bh], 0, %[wt]"
                 : [cur] "=&s"(cur), [off] "=&s"(off), [sh] "=&s"(span), [bh] "=&s"(behind)
                 : [mr] "s"(m_reject_any), [kd] "s"(kd), [ka] "s"(ka), [od] "s"(off_down), [ou] "s"(off_up), [sd] "s"(sh_down),
                   [su] "s"(sh_up), [wt] "s"(waiting)
                 : "scc");
    if (__builtin_expect(behind != 0ull, 0)) {
      uint32_t cand = ka;
      for (bool again = true; again;) {  // the smallest key any body of the wave holds
        again = false;
#pragma unroll
        for (int b = 0; b < BPL; ++b) {
          uint64_t m = __builtin_amdgcn_ballot_w64(key[b] < cand);
          while (m) {
            cand  = __builtin_amdgcn_readlane(key[b], __builtin_ctzll(m));
            m     = __builtin_amdgcn_ballot_w64(key[b] < cand);
            again = BPL > 1;
          }
        }
      }
      cur                  = cand;
      const uint32_t level = cand & 31u;
      const uint32_t shift = nlevels - level;
      span                 = 32u << shift;
      off                  = (((1u << level) - 1u) + ((cand >> 5) >> shift)) * RB;
    }
    cur = __builtin_amdgcn_readfirstlane(cur);  // wave-uniform by construction; keep it in an SGPR
  }
#pragma unroll
  for (int b = 0; b < BPL; ++b) {
    if (valid[b]) {
      const uint32_t local = base + 64u * b;
#pragma unroll
      for (int k = 0; k < D; ++k) a[uint64_t(local) * D + k] = c * acc[b][k];
      if (COUNT) {
        counters[uint64_t(bi[b]) * 4 + 0] = c_nodes[b];
        counters[uint64_t(bi[b]) * 4 + 1] = c_leaf[b];
        counters[uint64_t(bi[b]) * 4 + 2] = c_mono[b];
        counters[uint64_t(bi[b]) * 4 + 3] = c_body[b];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// K9, row sweeps: FOUR independent sweeps per wave, one per 16-lane row (traversal mode 6; an experiment that is kept because
// its measurement is: profiles/r03/k9_row_sweep.txt).  The union of 16 Hilbert-adjacent walks is 23 % shorter than the union of
// 64 (5.7k against 7.4k entries at config 4), but a row's position is no longer wave-uniform: the record comes through the
// vector memory path (one address per row), the position lives in VGPRs, the row-wide conditions are cut out of ballots per
// lane, and every scalar operation of the wave sweep's bookkeeping becomes a vector one.  Same tests in the same order per
// body: bitwise the results of every other form.
// ------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(64) void bvh_force_row_kernel(const tree_rec<T>* __restrict__ node, T* __restrict__ a,
                                                           const T* __restrict__ x, T c, uint32_t sz, uint32_t first,
                                                           uint32_t count, T theta2, uint32_t nlevels) {
  const uint32_t group = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const uint32_t local = group * 64u + threadIdx.x;
  const bool valid     = local < count;
  const uint32_t bi    = first + (valid ? local : 0u);
  const pair_consts<T> pc;
  T xs[D], acc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    xs[k]  = x[uint64_t(bi) * D + k];
    acc[k] = T(0);
  }
  uint32_t key = valid ? 0u : 0xffffffffu;
  // the row's position, the same value in its 16 lanes: packed key, 32 << (levels below), level-order index of the entry
  uint32_t cur = 0, span = 32u << nlevels, idx = 0;
  const uint32_t end_key = (sz << 5) - 1u;  // see bvh_force_wave_kernel
  const uint32_t rshift  = threadIdx.x & 48u;
  uint32_t budget        = (4u << nlevels) + 64u;  // a sweep visits every tree entry at most once: an exit every wave reaches
  while (__builtin_amdgcn_ballot_w64(cur < end_key) != 0ull && budget-- != 0u) {
    const bool live      = cur < end_key;
    const tree_rec<T> rc = node[live ? idx : 0u];
    const uint32_t right = (idx & 1u) ^ 1u;     // an entry is a right child iff its level-order index is even (root included)
    const uint32_t ka = cur + span - right, kd = cur + 1u;
    T d[D];
#pragma unroll
    for (int k = 0; k < D; ++k) d[k] = xs[k] - rc.v[k];
    const T d2 = dist2_ref<T, D>(d);
    T scaled;
    {
#pragma clang fp contract(off)
      scaled = theta2 * d2;
    }
    const bool active = live && key == cur;
    const bool approx = !(rc.v[D + 2] >= scaled);
    const bool accept = active && approx, reject = active && !approx;
    const uint64_t m_accept = __builtin_amdgcn_ballot_w64(accept);
    if (m_accept != 0ull) tree_accumulate<T, D>(accept, m_accept, acc, d, d2, rc.v[D], pc);
    key = accept ? ka : (reject ? kd : key);
    const bool row_reject = ((__builtin_amdgcn_ballot_w64(reject) >> rshift) & 0xffffull) != 0ull;
    const bool row_wait   = ((__builtin_amdgcn_ballot_w64(live && key < ka) >> rshift) & 0xffffull) != 0ull;
    uint32_t mn = key;  // smallest key of the row (needed only when the row is behind; rows take their branches together)
    if (__builtin_amdgcn_ballot_w64(live && !row_reject && row_wait) != 0ull) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const uint32_t other = uint32_t(__shfl_xor(int(mn), o, 16));
        mn                   = other < mn ? other : mn;
      }
    }
    if (live) {
      if (row_reject) {  // some lane of the row opened the entry: its left child is the smallest key the row can hold
        cur = kd;
        idx = 2u * idx + 1u;
        span >>= 1;
      } else if (!row_wait) {  // ascend rule: left child -> sibling, right child -> parent + 1
        cur = ka;
        idx = right ? (idx >> 1) : idx + 1u;
        span <<= right;
      } else {  // a lane waits below the entry just left
        cur                  = mn;
        const uint32_t level = mn & 31u, shift = nlevels - level;
        span                 = 32u << shift;
        idx                  = ((1u << level) - 1u) + ((mn >> 5) >> shift);
      }
    }
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < D; ++k) a[uint64_t(local) * D + k] = c * acc[k];
  }
}

// ------------------------------------------------------------------------------------------------
// host side: the sweep's timeline, and the launch of the forms above from force_run's plan
// ------------------------------------------------------------------------------------------------
// tools/k9_timeline.py: per work item of a sweep launch (start, end) in 100 MHz ticks and the item, three words per launch block
__device__ unsigned long long* g_k9_timeline = nullptr;
static unsigned long long* g_k9_timeline_host = nullptr;  // the same buffer, for nbody_exp_k9_timeline
static size_t g_k9_timeline_words = 0, g_k9_timeline_cap = 0;

static int k9_timeline_prepare(uint32_t grid, hipStream_t st) {
  if (g_k9_timeline_cap < 3 * size_t(grid)) {
    if (g_k9_timeline_host) (void)hipFree(g_k9_timeline_host);
    g_k9_timeline_host = nullptr;
    g_k9_timeline_cap  = 3 * size_t(grid);
    NB_HIP(hipMalloc(&g_k9_timeline_host, g_k9_timeline_cap * sizeof(unsigned long long)));
    NB_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_k9_timeline), &g_k9_timeline_host, sizeof g_k9_timeline_host));
  }
  NB_HIP(hipMemsetAsync(g_k9_timeline_host, 0, g_k9_timeline_cap * sizeof(unsigned long long), st));
  g_k9_timeline_words = 3 * size_t(grid);
  return NBODY_OK;
}

// experiments library only (not in nbody_hip.h): the timeline of the last sweep launch made with NBODY_K9_TIMELINE=1
extern "C" long long nbody_exp_k9_timeline(unsigned long long* out, size_t max_words) {
  if (!g_k9_timeline_words || max_words < g_k9_timeline_words) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  if (hipMemcpy(out, g_k9_timeline_host, g_k9_timeline_words * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -3;
  return (long long)g_k9_timeline_words;
}

// K9's switches of this build (tools/README.md), all read here; the shipped library's k9_read_overrides returns the defaults.
static k9_overrides k9_read_overrides() {
  k9_overrides o;
  if (const char* e = experiment_env("NBODY_K9_MODE")) o.mode = atoi(e);
  if (const char* e = experiment_env("NBODY_K9_ORDER")) o.plain_order = e[0] == '0';
  if (const char* e = experiment_env("NBODY_K9_PARTS")) {
    const uint32_t p = uint32_t(atoi(e));
    o.parts          = p == 2u || p == 4u || p == 8u || p == 16u ? p : 1u;
  }
  if (const char* e = experiment_env("NBODY_K9_SPLIT")) o.split_den = uint32_t(atoi(e)) ? uint32_t(atoi(e)) : 16u;
  if (const char* e = experiment_env("NBODY_K9_LDS")) o.lds_bytes = uint32_t(atoi(e));
  if (const char* e = experiment_env("NBODY_K9_TIMELINE")) o.timeline = e[0] == '1';
  return o;
}

// force_run's one call into this file.  *done: the plan's form was one of the above and has been launched.  The shipped sweep is
// force_run's own launch; with NBODY_K9_TIMELINE=1 its buffer is made ready here.
template <typename T, int D>
static int k9_experiment_launch(const nbody_bvh* t, const nbody_state* s, const k9_plan& p, const k9_overrides& o, T th2,
                                const uint32_t* items, const uint32_t* nitems, hipStream_t st, bool* done) {
  auto* node = static_cast<const tree_rec<T>*>(t->node);
  T* a       = static_cast<T*>(s->a);
  const T *x = static_cast<const T*>(s->x), c = static_cast<T>(s->c);
  const auto wave = [&](auto plain, auto counting) {
    hipLaunchKernelGGL(t->counters_on ? counting : plain, dim3(p.grid), dim3(p.threads), p.lds_bytes, st, node, a, x, c, s->sz, s->first,
                       s->count, th2, t->nlevels, t->counters, items, nitems, p.stride, p.parts);
  };
  switch (p.form) {
    case k9_form::sweep: return o.timeline ? k9_timeline_prepare(p.grid, st) : NBODY_OK;
    case k9_form::compiled_sweep: wave(bvh_force_wave_kernel<T, D, 1, false>, bvh_force_wave_kernel<T, D, 1, true>); break;
    case k9_form::compiled_sweep_2: wave(bvh_force_wave_kernel<T, D, 2, false>, bvh_force_wave_kernel<T, D, 2, true>); break;
    case k9_form::row_sweeps:
      if (t->counters_on) {  // (the plan has refused nlevels > 26 with the same words)
        set_error(kK9RowsRefusal);
        return NBODY_ERR_ARG;
      }
      hipLaunchKernelGGL((bvh_force_row_kernel<T, D>), dim3(p.grid), dim3(p.threads), 0, st, node, a, x, c, s->sz, s->first, s->count, th2,
                         t->nlevels);
      break;
    default: return NBODY_OK;
  }
  *done = true;
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}
