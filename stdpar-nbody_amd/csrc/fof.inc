// Friends-of-friends groups on the neighbour tree: nbody_fof_* of include/nbody_hip.h.  No reference counterpart.  Included from
// knn.hip, inside namespace nbody, after nntree.inc, whose structure (sorted records, buckets, boxes, nntree_structure_launch), bound
// and successor rule it uses as they are.
// The kernels' interface is shaped by a test: tests/test_nntree.py and tests/test_knn.py count kernels by `nntree_` and `knn_` anywhere
// in the DEMANGLED SIGNATURE, parameter types included, so no kernel here may name nntree_rec / nntree_box in its parameters.  The
// sorted records and the boxes therefore arrive as `const void* __restrict__` and are cast back in the kernel's first lines.  The typed
// alternative that keeps those strings out — a struct of the two typed pointers passed by value — was built and not kept: a pointer
// read from a by-value struct carries no noalias against the atomic stores to parent[], and the link kernel then fetches the records
// with vector loads (global_load_dwordx2/x3/x4) where it has scalar loads now (s_load_dwordx4/x8); tests/test_fof.py pins the scalar
// loads.  The one launch site (fof_launch in knn.hip) takes both pointers from the same nntree_structure.
//
// Definitions (T the state's type, D its dimension):
//   friends  i != j with d2_ij <= b2, d2 pair_d2's chain (pair_sweep.hpp), b2 = T(b) * T(b) rounded once on the host.
//   group    a connected component of that relation; label = its lowest ORIGINAL index, size = its member count.
// Both are integers with one correct answer, so nothing below may depend on scheduling, and nothing does:
//   link     one target per lane, the 64 targets of a wave consecutive SORTED positions p; the walk of nntree_walk_kernel with the
//            constant cap b2: a node is skipped iff no lane has !(nntree_bound > b2) — strict, so a record at exactly b2 is met, and
//            exact for the reason given at the head of nntree.inc (the bound is monotone in pair_d2's own chain: no epsilon).  A lane
//            only links to records at positions q < p: pair_d2 is bitwise symmetric, so the pair (p, q) is tested once, by the later
//            of the two, and the same bits decide.  Hence the walk also ends at the first node whose range starts past the wave's
//            last position.  Padding is masked by position (q < p < n), the self pair by q < p.  Every hit is a unite(p, q) on
//            parent[] by fof_union.hpp's find and hook, whose head says why every loop ends and that none waits.  WHICH hooks succeed
//            depends on timing; the partition they leave does not, and because the larger root is always pointed at the smaller, a
//            set's root is its lowest sorted position whatever the order: root[] is deterministic too.
//            Every access to parent[] in the link kernel is a relaxed agent-scope atomic (load, store, CAS).  Nothing else carries
//            information between waves; the kernels after it are ordered by the stream.
//   flatten  root[p] = find(p) after the link kernel has finished, minidx[root] by integer atomic min of the original index, count[root]
//            by integer add — aggregated per wave first: consecutive sorted positions mostly share a root, so the leader of each run
//            of equal roots adds the run's length and the run's lowest index (a group of 10^6 members would otherwise issue 10^6
//            atomics to one address).  Integer min and add are order-free.
//   labels   label[j] = minidx[root[p]], size[j] = count[root[p]] through the record's original index j; and the catalogue sort's key.
//   summary  one block: groups (label[i] == i), catalogued groups c (size >= min_members among those), and the 64-bit max of
//            (size << 32) | ~label: the largest group, the lowest label among equals.
//   catalogue  radix_sort.hpp sorts (label, original position): a group's members come out contiguous, ascending in index.  Group heads
//            with size >= min_members are numbered in label order by count per strip, a one-block exclusive scan and a scatter (the
//            look of block_schedule.hpp; no decoupled look-back, which spins).  One wave per catalogued group then sums m and m x in
//            DOUBLE for both types: lane l takes members l, l + 64, ... in order, the 64 partials are folded by a fixed xor-shuffle
//            tree, com = sum(m x) / sum(m), one rounding to T.  The grid is sized from n and min_members; c is read from device memory.
// Why every loop ends (in full at the head of fof_union.hpp, whose text also runs on host threads under the sanitizers):
//   find     parent[x] <= x always — the identity has it, a hook writes a smaller root into a larger one, halving writes an ancestor —
//            so a chain strictly decreases and reaches a root after at most x steps, whatever other lanes do meanwhile.
//   hook     repeats only after a FAILED CAS on a root it had just found; that fails only if another lane's hook of that root
//            succeeded, every success removes one of n roots for good: at most n - 1 in all.
//   walks    the link walk visits nodes in strictly increasing successor order and stops at the root, a dead node or a node past the
//            wave; every other loop has a trip count fixed by n.
//   NO loop waits for another lane, wave or block to do something: no spin, no flag, no ticket, no decoupled look-back.
// No floating-point atomics, nothing read back, nothing allocated after create: two computes give the same bits, and a compute may be
// recorded.  Cost (profiles/fof/time_fof.txt): the shared structure, then a link walk that is latency bound like the kNN walk, with
// two dependent chains of atomic loads per linked pair on top.

constexpr int kFofSumBlock = 1024;  // lanes of the summary and of the scan block
constexpr uint32_t kFofNone = 0xffffffffu;

// parent[]'s operations for fof_union.hpp: relaxed, agent scope (the waves of one launch share nothing else)
struct fof_dev_atomics {
  static __device__ __forceinline__ uint32_t load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ bool cas(uint32_t* p, uint32_t expect, uint32_t want) {
    return __hip_atomic_compare_exchange_strong(p, &expect, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// ---- init ----------------------------------------------------------------------------------------------------------------------
// parent = identity over the padded sorted positions; minidx and count armed for the flatten.  grid: padded / kNtBlock.
static __global__ __launch_bounds__(kNtBlock) void fof_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ minidx,
                                                                   uint32_t* __restrict__ count, uint32_t n) {
  const uint32_t p = blockIdx.x * kNtBlock + threadIdx.x;  // < padded
  parent[p]        = p;
  if (p < n) {
    minidx[p] = kFofNone;
    count[p]  = 0u;
  }
}

// ---- link ----------------------------------------------------------------------------------------------------------------------
// grid: padded / kNtBlock blocks; every wave on its own (no LDS, no barrier).
template <typename T, int D>
static __global__ __launch_bounds__(kNtBlock) void fof_link_kernel(const void* __restrict__ srt_, const void* __restrict__ boxes_, uint32_t* parent,
                                                                   uint32_t n, uint32_t levels, T b2) {
  const auto* srt     = static_cast<const nntree_rec<T>*>(srt_);
  const auto* boxes   = static_cast<const nntree_box<T>*>(boxes_);
  constexpr int U     = sizeof(T) == 8 ? 2 : 4;  // records a batch
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(blockIdx.x * (kNtBlock / 64) + (threadIdx.x >> 6))));
  if (wave * 64u >= n) return;                 // wave-uniform
  const uint32_t tp   = wave * 64u + lane;     // < padded: the sorted records are padded to whole blocks
  const uint32_t last = wave * 64u + 63u;      // the wave's last position: no lane links to a record beyond it
  const bool live     = tp < n;

  T xi[D];
#pragma unroll
  for (int c = 0; c < D; ++c) xi[c] = srt[tp].p[c];

  uint32_t node = 1u;
#pragma unroll 1
  for (;;) {
    const uint32_t depth = 31u - uint32_t(__builtin_clz(node));
    const uint32_t sh    = levels - depth;
    const uint32_t first = (node - (1u << depth)) << sh;  // the node's first leaf
    const uint32_t q0    = first * uint32_t(kNtB);        // ... and its first sorted position
    if (q0 >= n || q0 > last) break;                      // dead, or wholly past the wave: so is every node after it
    const T bound = nntree_bound<T, D>(boxes[node], xi);
    if (__builtin_amdgcn_ballot_w64(!(bound > b2)) != 0ull) {  // some lane needs the node
      if (sh != 0u) {
        node = 2u * node;
        continue;
      }
      const nntree_rec<T>* src = srt + size_t(first) * kNtB;
#pragma unroll 1
      for (int jj = 0; jj < kNtB; jj += U) {
        if (q0 + uint32_t(jj) > last) break;  // wave-uniform: q < p fails for every lane from here on
        bool hit[U], any = false;
#pragma unroll
        for (int b = 0; b < U; ++b) {
          T s[D];
#pragma unroll
          for (int c = 0; c < D; ++c) s[c] = src[jj + b].p[c];
          const T d2 = pair_d2<T, D>(s, xi);
          hit[b]     = live && q0 + uint32_t(jj + b) < tp && d2 <= b2;  // q < p < n: the self pair and the padding are out by position
          any |= hit[b];
        }
        if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
#pragma unroll
          for (int b = 0; b < U; ++b)
            if (hit[b]) fof_hook<fof_dev_atomics>(parent, tp, q0 + uint32_t(jj + b));
        }
      }
    }
    node = (node + 1u) >> __builtin_ctz(node + 1u);  // skipped or finished: the same move
    if (node == 1u) break;
  }
}

// ---- flatten -------------------------------------------------------------------------------------------------------------------
// One lane per sorted position p < padded, after the link kernel: the roots are final.  Lanes past n carry root kFofNone, which no
// live lane has, so they end the last run and add nothing.
template <typename T>
static __global__ __launch_bounds__(kNtBlock) void fof_flatten_kernel(const void* __restrict__ srt_, uint32_t* parent, uint32_t* __restrict__ root,
                                                                      uint32_t* minidx, uint32_t* count, uint32_t n) {
  const auto* srt     = static_cast<const nntree_rec<T>*>(srt_);
  const uint32_t p    = blockIdx.x * kNtBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool live     = p < n;
  const uint32_t r    = live ? fof_find<fof_dev_atomics>(parent, p) : kFofNone;
  root[p]             = r;
  uint32_t m          = live ? uint32_t(srt[p].j) : kFofNone;
  const uint32_t prev = __shfl_up(r, 1, 64);
  const bool leader   = lane == 0u || prev != r;
  const uint64_t mask = __builtin_amdgcn_ballot_w64(leader);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {  // the lowest index of the run, at its leader (a lane of the same root further on may join: harmless)
    const uint32_t v = __shfl_down(m, off, 64), rr = __shfl_down(r, off, 64);
    if (lane + uint32_t(off) < 64u && rr == r) m = v < m ? v : m;
  }
  if (leader && live) {
    const uint64_t higher = (mask >> lane) >> 1;
    const uint32_t len    = higher ? uint32_t(__builtin_ctzll(higher)) + 1u : 64u - lane;
    __hip_atomic_fetch_add(count + r, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(minidx + r, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- labels and sizes ----------------------------------------------------------------------------------------------------------
// One lane per sorted position p < n, after the flatten: original order through the record's index.  key: the catalogue sort's.
template <typename T>
static __global__ __launch_bounds__(kNtBlock) void fof_labels_kernel(const void* __restrict__ srt_, const uint32_t* __restrict__ root,
                                                                     const uint32_t* __restrict__ minidx, const uint32_t* __restrict__ count,
                                                                     uint32_t* __restrict__ label, uint32_t* __restrict__ size,
                                                                     uint64_t* __restrict__ key, uint32_t n) {
  const auto* srt  = static_cast<const nntree_rec<T>*>(srt_);
  const uint32_t p = blockIdx.x * kNtBlock + threadIdx.x;
  if (p >= n) return;
  const uint32_t r = root[p], j = uint32_t(srt[p].j);
  const uint32_t l = minidx[r];
  label[j]         = l;
  size[j]          = count[r];
  key[j]           = uint64_t(l);
}

// ---- summary -------------------------------------------------------------------------------------------------------------------
// One block: out[0] groups, out[1] catalogued groups, out[2] the largest size, out[3] its label (the lowest among equals).
static __global__ __launch_bounds__(kFofSumBlock) void fof_summary_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ size,
                                                                          uint32_t n, uint32_t min_members, uint32_t* __restrict__ out) {
  __shared__ uint32_t rg[kFofSumBlock / 64], rc[kFofSumBlock / 64];
  __shared__ uint64_t rb[kFofSumBlock / 64];
  uint32_t g = 0u, c = 0u;
  uint64_t best = 0ull;
  for (uint32_t i = threadIdx.x; i < n; i += kFofSumBlock) {
    if (label[i] != i) continue;
    const uint32_t s = size[i];
    ++g;
    c += s >= min_members ? 1u : 0u;
    const uint64_t v = (uint64_t(s) << 32) | uint64_t(~i);
    best             = v > best ? v : best;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    g += __shfl_xor(g, off, 64);
    c += __shfl_xor(c, off, 64);
    const uint64_t o = __shfl_xor(best, off, 64);
    best             = o > best ? o : best;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    rg[wave] = g;
    rc[wave] = c;
    rb[wave] = best;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kFofSumBlock / 64; ++w) {
      g += rg[w];
      c += rc[w];
      best = rb[w] > best ? rb[w] : best;
    }
    out[0] = g;
    out[1] = c;
    out[2] = uint32_t(best >> 32);
    out[3] = ~uint32_t(best);
  }
}

// ---- catalogue: ordered compaction of the group heads --------------------------------------------------------------------------
// key / perm: the bodies sorted by (label, index).  Position s is the head of a catalogued group if it starts a run of equal keys
// and that group's size is >= min_members.
__device__ __forceinline__ bool fof_head(const uint64_t* key, const uint32_t* perm, const uint32_t* size, uint32_t s, uint32_t n,
                                         uint32_t min_members) {
  if (s >= n) return false;
  if (s != 0u && key[s - 1u] == key[s]) return false;
  return size[perm[s]] >= min_members;
}

__device__ __forceinline__ uint32_t fof_wave_scan(uint32_t v, int lane) {  // inclusive, over the 64 lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// grid: strips of kNtBlock positions
static __global__ __launch_bounds__(kNtBlock) void fof_cat_count_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ perm,
                                                                        const uint32_t* __restrict__ size, uint32_t n, uint32_t min_members,
                                                                        uint32_t* __restrict__ scount) {
  __shared__ uint32_t wcnt[kNtBlock / 64];
  const uint32_t s = blockIdx.x * kNtBlock + threadIdx.x;
  uint32_t c       = uint32_t(__popcll(__builtin_amdgcn_ballot_w64(fof_head(key, perm, size, s, n, min_members))));
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kNtBlock / 64; ++w) c += wcnt[w];
    scount[blockIdx.x] = c;
  }
}

// one block: scount[0 .. nb) -> its exclusive scan in place
static __global__ __launch_bounds__(kFofSumBlock) void fof_cat_scan_kernel(uint32_t* __restrict__ scount, uint32_t nb) {
  __shared__ uint32_t wsum[kFofSumBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t running = 0;
  for (uint32_t base = 0; base < nb; base += kFofSumBlock) {
    const uint32_t j   = base + threadIdx.x;
    const uint32_t v   = j < nb ? scount[j] : 0u;
    const uint32_t inc = fof_wave_scan(v, lane);
    __syncthreads();  // the previous round's wsum has been read
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kFofSumBlock / 64; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (j < nb) scount[j] = running + before + inc - v;
    running += total;
  }
}

// entry e of the catalogue: its label, its size and where its members start in the sorted order.  cmax: the entries allocated
// (n / min_members: there cannot be more groups of that size).
static __global__ __launch_bounds__(kNtBlock) void fof_cat_scatter_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ perm,
                                                                          const uint32_t* __restrict__ size, uint32_t n, uint32_t min_members,
                                                                          const uint32_t* __restrict__ soff, uint32_t* __restrict__ cat_label,
                                                                          uint32_t* __restrict__ cat_size, uint32_t* __restrict__ cat_start,
                                                                          uint32_t cmax) {
  __shared__ uint32_t wcnt[kNtBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t s      = blockIdx.x * kNtBlock + threadIdx.x;
  const bool head       = fof_head(key, perm, size, s, n, min_members);
  const uint64_t ballot = __builtin_amdgcn_ballot_w64(head);
  if (lane == 0) wcnt[wave] = uint32_t(__popcll(ballot));
  __syncthreads();
  if (!head) return;
  uint32_t e = soff[blockIdx.x] + uint32_t(__popcll(ballot & ((1ull << lane) - 1ull)));
  for (int w = 0; w < wave; ++w) e += wcnt[w];
  if (e < cmax) {  // always: see cmax
    cat_label[e] = uint32_t(key[s]);
    cat_size[e]  = size[perm[s]];
    cat_start[e] = s;
  }
}

// ---- catalogue: mass and centre of mass ----------------------------------------------------------------------------------------
// One wave per entry; grid: cmax entries cut into blocks of kNtBlock / 64, the c catalogued ones read from summary[1].  recs: the
// packed records in ORIGINAL order ({x[3], m}); perm: the sorted order's original indices, ascending inside a group.
template <typename T, int D>
static __global__ __launch_bounds__(kNtBlock) void fof_cat_sum_kernel(const pair_rec<T>* __restrict__ recs, const uint32_t* __restrict__ perm,
                                                                      const uint32_t* __restrict__ cat_size, const uint32_t* __restrict__ cat_start,
                                                                      const uint32_t* __restrict__ summary, T* __restrict__ cat_mass,
                                                                      T* __restrict__ cat_com, uint32_t cmax) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t e    = uint32_t(__builtin_amdgcn_readfirstlane(int(blockIdx.x * (kNtBlock / 64) + (threadIdx.x >> 6))));
  const uint32_t c    = summary[1];
  if (e >= c || e >= cmax) return;  // wave-uniform
  const uint32_t cnt = cat_size[e], s0 = cat_start[e];
  double a[D + 1];  // sum m, sum m x
#pragma unroll
  for (int q = 0; q < D + 1; ++q) a[q] = 0.0;
  constexpr uint32_t V = 8;  // members a lane has in flight; the additions stay in member order
  uint32_t t = lane;
  for (; t + 64u * (V - 1u) < cnt; t += 64u * V) {
    pair_rec<T> r[V];
#pragma unroll
    for (uint32_t v = 0; v < V; ++v) r[v] = recs[perm[s0 + t + 64u * v]];
#pragma unroll
    for (uint32_t v = 0; v < V; ++v) {
      const double m = double(r[v].m);
      a[0] += m;
#pragma unroll
      for (int k = 0; k < D; ++k) a[1 + k] += m * double(r[v].p[k]);
    }
  }
  for (; t < cnt; t += 64u) {
    const pair_rec<T> r = recs[perm[s0 + t]];
    const double m      = double(r.m);
    a[0] += m;
#pragma unroll
    for (int k = 0; k < D; ++k) a[1 + k] += m * double(r.p[k]);
  }
#pragma unroll
  for (int q = 0; q < D + 1; ++q)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a[q] += __shfl_xor(a[q], off, 64);
  if (lane == 0u) {
    cat_mass[e] = T(a[0]);
#pragma unroll
    for (int k = 0; k < D; ++k) cat_com[size_t(e) * D + k] = T(a[1 + k] / a[0]);
  }
}
