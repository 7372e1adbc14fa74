// The TREE method of nbody_knn_* (NBODY_KNN_TREE): the same k nearest neighbours, densities and summary as the all-pairs sweep of
// knn.hip, BIT FOR BIT, from a source loop that does not visit everything.  Included from knn.hip, inside namespace nbody, after
// knn_insert, knn_finish_tail and the summary kernel, which it uses.  (No kernel here has `knn_` in its name: the all-pairs kernels
// are counted by that prefix.)
//
// Structure, rebuilt by every compute (the state is neither changed nor permuted):
//   records  the bodies sorted by (Morton key, index): {x[3], original index}, one scalar load each.  Keys are 21 bits an axis in
//            3D and 32 in 2D, quantised on the system's bounds; an axis of zero extent contributes zero bits.  ONLY SPEED depends on
//            the keys: whatever they are, the structure below holds every body exactly once.
//   buckets  kNtB consecutive sorted records.  A bucket's box is the min / max of the coordinates of its records p < n: no padding
//            term, no tolerance.
//   tree     a complete binary tree over the buckets in heap order (root 1, children 2 i and 2 i + 1, the leaves at L ... 2 L - 1,
//            L the power of two >= the bucket count), a node's box the union of its children's.  A node whose range starts at or
//            past n is DEAD — decided from the index arithmetic, never from a box; dead nodes are neither written nor read.
// Walk: one target per lane, the 64 targets of a wave consecutive SORTED positions, so the lanes want nearly the same nodes.  The
// node index is wave-uniform and the box and the records come through scalar loads.  Depth first, left to right, no stack: the
// node after i, whether i was skipped or finished, is (i + 1) >> ctz(i + 1) — the sibling of a left child, the parent's successor
// of a right child — and the walk is over when that is the root, or at the first dead node (every later one is dead too).
//
// What makes it exact:
//   the bound   per axis g_k = max(lo_k - x_k, x_k - hi_k, 0), then t = g_0 g_0, t = fma(g_k, g_k, t): pair_d2's chain, contraction
//               off.  For a record y inside the box |y_k - x_k| >= g_k in exact arithmetic; a correctly rounded subtraction is
//               monotone, so the COMPUTED |d_k| >= the computed g_k, and the square and the FMA are monotone in |d_k| and t.  Hence
//               the computed d2 of every record in the box is >= the computed bound.  No epsilon.
//   the prune   the walk meets records in sorted-position order, not index order, so lists are kept LEXICOGRAPHICALLY on (d2,
//               original index): knn_insert<T, K, true>.  A record whose d2 EQUALS the list's k-th but whose index is lower must still
//               get in, so a node is skipped only if bound > cap, strictly, and the batch gate is d2 <= cap.
//   the cap     the k-th entry of the lane's list (k the handle's, not the capacity K): the true k-th distance is <= the k-th of
//               any subset, so a record beyond it cannot be among the k that are output.  Entries k ... K - 1 of a list are scratch.
//               The cap may be stale (larger): that only admits records the insert then orders correctly.
//   masking     the self pair is excluded by sorted position (equivalent to by index), padding by p >= n.  A masked record is
//               turned into (+inf, 0xffffffff), which is below no entry of any list — it is SKIPPED.  (An (inf, j) with a real j
//               would pass a `<=` gate against a list that is not full and leave j in a slot that must read 0xffffffff.)  A d2
//               that overflowed to +inf gets the same treatment: the all-pairs sweep's strict `<` never takes it either.
//   finish      the walk writes row perm[p] of idx and d2; a kernel of its own then computes rho through knn_finish_tail, the
//               all-pairs finish's arithmetic, so the walk has no divide and no root.
//   once        every bucket is offered to a lane once: the seed range by the seed, every other bucket by the walk, which skips
//               the seed range BY INDEX.  (A lexicographic insert of a duplicate would store it twice.)
//   seeding     a left-to-right walk prunes badly until the list holds near bodies, so every wave first sweeps the buckets around
//               its own sorted positions (its two and kNtSeed = 2 on either side) and keeps the list.
// Lanes past n carry a list of -inf: no bound and no d2 is <= -inf, so they never ask for a node or a record.
// Bound (measured, profiles/knn_tree/time_knn_tree.txt): the walk is about 85 % of a compute and it is LATENCY bound, not VALU bound —
// every node is a dependent scalar load, a bound and a ballot, so a wave's time is its chain of visits and the device is filled by
// occupancy alone.  Not done: loading both children's boxes (adjacent in heap order) with one request, a nearest-first order.

// Experiment builds (make experiments EXPDEFS="-DNBODY_NT_B=16 -DNBODY_NT_SEED=2") may set the bucket size and the seed's reach; what
// was measured is in profiles/knn_tree/time_knn_tree.txt.
#if defined(NBODY_EXPERIMENTS) && defined(NBODY_NT_B)
constexpr int kNtB = NBODY_NT_B;
#else
constexpr int kNtB = 32;  // records a bucket: a power of two <= 64 (64 / kNtB buckets are one wave's targets)
#endif
#if defined(NBODY_EXPERIMENTS) && defined(NBODY_NT_SEED)
constexpr int kNtSeed = NBODY_NT_SEED;
#else
constexpr int kNtSeed = 2;  // buckets on either side of the wave's own that the seed sweeps
#endif
static_assert(kNtB >= 2 && kNtB <= 64 && (kNtB & (kNtB - 1)) == 0 && kNtSeed >= 0, "bucket size");
constexpr int kNtBlock     = 256;   // lanes a block of every kernel here but the upper levels'
constexpr int kNtUpper     = 1024;  // lanes of the one block that builds the upper levels
constexpr int kNtMaxBounds = 256;   // at most this many partial bounds (one a block of the bounds kernel)

template <typename T>
struct nntree_index {
  using type = uint32_t;
};
template <>
struct nntree_index<double> {
  using type = uint64_t;
};

// Sorted record: the position and the ORIGINAL index (as wide as T, so the record is 4 T: one s_load_dwordx4 / x8).
template <typename T>
struct alignas(sizeof(T) * 4) nntree_rec {
  T p[3];
  typename nntree_index<T>::type j;
};

// Box of a node (and a partial of the bounds): 8 T, one s_load_dwordx8 / x16.
template <typename T>
struct alignas(sizeof(T) * 8) nntree_box {
  T lo[3], hi[3], unused[2];
};

// The shape of the tree, from n alone.
struct nntree_shape {
  uint32_t buckets, levels, leaves, bounds_blocks;  // leaves = 1 << levels >= buckets
};
inline nntree_shape nntree_shape_for(uint32_t n) {
  nntree_shape s;
  s.buckets = (n + uint32_t(kNtB) - 1u) / uint32_t(kNtB);
  s.levels  = 0;
  while ((1u << s.levels) < s.buckets) ++s.levels;
  s.leaves        = 1u << s.levels;
  s.bounds_blocks = (n + 1023u) / 1024u;
  if (s.bounds_blocks > uint32_t(kNtMaxBounds)) s.bounds_blocks = uint32_t(kNtMaxBounds);
  return s;
}

// min / max of lo / hi over the block's lanes, in every lane.  red: [2 D][kNtBlock / 64].
template <typename T, int D>
__device__ __forceinline__ void nntree_block_minmax(T (&lo)[D], T (&hi)[D], T (*red)[kNtBlock / 64]) {
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[k] = __builtin_elementwise_min(lo[k], __shfl_xor(lo[k], off, 64));
      hi[k] = __builtin_elementwise_max(hi[k], __shfl_xor(hi[k], off, 64));
    }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      red[k][wave]     = lo[k];
      red[D + k][wave] = hi[k];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < D; ++k) {
    lo[k] = red[k][0];
    hi[k] = red[D + k][0];
    for (int w = 1; w < kNtBlock / 64; ++w) {
      lo[k] = __builtin_elementwise_min(lo[k], red[k][w]);
      hi[k] = __builtin_elementwise_max(hi[k], red[D + k][w]);
    }
  }
}

// ---- bounds --------------------------------------------------------------------------------------------------------------------
// Partial min / max of x per block over a grid-strided range; no atomics.  The keys kernel folds the partials.
template <typename T, int D>
static __global__ __launch_bounds__(kNtBlock) void nntree_bounds_kernel(const pair_rec<T>* __restrict__ recs, nntree_box<T>* __restrict__ part,
                                                                        uint32_t n) {
  __shared__ T red[2 * D][kNtBlock / 64];
  T lo[D], hi[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    lo[k] = pair_inf<T>();
    hi[k] = -pair_inf<T>();
  }
  for (uint32_t i = blockIdx.x * kNtBlock + threadIdx.x; i < n; i += gridDim.x * kNtBlock) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const T v = recs[i].p[k];
      lo[k]     = __builtin_elementwise_min(lo[k], v);
      hi[k]     = __builtin_elementwise_max(hi[k], v);
    }
  }
  nntree_block_minmax<T, D>(lo, hi, red);
  if (threadIdx.x == 0) {
    nntree_box<T> b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = k < D ? lo[k < D ? k : 0] : T(0);
      b.hi[k] = k < D ? hi[k < D ? k : 0] : T(0);
    }
    b.unused[0] = b.unused[1] = T(0);
    part[blockIdx.x] = b;
  }
}

// ---- keys ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t nntree_spread3(uint64_t v) {  // 21 bits, two zero bits after each
  v &= 0x1fffffull;
  v = (v | (v << 32)) & 0x001f00000000ffffull;
  v = (v | (v << 16)) & 0x001f0000ff0000ffull;
  v = (v | (v << 8)) & 0x100f00f00f00f00full;
  v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}
__device__ __forceinline__ uint64_t nntree_spread2(uint64_t v) {  // 32 bits, one zero bit after each
  v &= 0xffffffffull;
  v = (v | (v << 16)) & 0x0000ffff0000ffffull;
  v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
  v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}

// Every block folds the nparts <= kNtBlock partial bounds for itself, then one key per lane.  Quantised in double for both types;
// the cell is clamped to [0, cells - 1]; an axis of zero (or non-finite) extent has scale 0: all its cells are 0.
template <typename T, int D>
static __global__ __launch_bounds__(kNtBlock) void nntree_keys_kernel(const pair_rec<T>* __restrict__ recs, const nntree_box<T>* __restrict__ part,
                                                                      uint32_t nparts, uint64_t* __restrict__ keys, uint32_t n) {
  __shared__ T red[2 * D][kNtBlock / 64];
  T lo[D], hi[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    lo[k] = threadIdx.x < nparts ? part[threadIdx.x].lo[k] : pair_inf<T>();
    hi[k] = threadIdx.x < nparts ? part[threadIdx.x].hi[k] : -pair_inf<T>();
  }
  nntree_block_minmax<T, D>(lo, hi, red);
  const uint32_t i = blockIdx.x * kNtBlock + threadIdx.x;
  if (i >= n) return;
  constexpr double cells = D == 3 ? 2097152.0 : 4294967296.0;
  uint64_t key = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double ext = double(hi[k]) - double(lo[k]);
    const double sc  = (ext > 0.0 && ext < __builtin_huge_val()) ? cells / ext : 0.0;
    const double v   = (double(recs[i].p[k]) - double(lo[k])) * sc;
    const uint64_t q = v >= cells - 1.0 ? uint64_t(cells - 1.0) : (v > 0.0 ? uint64_t(v) : 0ull);
    key |= (D == 3 ? nntree_spread3(q) : nntree_spread2(q)) << k;
  }
  keys[i] = key;
}

// ---- gather and the buckets' boxes ---------------------------------------------------------------------------------------------
// One lane per sorted position p < padded (a multiple of kNtBlock): the record of body perm[p], or padding (the origin, index
// 0xffffffff) for p >= n; the 32 lanes of a bucket reduce its box over the records p < n.  leafbox: the leaves' boxes, boxes + L.
template <typename T, int D>
static __global__ __launch_bounds__(kNtBlock) void nntree_gather_kernel(const pair_rec<T>* __restrict__ recs, const uint32_t* __restrict__ perm,
                                                                        nntree_rec<T>* __restrict__ srt, nntree_box<T>* __restrict__ leafbox,
                                                                        uint32_t n, uint32_t buckets) {
  const uint32_t p = blockIdx.x * kNtBlock + threadIdx.x;
  nntree_rec<T> r;
  r.p[0] = r.p[1] = r.p[2] = T(0);
  r.j                      = kNoNeighbour;
  T lo[D], hi[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    lo[k] = pair_inf<T>();
    hi[k] = -pair_inf<T>();
  }
  if (p < n) {
    const uint32_t j = perm[p];
    r.j              = j;
#pragma unroll
    for (int k = 0; k < D; ++k) r.p[k] = lo[k] = hi[k] = recs[j].p[k];
  }
  srt[p] = r;
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int off = kNtB / 2; off > 0; off >>= 1) {
      lo[k] = __builtin_elementwise_min(lo[k], __shfl_xor(lo[k], off, 64));
      hi[k] = __builtin_elementwise_max(hi[k], __shfl_xor(hi[k], off, 64));
    }
  const uint32_t bucket = p / uint32_t(kNtB);
  if ((threadIdx.x & (kNtB - 1)) == 0 && bucket < buckets) {
    nntree_box<T> b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = k < D ? lo[k < D ? k : 0] : T(0);
      b.hi[k] = k < D ? hi[k < D ? k : 0] : T(0);
    }
    b.unused[0] = b.unused[1] = T(0);
    leafbox[bucket] = b;
  }
}

// ---- the upper levels ----------------------------------------------------------------------------------------------------------
// One block, bottom up, a barrier between levels.  Node q of the level of 2^d nodes starts at leaf q << (levels - d); it is dead
// if that leaf's first record is >= n, and so is every later node of the level.  A live node's left child is live (it starts at
// the same leaf); its right child may be dead, then the node's box is the left child's.
template <typename T, int D>
static __global__ __launch_bounds__(kNtUpper) void nntree_upper_kernel(nntree_box<T>* __restrict__ boxes, uint32_t n, uint32_t levels) {
  for (int d = int(levels) - 1; d >= 0; --d) {
    const uint32_t cnt = 1u << d, sh = levels - uint32_t(d);
    for (uint32_t q = threadIdx.x; q < cnt; q += kNtUpper) {
      const uint32_t first = q << sh;
      if (first * uint32_t(kNtB) >= n) break;
      const uint32_t i = cnt + q;
      nntree_box<T> a  = boxes[2u * i];
      if ((first + (1u << (sh - 1u))) * uint32_t(kNtB) < n) {
        const nntree_box<T> b = boxes[2u * i + 1u];
#pragma unroll
        for (int k = 0; k < D; ++k) {
          a.lo[k] = __builtin_elementwise_min(a.lo[k], b.lo[k]);
          a.hi[k] = __builtin_elementwise_max(a.hi[k], b.hi[k]);
        }
      }
      boxes[i] = a;
    }
    __threadfence_block();
    __syncthreads();
  }
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------
// The k-th entry of a list of capacity K (k wave-uniform, 1 <= k <= K); static indices only.  Every entry passes through an empty asm
// on its way into the select chain: without it the compiler folds the chain into ONE load at a dynamic index, and a list that is
// indexed dynamically anywhere leaves the registers for LDS or scratch everywhere.
template <typename T, int K>
__device__ __forceinline__ T nntree_cap(const T (&ld)[K], int k) {
  T c = ld[K - 1];
#pragma unroll
  for (int s = 0; s < K - 1; ++s) {
    T v = ld[s];
    asm("" : "+v"(v));
    c = (s == k - 1) ? v : c;
  }
  return c;
}

// The lower bound of the computed d2 of every record inside the box, for the target at xi (see the head of the file).
template <typename T, int D>
__device__ __forceinline__ T nntree_bound(const nntree_box<T>& b, const T (&xi)[D]) {
#pragma clang fp contract(off)
  T g[D];
#pragma unroll
  for (int k = 0; k < D; ++k) g[k] = __builtin_elementwise_max(__builtin_elementwise_max(b.lo[k] - xi[k], xi[k] - b.hi[k]), T(0));
  T t = g[0] * g[0];
#pragma unroll
  for (int k = 1; k < D; ++k) t = __builtin_elementwise_fma(g[k], g[k], t);
  return t;
}

// One bucket (sorted positions p0 ... p0 + kNtB - 1, records at src: wave-uniform) against the target of a lane (sorted position
// tp), U records a batch.  CHECK: the self pair and the records p >= n are masked by position; without it the bucket holds neither.
template <typename T, int D, int K, int U, bool CHECK>
__device__ __forceinline__ void nntree_bucket(T (&ld)[K], uint32_t (&lj)[K], T& cap, const T (&xi)[D], uint32_t tp,
                                              const nntree_rec<T>* __restrict__ src, uint32_t p0, uint32_t n, int k) {
#pragma unroll 1
  for (int jj = 0; jj < kNtB; jj += U) {
    T d2[U];
    uint32_t j[U];
#pragma unroll
    for (int b = 0; b < U; ++b) {
      T s[D];
#pragma unroll
      for (int c = 0; c < D; ++c) s[c] = src[jj + b].p[c];
      j[b]  = uint32_t(src[jj + b].j);
      d2[b] = pair_d2<T, D>(s, xi);
    }
    if constexpr (CHECK) {
#pragma unroll
      for (int b = 0; b < U; ++b) {
        const uint32_t p = p0 + uint32_t(jj + b);
        const bool ok    = p < n && p != tp;
        d2[b]            = ok ? d2[b] : pair_inf<T>();
        j[b]             = ok ? j[b] : kNoNeighbour;
      }
    }
    T mn = d2[0];
#pragma unroll
    for (int b = 1; b < U; ++b) mn = __builtin_elementwise_min(mn, d2[b]);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(mn <= cap) != 0ull, 0)) {
#pragma unroll
      for (int b = 0; b < U; ++b)  // a record no lane can take is skipped (its insertion would change nothing that is output)
        if (__builtin_amdgcn_ballot_w64(d2[b] <= cap) != 0ull)
          knn_insert<T, K, true>(ld, lj, d2[b], d2[b] < pair_inf<T>() ? j[b] : kNoNeighbour);
      cap = nntree_cap<T, K>(ld, k);
    }
  }
}

// grid: padded / kNtBlock blocks; every wave on its own (no LDS, no barrier).
template <typename T, int D, int K>
static __global__ __launch_bounds__(kNtBlock) void nntree_walk_kernel(const nntree_rec<T>* __restrict__ srt, const nntree_box<T>* __restrict__ boxes,
                                                                      uint32_t* __restrict__ idx, T* __restrict__ d2, uint32_t n,
                                                                      uint32_t levels, uint32_t buckets, int k) {
  constexpr int U     = sizeof(T) == 8 ? 2 : 4;  // records a batch
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(blockIdx.x * (kNtBlock / 64) + (threadIdx.x >> 6))));
  if (wave * 64u >= n) return;      // wave-uniform
  const uint32_t tp = wave * 64u + lane;  // < padded: the sorted records are padded to whole blocks
  const bool live   = tp < n;

  T xi[D], ld[K];
  uint32_t lj[K];
#pragma unroll
  for (int c = 0; c < D; ++c) xi[c] = srt[tp].p[c];
  const uint32_t self = uint32_t(srt[tp].j);
#pragma unroll
  for (int s = 0; s < K; ++s) {
    ld[s] = live ? pair_inf<T>() : -pair_inf<T>();
    lj[s] = kNoNeighbour;
  }
  T cap = ld[K - 1];

  // the seed: the wave's own buckets and kNtSeed on either side
  constexpr uint32_t kOwn = 64u / uint32_t(kNtB), kReach = uint32_t(kNtSeed);
  const uint32_t own      = wave * kOwn;
  const uint32_t s0       = own > kReach ? own - kReach : 0u;
  const uint32_t s1       = own + kOwn + kReach < buckets ? own + kOwn + kReach : buckets;
#pragma unroll 1
  for (uint32_t b = s0; b < s1; ++b) nntree_bucket<T, D, K, U, true>(ld, lj, cap, xi, tp, srt + size_t(b) * kNtB, b * uint32_t(kNtB), n, k);

  uint32_t node = 1u;
#pragma unroll 1
  for (;;) {
    const uint32_t depth = 31u - uint32_t(__builtin_clz(node));
    const uint32_t sh    = levels - depth;
    const uint32_t first = (node - (1u << depth)) << sh;  // the node's first leaf
    if (first * uint32_t(kNtB) >= n) break;               // dead, and so is every node after it
    const T bound = nntree_bound<T, D>(boxes[node], xi);
    if (__builtin_amdgcn_ballot_w64(!(bound > cap)) != 0ull) {  // some lane needs the node
      if (sh != 0u) {
        node = 2u * node;
        continue;
      }
      if (first < s0 || first >= s1) {  // a bucket outside the seed range
        const nntree_rec<T>* src = srt + size_t(first) * kNtB;
        if ((first + 1u) * uint32_t(kNtB) > n) nntree_bucket<T, D, K, U, true>(ld, lj, cap, xi, tp, src, first * uint32_t(kNtB), n, k);
        else nntree_bucket<T, D, K, U, false>(ld, lj, cap, xi, tp, src, first * uint32_t(kNtB), n, k);
      }
    }
    node = (node + 1u) >> __builtin_ctz(node + 1u);  // skipped or finished: the same move
    if (node == 1u) break;
  }

  if (live) {  // row perm[p] of the outputs; the indices in the list are original ones already
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if (s < k) {
        idx[uint64_t(self) * k + s] = lj[s];
        d2[uint64_t(self) * k + s]  = ld[s];
      }
    }
  }
}

// ---- finish --------------------------------------------------------------------------------------------------------------------
// One lane per body in ORIGINAL order: its row back into a list and through knn_finish_tail, the all-pairs finish's own arithmetic
// (M added in list order from the original-order records, the divide and the root), so rho has the same bits.  The tail writes the
// row again, unchanged.  Kept out of the walk so that the walk has neither a divide nor a root.
template <typename T, int D, int K>
static __global__ __launch_bounds__(kNtBlock) void nntree_finish_kernel(const pair_rec<T>* __restrict__ recs, uint32_t* __restrict__ idx,
                                                                        T* __restrict__ d2, T* __restrict__ rho, uint32_t n, int k) {
  const uint32_t i = blockIdx.x * kNtBlock + threadIdx.x;
  if (i >= n) return;
  T ld[K];
  uint32_t lj[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    ld[s] = s < k ? d2[uint64_t(i) * k + (s < k ? s : 0)] : pair_inf<T>();
    lj[s] = s < k ? idx[uint64_t(i) * k + (s < k ? s : 0)] : kNoNeighbour;
  }
  knn_finish_tail<T, D, K>(ld, lj, recs, idx, d2, rho, i, n, k);
}

// ---- host: the structure -------------------------------------------------------------------------------------------------------
// What every compute over this structure rebuilds, and the buffers it lives in: nbody_knn (NBODY_KNN_TREE) and nbody_fof (fof.inc)
// both hold one.  keys, perm and hist are the sort's; they are free again once the gather has run.
struct nntree_structure {
  nntree_shape tree{};
  void* sorted      = nullptr;             // nntree_rec<T>[padded]
  void* boxes       = nullptr;             // nntree_box<T>[2 leaves], heap order
  void* bounds      = nullptr;             // nntree_box<T>[bounds_blocks]
  uint64_t* keys[2] = {nullptr, nullptr};  // [n] each
  uint32_t* perm[2] = {nullptr, nullptr};  // [n] each: the sort's index buffers
  uint32_t* hist    = nullptr;             // radix_sort_scratch_words(n)
};

// Sized from n alone, through the handle's owner.  Nothing is cleared: every compute writes all of it before it reads it.
inline void nntree_structure_alloc(nntree_structure* t, device_buffers& mem, size_t tsz, uint32_t n, uint32_t padded) {
  t->tree = nntree_shape_for(n);
  mem.alloc(&t->sorted, tsz * 4 * size_t(padded));
  mem.alloc(&t->boxes, tsz * 8 * 2 * size_t(t->tree.leaves));
  mem.alloc(&t->bounds, tsz * 8 * size_t(t->tree.bounds_blocks));
  for (int b = 0; b < 2; ++b) {
    mem.alloc(&t->keys[b], sizeof(uint64_t) * size_t(n));
    mem.alloc(&t->perm[b], sizeof(uint32_t) * size_t(n));
  }
  mem.alloc(&t->hist, sizeof(uint32_t) * radix_sort_scratch_words(n));
}

// pack, bounds, keys, sort, gather + bucket boxes, upper levels: recs (pair_rec<T>[padded], original order), t->sorted and t->boxes
// are what the walks read.  The launch count follows from n alone (the sort's form does).
template <typename T, int D>
static int nntree_structure_launch(const nntree_structure* t, const nbody_state* s, pair_rec<T>* recs, uint32_t n, uint32_t padded,
                                   hipStream_t st) {
  const nntree_shape& sh = t->tree;
  auto* sorted           = static_cast<nntree_rec<T>*>(t->sorted);
  auto* boxes            = static_cast<nntree_box<T>*>(t->boxes);
  auto* bounds           = static_cast<nntree_box<T>*>(t->bounds);
  uint64_t* keys[2]      = {t->keys[0], t->keys[1]};
  uint32_t* perm[2]      = {t->perm[0], t->perm[1]};
  hipLaunchKernelGGL((pair_pack_kernel<T, D>), dim3(padded / kHBlock), dim3(kHBlock), 0, st, static_cast<const T*>(s->m),
                     static_cast<const T*>(s->x), recs, n, padded);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((nntree_bounds_kernel<T, D>), dim3(sh.bounds_blocks), dim3(kNtBlock), 0, st, recs, bounds, n);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((nntree_keys_kernel<T, D>), dim3((n + kNtBlock - 1) / kNtBlock), dim3(kNtBlock), 0, st, recs, bounds, sh.bounds_blocks,
                     keys[0], n);
  NB_HIP(hipGetLastError());
  int fin = 0;
  if (int r = radix_sort_pairs(keys, perm, n, D == 3 ? 63 : 64, t->hist, st, &fin)) return r;
  hipLaunchKernelGGL((nntree_gather_kernel<T, D>), dim3(padded / kNtBlock), dim3(kNtBlock), 0, st, recs, perm[fin], sorted,
                     boxes + sh.leaves, n, sh.buckets);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((nntree_upper_kernel<T, D>), dim3(1), dim3(kNtUpper), 0, st, boxes, n, sh.levels);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}
