// All-pairs k nearest neighbours, Casertano & Hut (1985) local densities, the density centre, core radius and core density:
// nbody_knn_* of include/nbody_hip.h.  No reference counterpart.  Reads a state's (m, x), changes nothing in it; selection is on the
// UNSOFTENED squared distance, so no softening is involved and the call works after any algorithm, also with eps = 0.
//
// Definitions (T the state's type, D its dimension, d = x_j - x_i):
//   d2_ij   the UNSOFTENED squared distance, pair_d2 of pair_sweep.hpp (exactly the d2 of neighbours.hip): one FMA chain in component
//           order, bitwise symmetric in (i, j).
//   order   the k neighbours of i are the k smallest (d2_ij, j), j != i, in lexicographic order (equal computed d2: the lowest index),
//           listed ascending in that order.  A body has min(k, n - 1) of them; unused slots hold (0xffffffff, +inf).
//   K       the capacity of the list a lane carries, the smallest of {4, 8, 16} that is >= k.  The tie rule is exact, so the first k
//           entries of a list do not depend on K.
//   rho_i   M_i / (V d_k^D): M_i the masses of neighbours 0 .. k - 2 added in list order (the k-th itself excluded: Casertano & Hut's
//           unbiased form), 3D: rho = M / (T(4 pi / 3) (d2_k sqrt(d2_k))), 2D: rho = M / (T(pi) d2_k).  Correctly rounded sqrt, true
//           divide.  k = 1 or fewer than k neighbours (n <= k): rho = 0.  d2_k = 0 (coincident bodies): what IEEE gives (+inf).
//   summary x_dc = sum rho x / sum rho; r_c = sqrt(sum rho^2 |x - x_dc|^2 / sum rho^2) (the rho^2-weighted NBODY form);
//           rho_c = sum rho^2 / sum rho.  Accumulated in double for both types, rounded to T at the end.  sum rho = 0 (k = 1, n <= k)
//           or a non-finite rho (coincident bodies) gives NaN by IEEE rules: not an error.
//
// A handle made with NBODY_KNN_TREE computes the same outputs, bit for bit, by the tree-pruned search of nntree.inc (included below);
// what follows is the ALL_PAIRS method.
// Four launches per compute, all on the caller's stream, nothing allocated after nbody_knn_create:
//   pack     pair_sweep.hpp's: one lane per record {x[3], m}, padded with records at the origin to whole tiles.  A padding record
//            never becomes a neighbour because of an INDEX BOUND: every slice of 64 records that reaches past n runs the checked
//            batch body, which replaces the d2 of a record j >= n by +inf.
//   sweep    the hot path, over pair_sweep_tiles of pair_sweep.hpp: ONE target per lane (the list alone is 48 VGPRs at K = 16 in
//            double), the tiles cut over grid.y chunks by knn_plan_for(sz): a function of sz alone; what is here is the pair batch,
//            the slice and the merge of the block's waves.  A lane carries its target's sorted list (d2[K], idx[K]) in registers;
//            every access is statically indexed in unrolled code.
//            No transcendental at all.  A batch of U records takes U - 1 v_min and ONE compare of the batch's minimum against the
//            list's last entry; only if some lane of the wave has a candidate (one ballot, one scalar branch) do the lanes walk the
//            batch in index order (one more ballot per record skips a record no lane can take) and insert each record with d2
//            strictly below the last entry by an unrolled compare-and-shift.
//            Strict `<` keeps the earlier (lower) index among equal values, because a lane meets its sources in ascending index
//            order.  The result is the same whichever way the branch goes.
//            Two batch bodies, chosen per slice by pair_sweep_tiles: the CHECKED one masks the self pair and the padding (d2 +inf)
//            by index; every other slice runs the plain body, which has no index test at all.
//            The block's waves merge through LDS, one wave's lists at a time (12 K bytes per lane), LEXICOGRAPHICALLY on (d2, idx):
//            a wave's slice of a later tile holds higher indices than another wave's slice of an earlier tile.  The chunk's lists
//            go to the partial arrays T[chunk][n][K], uint32[chunk][n][K].
//   finish   one lane per body: the chunks' lists merged by the same rule; writes idx[n][k], d2[n][k] row-major and rho[n].
//   summary  one block: the sums above, strided per lane, then across the wave and the block in a fixed order — a function of sz
//            alone, no atomics — into the handle's record.
// Nothing is read from the device or the CU count, no atomics, no waiting between blocks, and the order has an exact tie rule: two
// runs, an eager call and a replayed recorded one, and a handle destroyed and made again give the same bits.
// Bound: FP64 / FP32 VALU issue; per pair D subtractions, D chain operations, (U - 1) / U min + 1 / U compare, and for a batch that
// takes the branch U insertions of K compares and 2 K selects (3 K v_cndmask in double).
#include "pair_sweep.hpp"
#include "radix_sort.hpp"
#include "fof_union.hpp"
#include "nlist_plan.hpp"

#pragma clang fp contract(off)

namespace nbody {

constexpr int kKnnMax        = 16;  // NBODY_KNN_MAX
constexpr int kKnnSumBlock   = 1024;
constexpr int kKnnSummaryLen = 8;  // the handle's record: x_dc[3], r_c, rho_c, 3 unused — T each

// Launch shape, from sz alone: one target per lane for every size; as many chunks as bring the grid to about 2048 blocks, at most
// 64, at least two once there are two tiles, at most one per tile.  Boundaries: 256 | 257 bodies (one tile, one chunk | two tiles,
// two chunks) and 5888 | 5889 (one tile per chunk | several).
inline hermite_plan knn_plan_for(uint32_t sz) {
  hermite_plan p;
  p.R      = 1u;
  p.blocks = (sz + 63u) / 64u;
  p.ntiles = (sz + kHTile - 1u) / kHTile;
  uint32_t want = (2048u + p.blocks - 1u) / p.blocks;
  if (want > 64u) want = 64u;
  if (want < 2u) want = 2u;
  if (want > p.ntiles) want = p.ntiles;
  p.tiles_per_chunk = (p.ntiles + want - 1u) / want;
  p.chunks          = (p.ntiles + p.tiles_per_chunk - 1u) / p.tiles_per_chunk;
  return p;
}

// (d, j) into the ascending list by an unrolled compare-and-shift; every index is static.  LEX: lexicographic on (d2, idx) — the
// merges; otherwise strict `<` on d2 alone — the sweep, where a later record has the higher index.  A record that is not below the
// last entry changes nothing.
template <typename T, int K, bool LEX>
__device__ __forceinline__ void knn_insert(T (&ld)[K], uint32_t (&lj)[K], T d, uint32_t j) {
  bool below[K];
#pragma unroll
  for (int s = 0; s < K; ++s) below[s] = LEX ? (d < ld[s] || (d == ld[s] && j < lj[s])) : (d < ld[s]);
#pragma unroll
  for (int s = K - 1; s > 0; --s) {
    ld[s] = below[s - 1] ? ld[s - 1] : (below[s] ? d : ld[s]);
    lj[s] = below[s - 1] ? lj[s - 1] : (below[s] ? j : lj[s]);
  }
  ld[0] = below[0] ? d : ld[0];
  lj[0] = below[0] ? j : lj[0];
}

// ---- the pair batch ------------------------------------------------------------------------------------------------------------
// U records (global indices j0 ...) against the target of a lane (global index ti).  CHECK: the self pair and the records j >= n are
// masked by index; without it the slice holds neither.
template <typename T, int D, int K, int U, bool CHECK>
__device__ __forceinline__ void knn_pair_batch(T (&ld)[K], uint32_t (&lj)[K], const T (&xi)[D], uint32_t ti, const T (&s)[U][D], uint32_t j0,
                                               uint32_t n) {
  T d2[U];
#pragma unroll
  for (int b = 0; b < U; ++b) d2[b] = pair_d2<T, D>(s[b], xi);
  if constexpr (CHECK) {
#pragma unroll
    for (int b = 0; b < U; ++b) {
      const uint32_t j = j0 + uint32_t(b);
      d2[b]            = (j < n && j != ti) ? d2[b] : pair_inf<T>();
    }
  }
  T mn = d2[0];
#pragma unroll
  for (int b = 1; b < U; ++b) mn = __builtin_elementwise_min(mn, d2[b]);
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(mn < ld[K - 1]) != 0ull, 0)) {
#pragma unroll
    for (int b = 0; b < U; ++b)  // index order; a record no lane can take is skipped (its insertion would change nothing)
      if (__builtin_amdgcn_ballot_w64(d2[b] < ld[K - 1]) != 0ull) knn_insert<T, K, false>(ld, lj, d2[b], j0 + uint32_t(b));
  }
}

// One wave's slice of a tile: SUB records from src (LDS, wave-uniform addresses), global indices j0 ...
template <typename T, int D, int K, int U, bool CHECK>
__device__ __forceinline__ void knn_slice(T (&ld)[K], uint32_t (&lj)[K], const T (&xi)[D], uint32_t ti, const pair_rec<T>* src, uint32_t j0,
                                          uint32_t n) {
  constexpr int SUB = kHTile / kHWaves;
#pragma unroll 1
  for (int jj = 0; jj < SUB; jj += U) {
    T s[U][D];
#pragma unroll
    for (int b = 0; b < U; ++b)
#pragma unroll
      for (int k = 0; k < D; ++k) s[b][k] = src[jj + b].p[k];
    knn_pair_batch<T, D, K, U, CHECK>(ld, lj, xi, ti, s, j0 + uint32_t(jj), n);
  }
}

// ---- sweep ---------------------------------------------------------------------------------------------------------------------
// grid (blocks of 64 targets, chunks).  part_d: T[chunk][n][K], part_j: uint32[chunk][n][K] — a chunk's lists.
template <typename T, int D, int K>
__global__ __launch_bounds__(kHBlock) void knn_sweep_kernel(const pair_rec<T>* __restrict__ recs, T* __restrict__ part_d,
                                                            uint32_t* __restrict__ part_j, uint32_t n, uint32_t ntiles,
                                                            uint32_t tiles_per_chunk) {
  constexpr int U = sizeof(T) == 8 ? 2 : 4;  // records a batch
  constexpr size_t kTileBytes = sizeof(pair_rec<T>) * kHTile, kHandBytes = (sizeof(T) + sizeof(uint32_t)) * K * 64;
  __shared__ __attribute__((aligned(64))) unsigned char smem[kTileBytes > kHandBytes ? kTileBytes : kHandBytes];
  T* hand_d        = reinterpret_cast<T*>(smem);  // after the last tile has been consumed: one wave's lists, [K][64]
  uint32_t* hand_j = reinterpret_cast<uint32_t*>(hand_d + K * 64);

  const int lane      = threadIdx.x & 63;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));  // in an SGPR: source indices stay scalar

  const uint32_t ti = blockIdx.x * 64u + uint32_t(lane);
  T xi[D], ld[K];
  uint32_t lj[K];
  {
    const uint32_t i = ti < n ? ti : 0u;  // clamp: out-of-range lanes compute, never store
#pragma unroll
    for (int k = 0; k < D; ++k) xi[k] = recs[i].p[k];
  }
#pragma unroll
  for (int s = 0; s < K; ++s) {
    ld[s] = pair_inf<T>();
    lj[s] = kNoNeighbour;
  }
  const uint32_t own0 = blockIdx.x * 64u, own1 = own0 + 64u;  // the block's own targets

  pair_sweep_tiles<T>(recs, smem, wave, n, ntiles, tiles_per_chunk, own0, own1, [&](const pair_rec<T>* src, uint32_t j0, auto checked) {
    knn_slice<T, D, K, U, decltype(checked)::value>(ld, lj, xi, ti, src, j0, n);
  });

  // the four waves' lists, one wave at a time, lexicographically
#pragma unroll 1
  for (uint32_t p = 1; p < uint32_t(kHWaves); ++p) {
    __syncthreads();  // the last tile, or the previous wave's lists, have been read
    if (wave == p) {
#pragma unroll
      for (int s = 0; s < K; ++s) {
        hand_d[s * 64 + lane] = ld[s];
        hand_j[s * 64 + lane] = lj[s];
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int s = 0; s < K; ++s) knn_insert<T, K, true>(ld, lj, hand_d[s * 64 + lane], hand_j[s * 64 + lane]);
    }
  }
  if (wave == 0 && ti < n) {
    const uint64_t row = (uint64_t(blockIdx.y) * n + ti) * K;
#pragma unroll
    for (int s = 0; s < K; ++s) {
      part_d[row + s] = ld[s];
      part_j[row + s] = lj[s];
    }
  }
}

// The tail of a body's list, shared by the all-pairs finish and the tree walk (nntree.inc) so that both write the same bits: row i of
// idx[n][k] and d2[n][k], and rho[i].
template <typename T, int D, int K>
__device__ __forceinline__ void knn_finish_tail(const T (&ld)[K], const uint32_t (&lj)[K], const pair_rec<T>* __restrict__ recs,
                                                uint32_t* __restrict__ idx, T* __restrict__ d2, T* __restrict__ rho, uint32_t i, uint32_t n,
                                                int k) {
  T M = T(0), dk = pair_inf<T>();
  uint32_t jk = kNoNeighbour;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    if (s < k) {
      idx[uint64_t(i) * k + s] = lj[s];
      d2[uint64_t(i) * k + s]  = ld[s];
    }
    if (s < k - 1 && lj[s] < n) M += recs[lj[s]].m;  // neighbours 0 .. k - 2 in list order
    if (s == k - 1) {
      dk = ld[s];
      jk = lj[s];
    }
  }
  T r = T(0);
  if (k >= 2 && jk != kNoNeighbour) {
    if constexpr (D == 3) r = M / (T(4.18879020478639098461685784437267051) * (dk * __builtin_elementwise_sqrt(dk)));
    else r = M / (T(3.14159265358979323846264338327950288) * dk);
  }
  rho[i] = r;
}

// ---- finish --------------------------------------------------------------------------------------------------------------------
template <typename T, int D, int K>
__global__ __launch_bounds__(kHBlock) void knn_finish_kernel(const T* __restrict__ part_d, const uint32_t* __restrict__ part_j,
                                                             const pair_rec<T>* __restrict__ recs, uint32_t* __restrict__ idx,
                                                             T* __restrict__ d2, T* __restrict__ rho, uint32_t n, uint32_t chunks, int k) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= n) return;
  T ld[K];
  uint32_t lj[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    ld[s] = part_d[uint64_t(i) * K + s];
    lj[s] = part_j[uint64_t(i) * K + s];
  }
  for (uint32_t ch = 1; ch < chunks; ++ch) {
    const uint64_t row = (uint64_t(ch) * n + i) * K;
#pragma unroll
    for (int s = 0; s < K; ++s) knn_insert<T, K, true>(ld, lj, part_d[row + s], part_j[row + s]);
  }
  knn_finish_tail<T, D, K>(ld, lj, recs, idx, d2, rho, i, n, k);
}

// ---- summary -------------------------------------------------------------------------------------------------------------------
// One block.  In double for both types; every sum strided per lane, then over the wave by xor shuffles, then the waves in wave order.
template <int NV>
__device__ __forceinline__ void knn_block_sum(double (&v)[NV], double (*red)[kKnnSumBlock / 64]) {
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // red is free again
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) red[q][wave] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double t = red[q][0];
    for (int w = 1; w < kKnnSumBlock / 64; ++w) t += red[q][w];
    v[q] = t;  // every lane holds the same total
  }
}

template <typename T, int D>
__global__ __launch_bounds__(kKnnSumBlock) void knn_summary_kernel(const T* __restrict__ rho, const pair_rec<T>* __restrict__ recs,
                                                                   T* __restrict__ out, uint32_t n) {
  __shared__ double red[D + 2][kKnnSumBlock / 64];
  double a[D + 2];  // sum rho, sum rho^2, sum rho x
#pragma unroll
  for (int q = 0; q < D + 2; ++q) a[q] = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += kKnnSumBlock) {
    const double r = double(rho[i]);
    a[0] += r;
    a[1] += r * r;
#pragma unroll
    for (int k = 0; k < D; ++k) a[2 + k] += r * double(recs[i].p[k]);
  }
  knn_block_sum<D + 2>(a, red);
  double xc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) xc[k] = a[2 + k] / a[0];
  double b[1] = {0.0};  // sum rho^2 |x - x_dc|^2
  for (uint32_t i = threadIdx.x; i < n; i += kKnnSumBlock) {
    const double r = double(rho[i]);
    double q       = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double d = double(recs[i].p[k]) - xc[k];
      q += d * d;
    }
    b[0] += (r * r) * q;
  }
  knn_block_sum<1>(b, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = k < D ? T(xc[k < D ? k : 0]) : T(0);
    out[3] = T(__builtin_elementwise_sqrt(b[0] / a[1]));
    out[4] = T(a[1] / a[0]);
    out[5] = out[6] = out[7] = T(0);
  }
}

#include "nntree.inc"
#include "fof.inc"
#include "nlist.inc"

}  // namespace nbody

using namespace nbody;

// started: nbody_knn_compute has run (host call order, which a recorded step replays).  recs: pair_rec<T>[padded]; part: the chunks'
// d2 lists, T[chunks][n][K] (ALL_PAIRS only).
struct nbody_knn : hermite_handle {
  int k = 0, K = 0;
  uint32_t* part_j = nullptr;  // [chunks][n][K]: the lists' indices
  uint32_t* idx    = nullptr;  // [n][k]
  void* d2         = nullptr;  // T[n][k]
  void* rho        = nullptr;  // T[n]
  void* summary    = nullptr;  // T[kKnnSummaryLen]
  // NBODY_KNN_TREE only (nntree.inc); part and part_j stay NULL there
  int method = NBODY_KNN_ALL_PAIRS;
  nntree_structure st{};
};

namespace nbody {

template <typename T, int D, int K>
static int knn_launch(nbody_knn* h, const nbody_state* s, hipStream_t st) {
  const hermite_plan& p = h->plan;
  auto* recs            = static_cast<pair_rec<T>*>(h->recs);
  T* part_d             = static_cast<T*>(h->part);
  T* rho                = static_cast<T*>(h->rho);
  hipLaunchKernelGGL((pair_pack_kernel<T, D>), dim3(h->padded / kHBlock), dim3(kHBlock), 0, st, static_cast<const T*>(s->m),
                     static_cast<const T*>(s->x), recs, h->n, h->padded);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((knn_sweep_kernel<T, D, K>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part_d, h->part_j, h->n, p.ntiles,
                     p.tiles_per_chunk);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((knn_finish_kernel<T, D, K>), dim3((h->n + kHBlock - 1) / kHBlock), dim3(kHBlock), 0, st, part_d, h->part_j, recs,
                     h->idx, static_cast<T*>(h->d2), rho, h->n, p.chunks, h->k);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((knn_summary_kernel<T, D>), dim3(1), dim3(kKnnSumBlock), 0, st, rho, recs, static_cast<T*>(h->summary), h->n);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// The TREE method: the structure (nntree_structure_launch: pack, bounds, keys, sort, gather + bucket boxes, upper levels), walk,
// finish, summary.  The launch count follows from n alone (the sort's form does).
template <typename T, int D, int K>
static int knn_tree_launch(nbody_knn* h, const nbody_state* s, hipStream_t st) {
  const nntree_shape& t = h->st.tree;
  auto* recs            = static_cast<pair_rec<T>*>(h->recs);
  auto* sorted          = static_cast<nntree_rec<T>*>(h->st.sorted);
  auto* boxes           = static_cast<nntree_box<T>*>(h->st.boxes);
  T* rho                = static_cast<T*>(h->rho);
  const uint32_t n      = h->n;
  if (int r = nntree_structure_launch<T, D>(&h->st, s, recs, n, h->padded, st)) return r;
  hipLaunchKernelGGL((nntree_walk_kernel<T, D, K>), dim3(h->padded / kNtBlock), dim3(kNtBlock), 0, st, sorted, boxes, h->idx,
                     static_cast<T*>(h->d2), n, t.levels, t.buckets, h->k);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((nntree_finish_kernel<T, D, K>), dim3((n + kNtBlock - 1) / kNtBlock), dim3(kNtBlock), 0, st, recs, h->idx,
                     static_cast<T*>(h->d2), rho, n, h->k);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((knn_summary_kernel<T, D>), dim3(1), dim3(kKnnSumBlock), 0, st, rho, recs, static_cast<T*>(h->summary), n);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

}  // namespace nbody

extern "C" int nbody_knn_create(nbody_knn** out, int dtype, int dim, uint32_t n, int k) {
  return nbody_knn_create_on(out, dtype, dim, n, k, -1);
}

extern "C" int nbody_knn_create_on(nbody_knn** out, int dtype, int dim, uint32_t n, int k, int device) {
  return nbody_knn_create_method(out, dtype, dim, n, k, NBODY_KNN_ALL_PAIRS, device);
}

extern "C" int nbody_knn_method(const nbody_knn* h) {
  if (!h) {
    set_error("nbody_knn is NULL");
    return -1;
  }
  return h->method;
}

extern "C" int nbody_knn_create_method(nbody_knn** out, int dtype, int dim, uint32_t n, int k, int method, int device) {
  if (int r = create_check_args(out, dtype, dim, n, 1, 1u << 28, "knn needs 1 <= n <= 2^28 (got %u)")) return r;
  NB_ARG(k >= 1 && k <= kKnnMax, "knn needs 1 <= k <= %d (got %d)", kKnnMax, k);
  NB_ARG(method == NBODY_KNN_ALL_PAIRS || method == NBODY_KNN_TREE, "knn method must be 0 (all-pairs) or 1 (tree), got %d", method);
  if (int r = create_check_device(&device, "knn", true)) return r;
  device_guard guard(device);
  auto* h = new nbody_knn;
  h->k    = k;
  h->K    = k <= 4 ? 4 : k <= 8 ? 8 : 16;
  // nothing is cleared: every compute writes all of it before it reads it
  pair_handle_alloc(h, dtype, dim, n, device, knn_plan_for(n));
  h->method = method;
  if (method == NBODY_KNN_TREE) {  // what the tree path needs, and not the chunks' partial lists
    nntree_structure_alloc(&h->st, h->mem, h->tsz, n, h->padded);
  } else {
    const size_t rows = size_t(h->plan.chunks) * size_t(n) * size_t(h->K);
    h->mem.alloc(&h->part, h->tsz * rows);
    h->mem.alloc(&h->part_j, sizeof(uint32_t) * rows);
  }
  h->mem.alloc(&h->idx, sizeof(uint32_t) * size_t(n) * size_t(k));
  h->mem.alloc(&h->d2, h->tsz * size_t(n) * size_t(k));
  h->mem.alloc(&h->rho, h->tsz * size_t(n));
  h->mem.alloc(&h->summary, h->tsz * kKnnSummaryLen);
  return create_finish(out, h, nbody_knn_destroy, h->mem.error(), "nbody_knn_create allocation");
}

extern "C" void nbody_knn_destroy(nbody_knn* h) {
  if (!h) return;
  device_guard guard(h->device);
  delete h;
}

extern "C" int nbody_knn_compute(nbody_knn* h, const nbody_state* s, void* stream) {
  if (int r = pair_check_state(s, "nbody_knn_compute")) return r;
  NB_ARG(h != nullptr, "nbody_knn is NULL");
  NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
         "nbody_knn was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", h->dtype, h->dim, h->n, s->dtype,
         s->dim, s->sz);
  const hipStream_t st = as_stream(stream);
  if (int r = check_same_device(h->device, st, "nbody_knn")) return r;
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    device_guard guard(h->device);
    int r;
    if (h->method == NBODY_KNN_TREE)
      r = h->K == 4 ? knn_tree_launch<T, D, 4>(h, s, st) : h->K == 8 ? knn_tree_launch<T, D, 8>(h, s, st) : knn_tree_launch<T, D, 16>(h, s, st);
    else r = h->K == 4 ? knn_launch<T, D, 4>(h, s, st) : h->K == 8 ? knn_launch<T, D, 8>(h, s, st) : knn_launch<T, D, 16>(h, s, st);
    if (r == NBODY_OK) h->started = true;
    return r;
  });
}

extern "C" int nbody_knn_read(nbody_knn* h, int what, void* host_out, size_t bytes, void* stream) {
  NB_ARG(what >= 0 && what <= 2, "what must be 0 (idx), 1 (d2) or 2 (rho), got %d", what);
  NB_ARG(bytes != 0, "nbody_knn_read(what = %d): bytes is 0, it must be n k (idx, d2) or n (rho) elements", what);
  NB_ARG(h != nullptr, "nbody_knn is NULL");
  NB_ARG(host_out != nullptr, "host_out is NULL");
  const size_t need = what == 0 ? sizeof(uint32_t) * size_t(h->n) * size_t(h->k) : what == 1 ? h->tsz * size_t(h->n) * size_t(h->k) : h->tsz * size_t(h->n);
  NB_ARG(bytes == need, "nbody_knn_read(what = %d) needs %zu bytes, got %zu", what, need, bytes);
  const hipStream_t st = as_stream(stream);
  if (int r = pair_read_ready(h, "nbody_knn", "nbody_knn_read", "nbody_knn_compute", st)) return r;
  device_guard guard(h->device);
  const void* src = what == 0 ? static_cast<const void*>(h->idx) : what == 1 ? h->d2 : h->rho;
  NB_HIP(hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}

extern "C" int nbody_knn_density_centre(nbody_knn* h, void* centre_out, void* core_radius_out, void* core_density_out, void* stream) {
  NB_ARG(h != nullptr, "nbody_knn is NULL");
  const hipStream_t st = as_stream(stream);
  if (int r = pair_read_ready(h, "nbody_knn", "nbody_knn_density_centre", "nbody_knn_compute", st)) return r;
  device_guard guard(h->device);
  unsigned char raw[8 * kKnnSummaryLen];
  const size_t t = h->tsz;
  NB_HIP(hipMemcpyAsync(raw, h->summary, t * kKnnSummaryLen, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  if (centre_out) memcpy(centre_out, raw, t * size_t(h->dim));
  if (core_radius_out) memcpy(core_radius_out, raw + 3 * t, t);
  if (core_density_out) memcpy(core_density_out, raw + 4 * t, t);
  return NBODY_OK;
}

// ---- friends-of-friends groups (fof.inc) ---------------------------------------------------------------------------------------
// recs: pair_rec<T>[padded], original order (the catalogue's masses and positions); st: the structure nbody_knn's tree method builds
// too.  The catalogue's sort runs in the structure's keys / perm / hist, which are free once the gather has run.
struct nbody_fof : hermite_handle {
  uint32_t min_members = 1, cmax = 0, strips = 0;
  nntree_structure st{};
  uint32_t* parent    = nullptr;  // [padded], over sorted positions
  uint32_t* root      = nullptr;  // [padded]
  uint32_t* minidx    = nullptr;  // [n], by root
  uint32_t* count     = nullptr;  // [n], by root
  uint32_t* label     = nullptr;  // [n], original order
  uint32_t* size      = nullptr;  // [n], original order
  uint32_t* scount    = nullptr;  // [strips]: heads a strip, then their exclusive scan
  uint32_t* cat_label = nullptr;  // [cmax] each
  uint32_t* cat_size  = nullptr;
  uint32_t* cat_start = nullptr;
  void* cat_mass      = nullptr;  // T[cmax]
  void* cat_com       = nullptr;  // T[cmax][dim]
  uint32_t* summary   = nullptr;  // [4]
};

namespace nbody {

// init, the structure, link, flatten, labels, summary, the catalogue's sort, count, scan, scatter, sums.
template <typename T, int D>
static int fof_launch(nbody_fof* h, const nbody_state* s, T b2, hipStream_t st) {
  auto* recs       = static_cast<pair_rec<T>*>(h->recs);
  const void* sorted = h->st.sorted;  // nntree_rec<T>[padded], nntree_box<T>[2 leaves]: untyped on purpose, see the head of fof.inc
  const void* boxes  = h->st.boxes;
  const uint32_t n = h->n, mm = h->min_members;
  const dim3 padded_grid(h->padded / kNtBlock), n_grid((n + kNtBlock - 1) / kNtBlock), block(kNtBlock);
  hipLaunchKernelGGL(fof_init_kernel, padded_grid, block, 0, st, h->parent, h->minidx, h->count, n);
  NB_HIP(hipGetLastError());
  if (int r = nntree_structure_launch<T, D>(&h->st, s, recs, n, h->padded, st)) return r;
  hipLaunchKernelGGL((fof_link_kernel<T, D>), padded_grid, block, 0, st, sorted, boxes, h->parent, n, h->st.tree.levels, b2);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((fof_flatten_kernel<T>), padded_grid, block, 0, st, sorted, h->parent, h->root, h->minidx, h->count, n);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((fof_labels_kernel<T>), n_grid, block, 0, st, sorted, h->root, h->minidx, h->count, h->label, h->size, h->st.keys[0], n);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(fof_summary_kernel, dim3(1), dim3(kFofSumBlock), 0, st, h->label, h->size, n, mm, h->summary);
  NB_HIP(hipGetLastError());
  uint64_t* keys[2] = {h->st.keys[0], h->st.keys[1]};
  uint32_t* perm[2] = {h->st.perm[0], h->st.perm[1]};
  int fin           = 0;
  if (int r = radix_sort_pairs(keys, perm, n, 32, h->st.hist, st, &fin)) return r;
  hipLaunchKernelGGL(fof_cat_count_kernel, dim3(h->strips), block, 0, st, keys[fin], perm[fin], h->size, n, mm, h->scount);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(fof_cat_scan_kernel, dim3(1), dim3(kFofSumBlock), 0, st, h->scount, h->strips);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(fof_cat_scatter_kernel, dim3(h->strips), block, 0, st, keys[fin], perm[fin], h->size, n, mm, h->scount, h->cat_label,
                     h->cat_size, h->cat_start, h->cmax);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((fof_cat_sum_kernel<T, D>), dim3((h->cmax + kNtBlock / 64 - 1) / (kNtBlock / 64)), block, 0, st, recs, perm[fin], h->cat_size,
                     h->cat_start, h->summary, static_cast<T*>(h->cat_mass), static_cast<T*>(h->cat_com), h->cmax);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

}  // namespace nbody

extern "C" int nbody_fof_create(nbody_fof** out, int dtype, int dim, uint32_t n, uint32_t min_members) {
  return nbody_fof_create_on(out, dtype, dim, n, min_members, -1);
}

extern "C" int nbody_fof_create_on(nbody_fof** out, int dtype, int dim, uint32_t n, uint32_t min_members, int device) {
  if (int r = create_check_args(out, dtype, dim, n, 1, 1u << 28, "fof needs 1 <= n <= 2^28 (got %u)")) return r;
  NB_ARG(min_members >= 1 && min_members <= n, "fof needs 1 <= min_members <= n (got %u, n = %u)", min_members, n);
  if (int r = create_check_device(&device, "fof", true)) return r;
  device_guard guard(device);
  auto* h = new nbody_fof;
  // nothing is cleared: every compute writes all of it before it reads it
  pair_handle_alloc(h, dtype, dim, n, device, knn_plan_for(n));
  h->min_members = min_members;
  h->cmax        = n / min_members;  // there cannot be more groups of min_members bodies
  h->strips      = (n + kNtBlock - 1) / kNtBlock;
  nntree_structure_alloc(&h->st, h->mem, h->tsz, n, h->padded);
  h->mem.alloc(&h->parent, sizeof(uint32_t) * size_t(h->padded));
  h->mem.alloc(&h->root, sizeof(uint32_t) * size_t(h->padded));
  h->mem.alloc(&h->minidx, sizeof(uint32_t) * size_t(n));
  h->mem.alloc(&h->count, sizeof(uint32_t) * size_t(n));
  h->mem.alloc(&h->label, sizeof(uint32_t) * size_t(n));
  h->mem.alloc(&h->size, sizeof(uint32_t) * size_t(n));
  h->mem.alloc(&h->scount, sizeof(uint32_t) * size_t(h->strips));
  h->mem.alloc(&h->cat_label, sizeof(uint32_t) * size_t(h->cmax));
  h->mem.alloc(&h->cat_size, sizeof(uint32_t) * size_t(h->cmax));
  h->mem.alloc(&h->cat_start, sizeof(uint32_t) * size_t(h->cmax));
  h->mem.alloc(&h->cat_mass, h->tsz * size_t(h->cmax));
  h->mem.alloc(&h->cat_com, h->tsz * size_t(h->cmax) * size_t(dim));
  h->mem.alloc(&h->summary, sizeof(uint32_t) * 4);
  return create_finish(out, h, nbody_fof_destroy, h->mem.error(), "nbody_fof_create allocation");
}

extern "C" void nbody_fof_destroy(nbody_fof* h) {
  if (!h) return;
  device_guard guard(h->device);
  delete h;
}

extern "C" int nbody_fof_compute(nbody_fof* h, const nbody_state* s, double b, void* stream) {
  if (int r = pair_check_state(s, "nbody_fof_compute")) return r;
  NB_ARG(h != nullptr, "nbody_fof is NULL");
  NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
         "nbody_fof was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", h->dtype, h->dim, h->n, s->dtype,
         s->dim, s->sz);
  NB_ARG(b >= 0.0 && b <= DBL_MAX, "linking length b = %g must be finite and >= 0", b);
  const hipStream_t st = as_stream(stream);
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    // b is compared in double BEFORE it is converted: a finite double beyond T's range has no defined conversion to T
    NB_ARG(b <= double(sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)), "linking length b = %g: b^2 is not finite in the state's type", b);
    const T bt = T(b);
    const T b2 = bt * bt;  // rounded once in T
    NB_ARG(b2 <= (sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)), "linking length b = %g: b^2 is not finite in the state's type", b);
    if (int r = check_same_device(h->device, st, "nbody_fof")) return r;
    device_guard guard(h->device);
    const int r = fof_launch<T, D>(h, s, b2, st);
    if (r == NBODY_OK) h->started = true;
    return r;
  });
}

// the summary of the last compute, blocking (the callers have checked pair_read_ready)
static int fof_read_summary(nbody_fof* h, uint32_t (&out)[4], hipStream_t st) {
  NB_HIP(hipMemcpyAsync(out, h->summary, sizeof out, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}

extern "C" int nbody_fof_read(nbody_fof* h, int what, void* host_out, size_t bytes, void* stream) {
  NB_ARG(what >= 0 && what <= 5, "what must be 0 (label), 1 (size) or 2 .. 5 (the catalogue's label, size, mass, com), got %d", what);
  NB_ARG(h != nullptr, "nbody_fof is NULL");
  if (what <= 1) {
    NB_ARG(host_out != nullptr, "host_out is NULL");
    NB_ARG(bytes == sizeof(uint32_t) * size_t(h->n), "nbody_fof_read(what = %d) needs %zu bytes, got %zu", what, sizeof(uint32_t) * size_t(h->n), bytes);
  }
  const hipStream_t st = as_stream(stream);
  if (int r = pair_read_ready(h, "nbody_fof", "nbody_fof_read", "nbody_fof_compute", st)) return r;
  device_guard guard(h->device);
  const void* src = what == 0 ? h->label : h->size;
  if (what >= 2) {  // c entries: c is read back here (a replayed recorded compute changes it without a host call)
    uint32_t sum[4];
    if (int r = fof_read_summary(h, sum, st)) return r;
    const size_t elem = what <= 3 ? sizeof(uint32_t) : what == 4 ? h->tsz : h->tsz * size_t(h->dim);
    NB_ARG(bytes == elem * size_t(sum[1]), "nbody_fof_read(what = %d) needs %zu bytes (%u catalogued groups), got %zu", what, elem * size_t(sum[1]),
           sum[1], bytes);
    if (bytes == 0) return NBODY_OK;
    NB_ARG(host_out != nullptr, "host_out is NULL");
    src = what == 2 ? static_cast<const void*>(h->cat_label) : what == 3 ? static_cast<const void*>(h->cat_size) : what == 4 ? h->cat_mass : h->cat_com;
  }
  NB_HIP(hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}

extern "C" int nbody_fof_summary(nbody_fof* h, uint32_t* out4, void* stream) {
  NB_ARG(h != nullptr, "nbody_fof is NULL");
  NB_ARG(out4 != nullptr, "out4 is NULL");
  const hipStream_t st = as_stream(stream);
  if (int r = pair_read_ready(h, "nbody_fof", "nbody_fof_summary", "nbody_fof_compute", st)) return r;
  device_guard guard(h->device);
  uint32_t sum[4];
  if (int r = fof_read_summary(h, sum, st)) return r;
  memcpy(out4, sum, sizeof sum);
  return NBODY_OK;
}

// ---- fixed-radius neighbour lists (nlist.inc) ----------------------------------------------------------------------------------
// recs: pair_rec<T>[padded], original order (the structure's input); st: the structure nbody_knn's tree method and nbody_fof build
// too.  np: every launch shape, from (n, capacity) (nlist_plan.hpp).  started: nbody_nlist_compute has run.
struct nbody_nlist : hermite_handle {
  nlist_plan np{};
  bool has_radii = false;  // r2 holds per-body values (nbody_nlist_set_radii); else the scalar r of compute
  nntree_structure st{};
  void* r2          = nullptr;  // T[n]: r2_i in body order
  uint32_t* count   = nullptr;  // [n], body order
  uint64_t* offset  = nullptr;  // [n + 1]
  uint64_t* ssum    = nullptr;  // [strips]: the strips' sums, then their exclusive scan
  uint64_t* smax    = nullptr;  // [strips]: the strips' max of (count << 32) | ~index
  uint32_t* scratch = nullptr;  // [capacity]: the segments in ascending sorted position
  uint32_t* list    = nullptr;  // [capacity]: ... in ascending index
  uint64_t* summary = nullptr;  // [4]
};

namespace nbody {

// the structure, count walk, strip sums, scan (+ summary and status), offsets, and with a list: fill walk, segment order.
template <typename T, int D>
static int nlist_launch(nbody_nlist* h, const nbody_state* s, T r2, hipStream_t st) {
  const nlist_plan& p = h->np;
  auto* recs          = static_cast<pair_rec<T>*>(h->recs);
  const void* sorted  = h->st.sorted;  // untyped on purpose, see the head of fof.inc
  const void* boxes   = h->st.boxes;
  const T* radii      = h->has_radii ? static_cast<const T*>(h->r2) : nullptr;
  const uint32_t n = h->n, levels = h->st.tree.levels;
  const dim3 block(kNtBlock);
  if (int r = nntree_structure_launch<T, D>(&h->st, s, recs, n, h->padded, st)) return r;
  hipLaunchKernelGGL((nlist_count_kernel<T, D>), dim3(p.walk_blocks), block, 0, st, sorted, boxes, radii, r2, n, levels, h->count);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(nlist_strip_kernel, dim3(p.strips), block, 0, st, h->count, n, h->ssum, h->smax);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(nlist_scan_kernel, dim3(1), dim3(kNlScanBlock), 0, st, h->ssum, h->smax, p.strips, p.scan_trips, p.capacity, h->offset + n,
                     h->summary);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(nlist_offsets_kernel, dim3(p.strips), block, 0, st, h->count, h->ssum, n, h->offset);
  NB_HIP(hipGetLastError());
  if (!p.lists) return NBODY_OK;  // a counts-only handle
  hipLaunchKernelGGL((nlist_fill_kernel<T, D>), dim3(p.walk_blocks), block, 0, st, sorted, boxes, radii, r2, n, levels, h->offset, h->summary,
                     h->scratch, p.capacity);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(nlist_order_kernel, dim3(p.order_blocks), dim3(kNlWave), 0, st, h->count, h->offset, h->summary, h->scratch, h->list,
                     p.capacity);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// r2_i of set_radii's values into out, checked: returns the first bad index, or n
template <typename T>
static uint32_t nlist_radii_r2(const T* v, uint32_t n, bool squared, T* out) {
  for (uint32_t i = 0; i < n; ++i) {
    const T r2 = squared ? v[i] : v[i] * v[i];  // one multiply in T
    if (!(v[i] >= T(0)) || !(r2 <= (sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)))) return i;
    out[i] = r2;
  }
  return n;
}

}  // namespace nbody

extern "C" int nbody_nlist_create(nbody_nlist** out, int dtype, int dim, uint32_t n, uint64_t capacity) {
  return nbody_nlist_create_on(out, dtype, dim, n, capacity, -1);
}

extern "C" int nbody_nlist_create_on(nbody_nlist** out, int dtype, int dim, uint32_t n, uint64_t capacity, int device) {
  if (int r = create_check_args(out, dtype, dim, n, 1, kNlMaxN, "nlist needs 1 <= n <= 2^28 (got %u)")) return r;
  NB_ARG(capacity <= kNlMaxCapacity, "nlist needs capacity <= 2^32 list entries (got %llu)", static_cast<unsigned long long>(capacity));
  if (int r = create_check_device(&device, "nlist", true)) return r;
  device_guard guard(device);
  auto* h = new nbody_nlist;
  // nothing is cleared: every compute writes all it later reads
  pair_handle_alloc(h, dtype, dim, n, device, knn_plan_for(n));
  nlist_plan_for(n, capacity, &h->np);  // in range: checked above
  nntree_structure_alloc(&h->st, h->mem, h->tsz, n, h->padded);
  h->mem.alloc(&h->r2, h->tsz * size_t(n));
  h->mem.alloc(&h->count, sizeof(uint32_t) * size_t(n));
  h->mem.alloc(&h->offset, sizeof(uint64_t) * (size_t(n) + 1));
  h->mem.alloc(&h->ssum, sizeof(uint64_t) * size_t(h->np.strips));
  h->mem.alloc(&h->smax, sizeof(uint64_t) * size_t(h->np.strips));
  if (h->np.lists) {
    h->mem.alloc(&h->scratch, sizeof(uint32_t) * size_t(capacity));
    h->mem.alloc(&h->list, sizeof(uint32_t) * size_t(capacity));
  }
  h->mem.alloc(&h->summary, sizeof(uint64_t) * 4);
  return create_finish(out, h, nbody_nlist_destroy, h->mem.error(), "nbody_nlist_create allocation");
}

extern "C" void nbody_nlist_destroy(nbody_nlist* h) {
  if (!h) return;
  device_guard guard(h->device);
  delete h;
}

extern "C" int nbody_nlist_set_radii(nbody_nlist* h, const void* host_values, size_t bytes, int squared, void* stream) {
  NB_ARG(h != nullptr, "nbody_nlist is NULL");
  const bool clear = host_values == nullptr && bytes == 0;
  if (!clear) {
    NB_ARG(host_values != nullptr, "host_values is NULL");
    NB_ARG(bytes == h->tsz * size_t(h->n), "nbody_nlist_set_radii needs %zu bytes (n values of the handle's type), got %zu", h->tsz * size_t(h->n), bytes);
    NB_ARG(squared == 0 || squared == 1, "squared must be 0 or 1, got %d", squared);
  }
  const hipStream_t st = as_stream(stream);
  if (int r = check_same_device(h->device, st, "nbody_nlist")) return r;
  if (capture_id(st) != 0) {
    set_error("nbody_nlist_set_radii is blocking: it cannot be recorded (call it outside nbody_graph_begin/end)");
    return NBODY_ERR_STATE;
  }
  if (clear) {
    h->has_radii = false;
    return NBODY_OK;
  }
  // every r2_i on the host, checked before anything is copied
  std::vector<unsigned char> r2(bytes);
  const uint32_t bad = h->dtype == NBODY_F32 ? nlist_radii_r2(static_cast<const float*>(host_values), h->n, squared != 0, reinterpret_cast<float*>(r2.data()))
                                             : nlist_radii_r2(static_cast<const double*>(host_values), h->n, squared != 0, reinterpret_cast<double*>(r2.data()));
  if (bad != h->n) {
    const double v = h->dtype == NBODY_F32 ? double(static_cast<const float*>(host_values)[bad]) : static_cast<const double*>(host_values)[bad];
    NB_ARG(false, "nbody_nlist_set_radii: value %g at index %u: every radius must be >= 0 and its square finite in the handle's type", v, bad);
  }
  device_guard guard(h->device);
  NB_HIP(hipMemcpyAsync(h->r2, r2.data(), bytes, hipMemcpyHostToDevice, st));
  NB_HIP(hipStreamSynchronize(st));
  h->has_radii = true;
  return NBODY_OK;
}

extern "C" int nbody_nlist_compute(nbody_nlist* h, const nbody_state* s, double r, void* stream) {
  if (int rc = pair_check_state(s, "nbody_nlist_compute")) return rc;
  NB_ARG(h != nullptr, "nbody_nlist is NULL");
  NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
         "nbody_nlist was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", h->dtype, h->dim, h->n, s->dtype,
         s->dim, s->sz);
  if (!h->has_radii) NB_ARG(r >= 0.0 && r <= DBL_MAX, "radius r = %g must be finite and >= 0", r);
  const hipStream_t st = as_stream(stream);
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    T r2 = T(0);
    if (!h->has_radii) {
      // r is compared in double BEFORE it is converted: a finite double beyond T's range has no defined conversion to T
      NB_ARG(r <= double(sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)), "radius r = %g: r^2 is not finite in the state's type", r);
      const T rt = T(r);
      r2         = rt * rt;  // rounded once in T
      NB_ARG(r2 <= (sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)), "radius r = %g: r^2 is not finite in the state's type", r);
    }
    if (int rc = check_same_device(h->device, st, "nbody_nlist")) return rc;
    device_guard guard(h->device);
    const int rc = nlist_launch<T, D>(h, s, r2, st);
    if (rc == NBODY_OK) h->started = true;
    return rc;
  });
}

// the summary of the last compute, blocking (the callers have checked pair_read_ready)
static int nlist_read_summary(nbody_nlist* h, uint64_t (&out)[4], hipStream_t st) {
  NB_HIP(hipMemcpyAsync(out, h->summary, sizeof out, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}

extern "C" int nbody_nlist_read(nbody_nlist* h, int what, void* host_out, size_t bytes, void* stream) {
  NB_ARG(what >= 0 && what <= 2, "what must be 0 (count), 1 (offset) or 2 (list), got %d", what);
  NB_ARG(h != nullptr, "nbody_nlist is NULL");
  if (what <= 1) {
    const size_t need = what == 0 ? sizeof(uint32_t) * size_t(h->n) : sizeof(uint64_t) * (size_t(h->n) + 1);
    NB_ARG(host_out != nullptr, "host_out is NULL");
    NB_ARG(bytes == need, "nbody_nlist_read(what = %d) needs %zu bytes, got %zu", what, need, bytes);
  }
  const hipStream_t st = as_stream(stream);
  if (int r = pair_read_ready(h, "nbody_nlist", "nbody_nlist_read", "nbody_nlist_compute", st)) return r;
  device_guard guard(h->device);
  const void* src = what == 0 ? static_cast<const void*>(h->count) : static_cast<const void*>(h->offset);
  if (what == 2) {  // total entries: the total is read back here (a replayed recorded compute changes it without a host call)
    uint64_t sum[4];
    if (int r = nlist_read_summary(h, sum, st)) return r;
    if (sum[3] != 0) {
      if (sum[3] & kNlStatusPerBody)
        set_error("nbody_nlist_read: no list was produced: the largest count %llu (body %llu) exceeds NBODY_NLIST_MAX_PER_BODY = %u",
                  static_cast<unsigned long long>(sum[1]), static_cast<unsigned long long>(sum[2]), kNlMaxPerBody);
      else
        set_error("nbody_nlist_read: no list was produced: it needs %llu entries, the handle's capacity is %llu",
                  static_cast<unsigned long long>(sum[0]), static_cast<unsigned long long>(h->np.capacity));
      return NBODY_ERR_STATE;
    }
    NB_ARG(bytes == sizeof(uint32_t) * size_t(sum[0]), "nbody_nlist_read(what = 2) needs %zu bytes (%llu entries), got %zu",
           sizeof(uint32_t) * size_t(sum[0]), static_cast<unsigned long long>(sum[0]), bytes);
    if (bytes == 0) return NBODY_OK;
    NB_ARG(host_out != nullptr, "host_out is NULL");
    src = h->list;
  }
  NB_HIP(hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}

extern "C" int nbody_nlist_summary(nbody_nlist* h, uint64_t* out4, void* stream) {
  NB_ARG(h != nullptr, "nbody_nlist is NULL");
  NB_ARG(out4 != nullptr, "out4 is NULL");
  const hipStream_t st = as_stream(stream);
  if (int r = pair_read_ready(h, "nbody_nlist", "nbody_nlist_summary", "nbody_nlist_compute", st)) return r;
  device_guard guard(h->device);
  uint64_t sum[4];
  if (int r = nlist_read_summary(h, sum, st)) return r;
  memcpy(out4, sum, sizeof sum);
  return NBODY_OK;
}
