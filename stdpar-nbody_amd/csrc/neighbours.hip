// All-pairs per-body potentials, nearest neighbours and the closest pair: nbody_neighbours_* of include/nbody_hip.h.
// No reference counterpart.  Reads a state's (m, x), changes nothing in it; Plummer softening required for the potential (eps = 0 is
// refused: the unsoftened potential's pair is the reference's m / (|d| + eps(T)), a different form).
//
// Definitions (T the state's type, D its dimension, e2 = fl_T(T(eps) * T(eps)), d = x_j - x_i):
//   d2_ij   the UNSOFTENED squared distance, pair_d2 of pair_sweep.hpp: one FMA chain in component order, bitwise symmetric in (i, j).
//   q_ij    d2_ij + e2 (one rounding).
//   phi_i   -c S_i, S_i = sum_{j != i} m_j / sqrt(q_ij).  The self pair is excluded BY INDEX (its term would be m_i / eps, not 0);
//           coincident distinct bodies contribute m_j / eps.  One reciprocal square root per pair: v_rsq_f64 polished to third order
//           (y (1 + e/2 + 3/8 e^2), e = 1 - q y^2) in double, the bare 1-ulp v_rsq_f32 in float — energy.hip's softened pair,
//           operation for operation.  No divide, no sqrt.
//   nn_i    the j != i with the smallest computed d2_ij, the LOWEST index among equal values; nnd2_i that d2.  Selection is on the
//           unsoftened d2, so nn and nnd2 have the same bits for every valid eps.  n = 1: nn = 0xffffffff, nnd2 = +inf, phi = 0.
//   closest pair   the (i, j), i < j, with the smallest d2, ties to the lowest i, then the lowest j: by the symmetry of d2 the body
//           of lowest index among those with minimal nnd2, with its nn.  n = 1: (0xffffffff, 0xffffffff, +inf).
//
// Four launches per compute, all on the caller's stream, nothing allocated after nbody_neighbours_create:
//   pack     pair_sweep.hpp's: one lane per record {x[3], m}, padded with zero-mass records at the origin to whole tiles.  A padding
//            record adds m y = 0 to S; it never becomes a neighbour because of an INDEX BOUND: every slice of 64 records that
//            reaches past n runs the checked batch body below, which replaces the d2 of a record j >= n by +inf.
//   sweep    the hot path, over pair_sweep_tiles of pair_sweep.hpp (the Hermite sweeps' shape): R targets per lane in registers,
//            the tiles cut over grid.y chunks by hermite_plan_for(sz, 2) — the sixth order's plan: a function of sz alone; what
//            is here is the pair batch, the slice and the merge of the block's waves.  A lane carries S, the running minimum of d2
//            and its index.  The terms of a slice (64 records) are summed by themselves, in U interleaved
//            chains joined pairwise, and the slice sums added up: one chain over a chunk lets a large term swallow the later ones
//            (energy.hip: 8.4e-6 of the potential at N = 65 537 in float).
//            Selection: a batch of U records takes U - 1 v_min and ONE compare of the batch's minimum against the running one per
//            target; only if some lane of the wave found a closer record (one scalar branch; a lane's minimum falls about ln(n)
//            times in all) do the lanes walk the batch in index order, min and 32-bit select under the compare's mask.  The result
//            is the same whichever way the branch goes.  The source index is wave-uniform (the wave number is read with
//            v_readfirstlane), so the walk compares against and selects from a scalar.
//            Two batch bodies, chosen per slice by pair_sweep_tiles: the CHECKED one masks the self pair (term 0, d2 +inf) and the
//            padding (d2 +inf) by index and runs only for slices that overlap the block's own targets or reach past n — at most two
//            of a wave's slices per chunk; every other slice runs the plain body, which has no index test at all.
//            The block's waves merge through LDS: S added in wave order, (d2, index) lexicographically — a wave's slice of a later
//            tile holds higher indices than another wave's slice of an earlier tile, so `<` on d2 alone would not keep the lowest
//            index.  The chunk's raw results go to the partial arrays.
//   finish   one lane per body: the chunks' S added IN CHUNK ORDER and scaled by -c, the chunks' (d2, index) merged by the same
//            rule; writes phi, nn, nnd2.
//   closest  one block: the lexicographic minimum of (nnd2, i) over the bodies, strided per lane, then across the wave and the
//            block — a minimum does not depend on the order it is taken in, no atomics — into the handle's record.
// The rounding order of S_i (chains of a slice, slices of a tile by wave, tiles in order, waves in order, chunks in order) follows
// from sz alone — nothing is read from the device or the CU count, no atomics, no waiting between blocks — and nn has an exact tie
// rule: two runs, an eager call and a replayed recorded one, and a handle destroyed and made again give the same bits.
// Bound: FP64 / FP32 VALU issue, like the Hermite sweeps; per pair D subtractions, D chain operations, one add, the weight (5 + rsq
// in double, 1 + rsq in float), one add into the slice sum and (U - 1) / U min + 1 / U compare.
#include "pair_sweep.hpp"

// every product that is meant to be fused below is written as an fma: m y in float rounds before it is added, whichever batch body
// (with or without the self pair's select between the two) a slice runs
#pragma clang fp contract(off)

namespace nbody {

constexpr int kNbClosestBlock = 1024;

template <typename T>
struct nb_closest_rec {  // the handle's closest-pair record
  T d2;
  uint32_t i, j;
};

template <typename T>
struct nb_consts {
  T k0375;
  __device__ __forceinline__ nb_consts() : k0375(T(0.375)) { asm volatile("" : "+s"(k0375)); }  // not an inline constant
};

// ---- the pair batch ------------------------------------------------------------------------------------------------------------
// U records (global indices j0 ...) against the R targets of a lane (global indices ti[r]).  ls[b][r]: the slice's U sum chains.
// CHECK: the self pair and the records j >= n are masked by index; without it the slice holds neither.
template <typename T, int D, int R, int U, bool CHECK>
__device__ __forceinline__ void nb_pair_batch(T (&ls)[U][R], T (&best)[R], uint32_t (&idx)[R], const T (&xi)[R][D], const uint32_t (&ti)[R],
                                              const pair_rec<T> (&s)[U], uint32_t j0, uint32_t n, const nb_consts<T>& pc, T e2) {
  T d2[U][R], w[U][R];
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r) d2[b][r] = pair_d2<T, D>(s[b].p, xi[r]);
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const T q = d2[b][r] + e2;
      if constexpr (sizeof(T) == 8) {  // y (1 + e/2 + 3/8 e^2), e = 1 - q y^2: the 2^-24 seed to third order
        const T y  = __builtin_amdgcn_rsq(q);
        const T e  = __builtin_fma(-q, y * y, 1.0);
        const T p  = __builtin_fma(e, pc.k0375, 0.5);
        const T my = s[b].m * y;
        w[b][r]    = __builtin_fma(my, p * e, my);
      } else {
        w[b][r] = s[b].m * __builtin_amdgcn_rsqf(q);
      }
    }
  if constexpr (CHECK) {
#pragma unroll
    for (int b = 0; b < U; ++b) {
      const uint32_t j = j0 + uint32_t(b);
      const bool real  = j < n;  // wave-uniform
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool self = j == ti[r];
        w[b][r]         = self ? T(0) : w[b][r];
        d2[b][r]        = (real && !self) ? d2[b][r] : pair_inf<T>();
      }
    }
  }
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r) ls[b][r] += w[b][r];
  // the batch's minimum against the running one: one compare per target, the walk only where some lane found a closer record
  bool closer = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    T mn = d2[0][r];
#pragma unroll
    for (int b = 1; b < U; ++b) mn = __builtin_elementwise_min(mn, d2[b][r]);
    closer = closer | (mn < best[r]);
  }
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(closer) != 0ull, 0)) {
#pragma unroll
    for (int b = 0; b < U; ++b)  // index order: `<` keeps the lowest index among equal values
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool take = d2[b][r] < best[r];
        best[r]         = __builtin_elementwise_min(best[r], d2[b][r]);
        idx[r]          = take ? j0 + uint32_t(b) : idx[r];
      }
  }
}

// One wave's slice of a tile: SUB records from src (LDS, wave-uniform addresses), global indices j0 ...; adds the slice's sum to S.
template <typename T, int D, int R, int U, bool CHECK>
__device__ __forceinline__ void nb_slice(T (&S)[R], T (&best)[R], uint32_t (&idx)[R], const T (&xi)[R][D], const uint32_t (&ti)[R],
                                         const pair_rec<T>* src, uint32_t j0, uint32_t n, const nb_consts<T>& pc, T e2) {
  constexpr int SUB = kHTile / kHWaves;
  T ls[U][R];
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r) ls[b][r] = T(0);
#pragma unroll 1
  for (int jj = 0; jj < SUB; jj += U) {
    pair_rec<T> s[U];  // field by field: a struct copy may be left in private memory by the compiler
#pragma unroll
    for (int b = 0; b < U; ++b) {
#pragma unroll
      for (int k = 0; k < D; ++k) s[b].p[k] = src[jj + b].p[k];
      s[b].m = src[jj + b].m;
    }
    nb_pair_batch<T, D, R, U, CHECK>(ls, best, idx, xi, ti, s, j0 + uint32_t(jj), n, pc, e2);
  }
  // the U chains pairwise: (0 + 1) + (2 + 3)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    T t;
    if constexpr (U == 4) t = (ls[0][r] + ls[1][r]) + (ls[2][r] + ls[3][r]);
    else if constexpr (U == 2) t = ls[0][r] + ls[1][r];
    else t = ls[0][r];
    S[r] += t;
  }
}

// ---- sweep ---------------------------------------------------------------------------------------------------------------------
// grid (blocks of 64 R targets, chunks).  part_s, part_d: T[chunk][n], part_j: uint32[chunk][n] — a chunk's raw S, minimum and index.
template <typename T, int D, int R>
__global__ __launch_bounds__(kHBlock) void neighbours_sweep_kernel(const pair_rec<T>* __restrict__ recs, T* __restrict__ part_s,
                                                                   T* __restrict__ part_d, uint32_t* __restrict__ part_j, T e2, uint32_t n,
                                                                   uint32_t ntiles, uint32_t tiles_per_chunk) {
  constexpr int U  = (sizeof(T) == 8 ? 2 : 4) / R;  // records a batch: 2 pairs in flight per lane in double, 4 in float
  constexpr int NH = (kHWaves - 1) * R * 64;        // the other waves' results, handed over through LDS
  constexpr size_t kTileBytes = sizeof(pair_rec<T>) * kHTile, kHandBytes = (2 * sizeof(T) + sizeof(uint32_t)) * NH;
  __shared__ __attribute__((aligned(64))) unsigned char smem[kTileBytes > kHandBytes ? kTileBytes : kHandBytes];
  T* hand_s        = reinterpret_cast<T*>(smem);  // after the last tile has been consumed
  T* hand_d        = hand_s + NH;
  uint32_t* hand_j = reinterpret_cast<uint32_t*>(hand_d + NH);

  const int lane      = threadIdx.x & 63;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));  // in an SGPR: source indices stay scalar

  T xi[R][D], S[R], best[R];
  uint32_t ti[R], idx[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ti[r]            = blockIdx.x * (64 * R) + r * 64 + lane;
    const uint32_t i = ti[r] < n ? ti[r] : 0u;  // clamp: out-of-range lanes compute, never store
#pragma unroll
    for (int k = 0; k < D; ++k) xi[r][k] = recs[i].p[k];
    S[r]    = T(0);
    best[r] = pair_inf<T>();
    idx[r]  = kNoNeighbour;
  }
  const uint32_t own0 = blockIdx.x * (64 * R), own1 = own0 + 64 * R;  // the block's own targets

  const nb_consts<T> pc;
  pair_sweep_tiles<T>(recs, smem, wave, n, ntiles, tiles_per_chunk, own0, own1, [&](const pair_rec<T>* src, uint32_t j0, auto checked) {
    nb_slice<T, D, R, U, decltype(checked)::value>(S, best, idx, xi, ti, src, j0, n, pc, e2);
  });

  // the four slices: S in wave order, (d2, index) lexicographically
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int slot = ((int(wave) - 1) * R + r) * 64 + lane;
      hand_s[slot]   = S[r];
      hand_d[slot]   = best[r];
      hand_j[slot]   = idx[r];
    }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int p = 1; p < kHWaves; ++p)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int slot = ((p - 1) * R + r) * 64 + lane;
        S[r] += hand_s[slot];
        pair_merge<T>(best[r], idx[r], hand_d[slot], hand_j[slot]);
      }
    const uint64_t row = uint64_t(blockIdx.y) * n;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (ti[r] < n) {
        part_s[row + ti[r]] = S[r];
        part_d[row + ti[r]] = best[r];
        part_j[row + ti[r]] = idx[r];
      }
    }
  }
}

// ---- finish --------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kHBlock) void neighbours_finish_kernel(const T* __restrict__ part_s, const T* __restrict__ part_d,
                                                                    const uint32_t* __restrict__ part_j, T* __restrict__ phi,
                                                                    uint32_t* __restrict__ nn, T* __restrict__ nnd2, T c, uint32_t n,
                                                                    uint32_t chunks) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= n) return;
  T S = part_s[i], best = part_d[i];
  uint32_t idx = part_j[i];
  for (uint32_t ch = 1; ch < chunks; ++ch) {
    const uint64_t e = uint64_t(ch) * n + i;
    S += part_s[e];
    pair_merge<T>(best, idx, part_d[e], part_j[e]);
  }
  phi[i]  = -c * S;
  nn[i]   = idx;
  nnd2[i] = best;
}

// ---- closest -------------------------------------------------------------------------------------------------------------------
// One block.  The lexicographic minimum of (nnd2_i, i); its body's nn is the pair's j.  A body without a neighbour (n = 1) gives
// (0xffffffff, 0xffffffff, +inf).
template <typename T>
__global__ __launch_bounds__(kNbClosestBlock) void neighbours_closest_kernel(const T* __restrict__ nnd2, const uint32_t* __restrict__ nn,
                                                                             nb_closest_rec<T>* __restrict__ out, uint32_t n) {
  __shared__ T red_d[kNbClosestBlock / 64];
  __shared__ uint32_t red_i[kNbClosestBlock / 64];
  T best       = pair_inf<T>();
  uint32_t idx = kNoNeighbour;
  for (uint32_t i = threadIdx.x; i < n; i += kNbClosestBlock) pair_merge<T>(best, idx, nnd2[i], i);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T od        = __shfl_xor(best, off, 64);
    const uint32_t oi = __shfl_xor(idx, off, 64);
    pair_merge<T>(best, idx, od, oi);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red_d[wave] = best;
    red_i[wave] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kNbClosestBlock / 64; ++w) pair_merge<T>(best, idx, red_d[w], red_i[w]);
    nb_closest_rec<T> r;
    const uint32_t j = idx < n ? nn[idx] : kNoNeighbour;
    r.d2             = best;
    r.i              = j == kNoNeighbour ? kNoNeighbour : idx;
    r.j              = j;
    *out             = r;
  }
}

}  // namespace nbody

using namespace nbody;

// started: nbody_neighbours_compute has run (host call order, which a recorded step replays).  recs: pair_rec<T>[padded]; part: the
// chunks' S, T[chunks][n].
struct nbody_neighbours : hermite_handle {
  void* part_d     = nullptr;  // T[chunks][n]: the chunks' minimum d2
  uint32_t* part_j = nullptr;  // [chunks][n]: its index
  void* phi        = nullptr;  // T[n]
  uint32_t* nn     = nullptr;  // [n]
  void* nnd2       = nullptr;  // T[n]
  void* closest    = nullptr;  // nb_closest_rec<T>
};

namespace nbody {

template <typename T, int D, int R>
static int neighbours_launch(nbody_neighbours* h, const nbody_state* s, T e2, hipStream_t st) {
  const hermite_plan& p = h->plan;
  auto* recs            = static_cast<pair_rec<T>*>(h->recs);
  T* part_s             = static_cast<T*>(h->part);
  T* part_d             = static_cast<T*>(h->part_d);
  T* nnd2               = static_cast<T*>(h->nnd2);
  hipLaunchKernelGGL((pair_pack_kernel<T, D>), dim3(h->padded / kHBlock), dim3(kHBlock), 0, st, static_cast<const T*>(s->m),
                     static_cast<const T*>(s->x), recs, h->n, h->padded);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((neighbours_sweep_kernel<T, D, R>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part_s, part_d, h->part_j,
                     e2, h->n, p.ntiles, p.tiles_per_chunk);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((neighbours_finish_kernel<T>), dim3((h->n + kHBlock - 1) / kHBlock), dim3(kHBlock), 0, st, part_s, part_d, h->part_j,
                     static_cast<T*>(h->phi), h->nn, nnd2, static_cast<T>(s->c), h->n, p.chunks);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((neighbours_closest_kernel<T>), dim3(1), dim3(kNbClosestBlock), 0, st, nnd2, h->nn,
                     static_cast<nb_closest_rec<T>*>(h->closest), h->n);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

}  // namespace nbody

extern "C" int nbody_neighbours_create(nbody_neighbours** out, int dtype, int dim, uint32_t n) {
  return nbody_neighbours_create_on(out, dtype, dim, n, -1);
}

extern "C" int nbody_neighbours_create_on(nbody_neighbours** out, int dtype, int dim, uint32_t n, int device) {
  if (int r = create_check_args(out, dtype, dim, n, 1, 1u << 28, "neighbours needs 1 <= n <= 2^28 (got %u)")) return r;
  if (int r = create_check_device(&device, "neighbours", true)) return r;
  device_guard guard(device);
  auto* h = new nbody_neighbours;
  // nothing is cleared: every compute writes all of it before it reads it
  pair_handle_alloc(h, dtype, dim, n, device, hermite_plan_for(n, 2));
  const size_t rows = size_t(h->plan.chunks) * size_t(n);
  h->mem.alloc(&h->part, h->tsz * rows);
  h->mem.alloc(&h->part_d, h->tsz * rows);
  h->mem.alloc(&h->part_j, sizeof(uint32_t) * rows);
  h->mem.alloc(&h->phi, h->tsz * size_t(n));
  h->mem.alloc(&h->nn, sizeof(uint32_t) * size_t(n));
  h->mem.alloc(&h->nnd2, h->tsz * size_t(n));
  h->mem.alloc(&h->closest, 16);
  return create_finish(out, h, nbody_neighbours_destroy, h->mem.error(), "nbody_neighbours_create allocation");
}

extern "C" void nbody_neighbours_destroy(nbody_neighbours* h) {
  if (!h) return;
  device_guard guard(h->device);
  delete h;
}

extern "C" int nbody_neighbours_compute(nbody_neighbours* h, const nbody_state* s, double eps, void* stream) {
  if (int r = pair_check_state(s, "nbody_neighbours_compute")) return r;
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    T e2;
    if (int r = hermite_check_call<T>(h, s, eps, as_stream(stream), "nbody_neighbours", "nbody_neighbours_compute", nullptr, &e2)) return r;
    device_guard guard(h->device);
    const int r = h->plan.R == 2 ? neighbours_launch<T, D, 2>(h, s, e2, as_stream(stream)) : neighbours_launch<T, D, 1>(h, s, e2, as_stream(stream));
    if (r == NBODY_OK) h->started = true;
    return r;
  });
}

extern "C" int nbody_neighbours_read(nbody_neighbours* h, int what, void* host_out, size_t bytes, void* stream) {
  NB_ARG(what >= 0 && what <= 2, "what must be 0 (phi), 1 (nn) or 2 (nnd2), got %d", what);
  NB_ARG(bytes != 0, "nbody_neighbours_read(what = %d): bytes is 0, it must be n elements", what);
  NB_ARG(h != nullptr, "nbody_neighbours is NULL");
  NB_ARG(host_out != nullptr, "host_out is NULL");
  const size_t need = (what == 1 ? sizeof(uint32_t) : h->tsz) * size_t(h->n);
  NB_ARG(bytes == need, "nbody_neighbours_read(what = %d) needs %zu bytes, got %zu", what, need, bytes);
  const hipStream_t st = as_stream(stream);
  if (int r = pair_read_ready(h, "nbody_neighbours", "nbody_neighbours_read", "nbody_neighbours_compute", st)) return r;
  device_guard guard(h->device);
  const void* src = what == 0 ? h->phi : what == 1 ? static_cast<const void*>(h->nn) : h->nnd2;
  NB_HIP(hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}

extern "C" int nbody_neighbours_closest_pair(nbody_neighbours* h, uint32_t* i, uint32_t* j, void* d2_out, void* stream) {
  NB_ARG(h != nullptr, "nbody_neighbours is NULL");
  const hipStream_t st = as_stream(stream);
  if (int r = pair_read_ready(h, "nbody_neighbours", "nbody_neighbours_closest_pair", "nbody_neighbours_compute", st)) return r;
  device_guard guard(h->device);
  unsigned char raw[16];
  NB_HIP(hipMemcpyAsync(raw, h->closest, sizeof raw, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  uint32_t ij[2];
  if (h->dtype == NBODY_F64) {
    nb_closest_rec<double> r;
    memcpy(&r, raw, sizeof r);
    ij[0] = r.i, ij[1] = r.j;
    if (d2_out) *static_cast<double*>(d2_out) = r.d2;
  } else {
    nb_closest_rec<float> r;
    memcpy(&r, raw, sizeof r);
    ij[0] = r.i, ij[1] = r.j;
    if (d2_out) *static_cast<float*>(d2_out) = r.d2;
  }
  if (i) *i = ij[0];
  if (j) *j = ij[1];
  return NBODY_OK;
}
