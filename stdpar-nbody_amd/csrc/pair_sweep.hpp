// What the all-pairs diagnostics of neighbours.hip (potentials, nearest neighbour, closest pair) and knn.hip (k nearest neighbours,
// local densities) share: the packed source record and its pack kernel, the unsoftened squared distance, the "no neighbour" values,
// the lexicographic (d2, index) merge, the tiled sweep over the source records and the host-side checks of the two handles.  The next
// diagnostic of this kind (a count within a radius, a mass-weighted list) brings its pair batch and its merge, nothing of this file.
//
// The sweep has the Hermite pair sum's shape (hermite_tile.hpp, whose tile, block and plan it uses): targets in registers, records
// staged through LDS tiles of kHTile and read as wave-uniform broadcasts, every tile cut over the four waves of the block, the tiles
// cut over grid.y chunks.  What a lane carries, what a slice of 64 records does to it and how the waves and chunks are merged are the
// caller's.  Unlike the Hermite sums a selection must keep the self pair and the padding records out BY INDEX (their d2 is 0, or the
// distance to the origin: both are valid distances); pair_sweep_tiles decides per slice whether any such record can be in it.
#pragma once
#include <type_traits>

#include "hermite_tile.hpp"

namespace nbody {

constexpr uint32_t kNoNeighbour = 0xffffffffu;  // the index where a body has no (further) neighbour; its d2 is +inf

template <typename T>
__device__ __forceinline__ T pair_inf() {
  return __builtin_huge_val();
}

// Source record: {x[3], m}, D components used.  32 B in double (two ds_read_b128), 16 B in float (one).  kNN's sweep does not read
// the mass; its finish takes it from here.
template <typename T>
struct alignas(sizeof(T) * 4) pair_rec {
  T p[3];
  T m;
};

// (d2, j) < (best, idx) lexicographically
template <typename T>
__device__ __forceinline__ void pair_merge(T& best, uint32_t& idx, T d2, uint32_t j) {
  const bool take = d2 < best || (d2 == best && j < idx);
  best            = take ? d2 : best;
  idx             = take ? j : idx;
}

// The UNSOFTENED squared distance of a source at pj from a target at xi, d = pj - xi, as one FMA chain in component order: t = d_0 d_0,
// then t = fma(d_k, d_k, t).  Bitwise symmetric in (i, j) — x_i - x_j is the exact negation of x_j - x_i — which is what lets the
// closest pair be read off the nearest neighbours, and what makes neighbours' nnd2 and kNN's first d2 the same bits.
template <typename T, int D>
__device__ __forceinline__ T pair_d2(const T* pj, const T (&xi)[D]) {
#pragma clang fp contract(off)
  T d[D];
#pragma unroll
  for (int k = 0; k < D; ++k) d[k] = pj[k] - xi[k];
  T t = d[0] * d[0];
#pragma unroll
  for (int k = 1; k < D; ++k) t = __builtin_elementwise_fma(d[k], d[k], t);
  return t;
}

// ---- pack ----------------------------------------------------------------------------------------------------------------------
// One lane per record; 2D zero-fills component 2.  padded: n rounded up to whole tiles.
template <typename T, int D>
static __global__ __launch_bounds__(kHBlock) void pair_pack_kernel(const T* __restrict__ m, const T* __restrict__ x, pair_rec<T>* __restrict__ recs,
                                                                   uint32_t n, uint32_t padded) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= padded) return;
  pair_rec<T> r;
  r.p[0] = r.p[1] = r.p[2] = r.m = T(0);  // padding: zero mass at the origin (kept out of a selection by the index bound of the checked slices)
  if (i < n) {
    r.m = m[i];
#pragma unroll
    for (int k = 0; k < D; ++k) r.p[k] = x[uint64_t(i) * D + k];
  }
  recs[i] = r;
}

// ---- the tile sweep ------------------------------------------------------------------------------------------------------------
// The source loop of a sweep kernel, block (kHBlock), grid (blocks of targets, chunks): the tiles of chunk blockIdx.y, each staged
// through smem (sizeof(pair_rec<T>) * kHTile bytes, aligned to a record; free again when the call returns, after a barrier of the
// caller's) while the next is in flight, and for each the slice of this wave (`wave`: wave-uniform, best in an SGPR) handed to
//   slice(src, j0, checked)   src: the slice's kHTile / kHWaves records in LDS, wave-uniform addresses; j0: the index of the first;
//                             checked: std::true_type if the slice may hold a target of this block, [own0, own1) — the self pair —
//                             or a record past n — padding —, and the body must mask both by index; std::false_type if it holds
//                             neither, so the body needs no index test at all.
// At most two of a wave's slices per chunk are checked.
template <typename T, typename F>
__device__ __forceinline__ void pair_sweep_tiles(const pair_rec<T>* __restrict__ recs, unsigned char* smem, uint32_t wave, uint32_t n,
                                                 uint32_t ntiles, uint32_t tiles_per_chunk, uint32_t own0, uint32_t own1, const F& slice) {
  constexpr int SUB       = kHTile / kHWaves;  // records of a tile one wave takes
  const pair_rec<T>* tile = reinterpret_cast<const pair_rec<T>*>(smem);
  T* tflat                = reinterpret_cast<T*>(smem);

  const uint32_t t0 = blockIdx.y * tiles_per_chunk;
  const uint32_t t1 = t0 + tiles_per_chunk < ntiles ? t0 + tiles_per_chunk : ntiles;

  const T* flat = reinterpret_cast<const T*>(recs);
  T stage[4];  // one record per lane, value by value
  auto stage_load = [&](uint32_t t) {  // the record array is padded to whole tiles
#pragma unroll
    for (int k = 0; k < 4; ++k) stage[k] = flat[(uint64_t(t) * kHTile + threadIdx.x) * 4 + k];
  };
  stage_load(t0);
  for (uint32_t t = t0; t < t1; ++t) {
    __syncthreads();  // every wave is done reading the previous tile
#pragma unroll
    for (int k = 0; k < 4; ++k) tflat[threadIdx.x * 4 + k] = stage[k];
    __syncthreads();
    if (t + 1 < t1) stage_load(t + 1);  // in flight while this tile is consumed

    const pair_rec<T>* src = &tile[wave * SUB];
    const uint32_t j0      = t * kHTile + wave * SUB;
    // wave-uniform: does the slice hold a target of this block (the self pair) or a record past n (padding)?
    const bool checked = (j0 + SUB > n) | ((j0 < own1) & (j0 + SUB > own0));
    if (checked) slice(src, j0, std::true_type{});
    else slice(src, j0, std::false_type{});
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// Both handles begin with hermite_handle: recs is pair_rec<T>[padded], part the first of the chunks' partial arrays.

// Fills the shared fields of a new handle and allocates its records (the caller has made `device` current).  Nothing is cleared:
// every compute writes all of them before it reads them.
inline void pair_handle_alloc(hermite_handle* h, int dtype, int dim, uint32_t n, int device, const hermite_plan& plan) {
  hermite_handle_fill(h, dtype, dim, n, device, plan);
  h->mem.alloc(&h->recs, h->tsz * 4 * size_t(h->padded));
}

// The head of a compute call: check_state without the arrays it never reads (v, a and ao may be NULL), then the whole system.
inline int pair_check_state(const nbody_state* s, const char* who) { return hermite_check_state(s, who, false); }

// The tail of a blocking read, after its argument checks: the device, then the state rules.  type: "nbody_neighbours" or "nbody_knn".
inline int pair_read_ready(const hermite_handle* h, const char* type, const char* who, const char* compute_api, hipStream_t st) {
  if (int r = check_same_device(h->device, st, type)) return r;
  if (capture_id(st) != 0) {
    set_error("%s is blocking: it cannot be recorded (call it outside nbody_graph_begin/end)", who);
    return NBODY_ERR_STATE;
  }
  if (!h->started) {
    set_error("%s before %s on this handle", who, compute_api);
    return NBODY_ERR_STATE;
  }
  return NBODY_OK;
}

}  // namespace nbody
