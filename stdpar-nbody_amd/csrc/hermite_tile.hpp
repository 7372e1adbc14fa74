// What the direct-sum Hermite integrators of hermite.hip (order 4: force, jerk) and hermite6.hip (order 6: force, jerk, snap) share:
// the launch plan, the packed source record, the tiled pair sum with its pair arithmetic, the chunk sums of the correctors and the
// host-side checks of the two handles.  G is the number of summed quantities, which is also the number of 4-value groups of a record:
// 2 for order 4, 3 for order 6.
//
// The pair sum: R targets per lane in registers, records staged through LDS tiles of kHTile and read as wave-uniform broadcasts, every
// tile split over the four waves of the block, the tiles split over grid.y chunks; the block's four slices are added in wave order and
// the raw sums of the chunk go to the partial array, which the correctors add IN CHUNK ORDER.  The rounding order of a body's sums
// (slices of a tile by wave, tiles in order, waves in order, chunks in order) follows from sz alone: hermite_plan_for reads nothing
// else — not the device, not the CU count — so two runs, an eager step and a replayed one, and a handle destroyed and made again give
// the same bits (tests/test_gpu_hermite_bits.py holds every change of this file to the bits recorded before it).
#pragma once
#include "common.hpp"

namespace nbody {

constexpr int kHBlock = 256;  // 4 waves: one group of 64 R targets, the tile cut in four
constexpr int kHWaves = kHBlock / 64;
constexpr int kHTile  = 256;  // source records per LDS tile (fixed: the rounding order depends on it); one record per lane to stage

// Source record of the pair kernels, G groups of four values: {p[3], m}, {v[3], 0} and for G = 3 {a[3], 0} (predicted position,
// velocity, acceleration; D components used, 2D zero-fills component 2).  64 B in double (four ds_read_b128), 32 B in float for
// G = 2; 96 B (six) and 48 B for G = 3.
template <typename T, int G>
struct alignas(sizeof(T) * (G == 2 ? 8 : 4)) hermite_rec {
  T g[G][4];
};
constexpr int kRecP = 0, kRecV = 1, kRecA = 2, kRecM = 3;  // groups; the mass is g[kRecP][kRecM]

// Launch shape, from sz alone.  R: targets per lane; chunks x tiles_per_chunk >= ntiles: the cut of the source range over grid.y.
// From 65536 bodies on two targets per lane (every record read from LDS serves two pairs, half as many blocks stage the source range,
// and every SIMD still has two waves); below, one target per lane and as many chunks as bring the grid to about 2048 blocks (8 per
// CU of the largest part): at most 64, at least min_chunks, at most one per tile.  Order 4 passes 1.  Order 6 passes 2: never fewer
// than two chunks once there are two tiles, so that its plan has three boundaries (one tile | one tile per chunk | several tiles per
// chunk, and R), all below 65537 bodies, where a test can afford to stand on both sides of each; the second chunk costs 3 D partial
// sums per body beside O(N) pairs.
struct hermite_plan {
  uint32_t R, blocks, ntiles, chunks, tiles_per_chunk;
};
inline hermite_plan hermite_plan_for(uint32_t sz, uint32_t min_chunks) {
  hermite_plan p;
  p.R      = sz >= 65536u ? 2u : 1u;
  p.blocks = (sz + 64u * p.R - 1u) / (64u * p.R);
  p.ntiles = (sz + kHTile - 1u) / kHTile;
  uint32_t want = (2048u + p.blocks - 1u) / p.blocks;
  if (want > 64u) want = 64u;
  if (want < min_chunks) want = min_chunks;
  if (want > p.ntiles) want = p.ntiles;
  p.tiles_per_chunk = (p.ntiles + want - 1u) / want;
  p.chunks          = (p.ntiles + p.tiles_per_chunk - 1u) / p.tiles_per_chunk;
  return p;
}

// ---- the pair ------------------------------------------------------------------------------------------------------------------
// First stage of a pair, both orders: d = x_j - x_i, u = v_j - v_i, q = |d|^2 + e2 (the softened K1's FMA chain seeded with e2),
// du = d.u (FMA chain).
template <typename T, int D, int G>
__device__ __forceinline__ void hermite_pair_head(T (&d)[D], T (&u)[D], T& q, T& du, const hermite_rec<T, G>& s, const T (&xi)[D],
                                                  const T (&vi)[D], T e2) {
#pragma unroll
  for (int k = 0; k < D; ++k) {
    d[k] = s.g[kRecP][k] - xi[k];
    u[k] = s.g[kRecV][k] - vi[k];
  }
  T t = e2;
#pragma unroll
  for (int k = 0; k < D; ++k) t = __builtin_elementwise_fma(d[k], d[k], t);
  q   = t;
  T g = d[0] * u[0];
#pragma unroll
  for (int k = 1; k < D; ++k) g = __builtin_elementwise_fma(d[k], u[k], g);
  du = g;
}

// w = m q^(-3/2) — soft_weight's arithmetic, operation for operation — from the ONE reciprocal square root y = rsq(q) a pair takes,
// and what each order builds its 1 / q from.  Double: A = fl(y y), e = fl(1 - q A) (one FMA: the exact residual of the ROUNDED A up to
// 2^-76), so 1 / q = A / (1 - e) = A (1 + e + e^2 + O(e^3)), e <= 2^-23.  Float: A = y y from the 1-ulp v_rsq_f32 is 1 / q within
// 2.5 ulp — the size of m y^3's own ~3 ulp — and takes no correction (e is not set).
//
// Rounding error of one pair term, P_g, in units of eps_T (2^-52, 2^-23; one rounding = 0.5) times the term's magnitude scale (every
// product taken as the product of norms, every sum as the sum of absolute values), counted from d, u, b, q, d.u and |u|^2 + d.b as the
// pair's head made them.  tests/hermite_wide_model.py carries the table, tests/test_gpu_hermite_wide.py holds the kernels to it:
//                         a       jerk    snap
//   double                2.5     5       7
//   float                 4.5     8.5     12
// a is w's figure.  Double: 2.5, the series above.  Float: y within 1 ulp makes y^3 within 3, and A = y y, A y and m (A y) round once
// each: 4.5.  The jerk's and the snap's figures are derived beside hermite_pair_batch of each order; the jerk's is the same in both.
template <typename T>
__device__ __forceinline__ T hermite_pair_weight(T q, T m, const pair_consts<T>& pc, T& A, T& e) {
  if constexpr (sizeof(T) == 8) {
    const double y  = __builtin_amdgcn_rsq(q);
    A               = y * y;
    e               = __builtin_fma(-q, A, 1.0);
    const double y3 = A * y;
    const double p  = __builtin_fma(e, pc.k1875, pc.k15);
    const double g  = p * e;
    const double my = m * y3;
    return __builtin_fma(my, g, my);  // == pair_math<double>::weight_far<false>
  } else {
    const float y = __builtin_amdgcn_rsqf(q);
    A             = y * y;
    return m * (A * y);  // == soft_weight<float>
  }
}

// Order 4.  U records against the R targets of a lane, stage by stage like pair_batch_soft (independent chains in flight):
//   acc[0] += w d,                w = m q^(-3/2)
//   acc[1] += w (u + alpha d),    alpha = -3 du / q
// Double: B = -3 A (<= 1/2 ulp beyond A's), alpha' = fma(B, fma(e, e, e), B) (truncation 2^-69, one rounding), alpha = du alpha' (one
// rounding): alpha is within 2 ulp of -3 fl(d.u) / q, against w's <= 2.5 ulp of m q^(-3/2); t = fma(alpha, d, u) rounds once.  The
// jerk's pair term fl-error is therefore <= 2.5 ulp on its w u part and <= 5 ulp on its w alpha d part.
// Float: A within 2.5 ulp of 1 / q, -3 A and du (-3 A) round once each: alpha within 3.5 ulp; t rounds once (0.5, on |u| + |alpha d|);
// with w's 4.5 the term is within 5 ulp on its w u part and 4.5 + 3.5 + 0.5 = 8.5 ulp on its w alpha d part.
// Self pair, coincident bodies at equal velocity, zero-mass padding: d = 0 (and u = 0) or w = 0 add exactly 0; q >= e2 keeps all finite.
template <typename T, int D, int R, int U>
__device__ __forceinline__ void hermite_pair_batch(T (&acc)[2][R][D], const T (&tg)[2][R][D], const hermite_rec<T, 2> (&s)[U],
                                                   const pair_consts<T>& pc, T e2) {
  T d[U][R][D], u[U][R][D], q[U][R], du[U][R], w[U][R], al[U][R];
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r) hermite_pair_head<T, D, 2>(d[b][r], u[b][r], q[b][r], du[b][r], s[b], tg[kRecP][r], tg[kRecV][r], e2);
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      T A, e;
      w[b][r] = hermite_pair_weight<T>(q[b][r], s[b].g[kRecP][kRecM], pc, A, e);
      if constexpr (sizeof(T) == 8) {
        const double B  = -3.0 * A;
        const double ap = __builtin_fma(B, __builtin_fma(e, e, e), B);
        al[b][r]        = du[b][r] * ap;
      } else {
        al[b][r] = du[b][r] * (-3.0f * A);
      }
    }
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const T t    = __builtin_elementwise_fma(al[b][r], d[b][r][k], u[b][r][k]);
        acc[0][r][k] = __builtin_elementwise_fma(w[b][r], d[b][r][k], acc[0][r][k]);
        acc[1][r][k] = __builtin_elementwise_fma(w[b][r], t, acc[1][r][k]);
      }
}

// Order 6.  With b = a_j - a_i and g2 = |u|^2 + d.b (FMA chains) besides:
//   acc[0] += w d,
//   acc[1] += w (u + c1 d),                           c1 = -3 alpha,             alpha = du / q
//   acc[2] += w (b + c2 u + c3 d),                    c2 = -6 alpha = 2 c1,      c3 = 15 alpha^2 - 3 gamma,  gamma = g2 / q
// Double: 1 / q as fma(A, fma(e, e, e), A): truncation 2^-69, two roundings.  alpha, gamma: one more rounding each on top of their dot
// products'; c3 = fma(15 alpha, alpha, -3 gamma).  (Order 4's alpha folds the -3 into B first and differs from c1 in the last bit:
// each order keeps its own.)
// The pair term's fl-error, I the error of iq = 1 / q (double 1 ulp: two roundings; float 2.5 ulp: A) and W that of w (2.5, 4.5):
//   alpha, gamma   I + 0.5 (the product with du, with g2)                                           1.5 ulp    float 3
//   c1 = c2 / 2    + 0.5 (the product with -3; c2 = c1 + c1 is exact)                               2          3.5
//   c3             15 alpha: I + 1, times alpha: 2 I + 1.5, the FMA's rounding 0.5 (the -3 gamma
//                  part, I + 1.5, is smaller)                                                       4          7
//   jerk  w tj     tj = fma(c1, d, u) rounds once: W + 0.5 on w u, W + c1's + 0.5 on w c1 d         5          8.5
//   snap  w ts     ts = fma(c3, d, fma(c2, u, b)), two roundings: W + 1 on w b, W + c2's + 1 on
//                  w c2 u, W + c3's + 0.5 on w c3 d                                                 7          12
// Self pair, coincident bodies at equal velocity and acceleration, zero-mass padding: d = u = b = 0 or w = 0 add exactly 0 (alpha =
// gamma = 0 there, no 0 x inf: q >= e2 keeps everything finite).  All velocities zero: du = 0, c1 = c2 = -0, the jerk's term is 0.
template <typename T, int D, int R, int U>
__device__ __forceinline__ void hermite_pair_batch(T (&acc)[3][R][D], const T (&tg)[3][R][D], const hermite_rec<T, 3> (&s)[U],
                                                   const pair_consts<T>& pc, T e2) {
  T d[U][R][D], u[U][R][D], b[U][R][D], q[U][R], du[U][R], g2[U][R], w[U][R], c1[U][R], c3[U][R];
#pragma unroll
  for (int n = 0; n < U; ++n)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      hermite_pair_head<T, D, 3>(d[n][r], u[n][r], q[n][r], du[n][r], s[n], tg[kRecP][r], tg[kRecV][r], e2);
#pragma unroll
      for (int k = 0; k < D; ++k) b[n][r][k] = s[n].g[kRecA][k] - tg[kRecA][r][k];
      T f = u[n][r][0] * u[n][r][0];
#pragma unroll
      for (int k = 1; k < D; ++k) f = __builtin_elementwise_fma(u[n][r][k], u[n][r][k], f);
#pragma unroll
      for (int k = 0; k < D; ++k) f = __builtin_elementwise_fma(d[n][r][k], b[n][r][k], f);
      g2[n][r] = f;
    }
#pragma unroll
  for (int n = 0; n < U; ++n)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      T A, e, iq;
      w[n][r] = hermite_pair_weight<T>(q[n][r], s[n].g[kRecP][kRecM], pc, A, e);
      if constexpr (sizeof(T) == 8)
        iq = __builtin_fma(A, __builtin_fma(e, e, e), A);
      else
        iq = A;
      const T al = du[n][r] * iq, ga = g2[n][r] * iq;
      c1[n][r]   = T(-3) * al;
      c3[n][r]   = __builtin_elementwise_fma(T(15) * al, al, T(-3) * ga);
    }
#pragma unroll
  for (int n = 0; n < U; ++n)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const T c2 = c1[n][r] + c1[n][r];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const T tj   = __builtin_elementwise_fma(c1[n][r], d[n][r][k], u[n][r][k]);
        const T ts   = __builtin_elementwise_fma(c3[n][r], d[n][r][k], __builtin_elementwise_fma(c2, u[n][r][k], b[n][r][k]));
        acc[0][r][k] = __builtin_elementwise_fma(w[n][r], d[n][r][k], acc[0][r][k]);
        acc[1][r][k] = __builtin_elementwise_fma(w[n][r], tj, acc[1][r][k]);
        acc[2][r][k] = __builtin_elementwise_fma(w[n][r], ts, acc[2][r][k]);
      }
    }
}

// ---- the tiled pair sum ----------------------------------------------------------------------------------------------------------
// The whole body of a pair kernel: grid (blocks of 64 R targets, chunks).  flat: the records as 4 G values each, padded to whole
// tiles with zero-mass records.  part: [chunk][G D][n] raw sums, unscaled (the D components of quantity 0, then of quantity 1, ...).
// GATHER (block time steps): the n targets are the bodies act[0 .. n), slot by slot, and part is over the slots; otherwise they are
// the bodies 0 .. n.
template <typename T, int D, int R, int G, bool GATHER>
__device__ __forceinline__ void hermite_tile_sum(const T* __restrict__ flat, T* __restrict__ part, T e2, uint32_t n, uint32_t ntiles,
                                                 uint32_t tiles_per_chunk, const uint32_t* __restrict__ act) {
  using rec_t       = hermite_rec<T, G>;
  constexpr int V   = 4 * G;                           // values per record
  constexpr int SUB = kHTile / kHWaves;                // records of a tile one wave takes
  constexpr int U   = (sizeof(T) == 8 ? 2 : 4) / R;    // records a batch: 2 pairs in flight per lane in double, 4 in float
  constexpr int NP  = (kHWaves - 1) * R * G * D * 64;  // the other waves' sums, handed over through LDS
  constexpr size_t kTileBytes = sizeof(rec_t) * kHTile, kPartBytes = sizeof(T) * NP;
  __shared__ __attribute__((aligned(64))) unsigned char smem[kTileBytes > kPartBytes ? kTileBytes : kPartBytes];
  const rec_t* tile = reinterpret_cast<const rec_t*>(smem);
  T* tflat          = reinterpret_cast<T*>(smem);
  T* hand           = reinterpret_cast<T*>(smem);  // after the last tile has been consumed

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  T tg[G][R][D], acc[G][R][D];
  uint32_t ti[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ti[r]      = blockIdx.x * (64 * R) + r * 64 + lane;
    uint32_t i = ti[r] < n ? ti[r] : 0u;  // clamp: out-of-range lanes compute, never store
    if constexpr (GATHER) i = act[i];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int k = 0; k < D; ++k) {
        tg[g][r][k]  = reinterpret_cast<const rec_t*>(flat)[i].g[g][k];
        acc[g][r][k] = T(0);
      }
  }

  const uint32_t t0 = blockIdx.y * tiles_per_chunk;
  const uint32_t t1 = t0 + tiles_per_chunk < ntiles ? t0 + tiles_per_chunk : ntiles;
  const pair_consts<T> pc;

  // one record per lane, value by value: a struct copy of this size is left in private memory (scratch) by the compiler
  T stage[V];
  auto stage_load = [&](uint32_t t) {  // the record array is padded to whole tiles
#pragma unroll
    for (int k = 0; k < V; ++k) stage[k] = flat[(uint64_t(t) * kHTile + threadIdx.x) * V + k];
  };
  stage_load(t0);
  for (uint32_t t = t0; t < t1; ++t) {
    __syncthreads();  // every wave is done reading the previous tile
#pragma unroll
    for (int k = 0; k < V; ++k) tflat[threadIdx.x * V + k] = stage[k];
    __syncthreads();
    if (t + 1 < t1) stage_load(t + 1);  // in flight while this tile is consumed

    const rec_t* src = &tile[wave * SUB];
#pragma unroll 1
    for (int jj = 0; jj < SUB; jj += U) {
      rec_t s[U];  // field by field, for the same reason
#pragma unroll
      for (int b = 0; b < U; ++b) {  // wave-uniform address: LDS broadcast
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int k = 0; k < D; ++k) s[b].g[g][k] = src[jj + b].g[g][k];
        s[b].g[kRecP][kRecM] = src[jj + b].g[kRecP][kRecM];
      }
      hermite_pair_batch<T, D, R, U>(acc, tg, s, pc, e2);
    }
  }

  // the four slices in wave order
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int k = 0; k < D; ++k) hand[((((wave - 1) * R + r) * G + g) * D + k) * 64 + lane] = acc[g][r][k];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int p = 1; p < kHWaves; ++p)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int k = 0; k < D; ++k) acc[g][r][k] += hand[((((p - 1) * R + r) * G + g) * D + k) * 64 + lane];
    T* out = part + uint64_t(blockIdx.y) * (G * D) * n;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (ti[r] < n) {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int k = 0; k < D; ++k) out[uint64_t(g * D + k) * n + ti[r]] = acc[g][r][k];
      }
    }
  }
}

// ---- chunk sums ------------------------------------------------------------------------------------------------------------------
// Component k of body i: s[g] = c * (the chunks' raw sums of quantity g, added in chunk order), part as hermite_tile_sum wrote it.
template <typename T, int D, int G>
__device__ __forceinline__ void hermite_chunk_sums(T (&s)[G], const T* __restrict__ part, T c, uint32_t n, uint32_t i, uint32_t chunks,
                                                   int k) {
#pragma unroll
  for (int g = 0; g < G; ++g) s[g] = part[uint64_t(g * D + k) * n + i];
  for (uint32_t ch = 1; ch < chunks; ++ch)
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] += part[(uint64_t(ch) * (G * D) + g * D + k) * n + i];
#pragma unroll
  for (int g = 0; g < G; ++g) s[g] = c * s[g];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// What struct nbody_hermite and struct nbody_hermite6 both begin with.
struct hermite_handle {
  int dtype = 0, dim = 0, device = 0;  // device: nbody_*_create_on's; every call runs there
  uint32_t n = 0, padded = 0;
  size_t tsz = 0;
  hermite_plan plan{};
  void* recs   = nullptr;  // hermite_rec<T, G>[padded]
  void* part   = nullptr;  // T[chunks][G D][n]
  bool started = false;    // the start call has run (host call order, which a recorded step replays)
  device_buffers mem;      // owns recs, part and what the handle's own struct adds
};

// The shared fields of a new handle.
inline void hermite_handle_fill(hermite_handle* h, int dtype, int dim, uint32_t n, int device, const hermite_plan& plan) {
  h->device = device;
  h->dtype  = dtype;
  h->dim    = dim;
  h->n      = n;
  h->tsz    = dtype == NBODY_F32 ? 4 : 8;
  h->plan   = plan;
  h->padded = plan.ntiles * uint32_t(kHTile);
}

// Fills the shared fields of a new handle and allocates its records and partial sums (the caller has made `device` current).
// Nothing is cleared: every launch sequence writes all of recs and part before it reads them.  (A memset here would be ordered
// against the NULL stream only, not against the non-blocking stream of a context, and could land after the first predict.)
inline void hermite_handle_alloc(hermite_handle* h, int dtype, int dim, uint32_t n, int device, int G, uint32_t min_chunks) {
  hermite_handle_fill(h, dtype, dim, n, device, hermite_plan_for(n, min_chunks));
  h->mem.alloc(&h->recs, h->tsz * 4 * G * size_t(h->padded));
  h->mem.alloc(&h->part, h->tsz * size_t(h->plan.chunks) * G * size_t(dim) * size_t(n));
}

// The common head of a start or step call, before the dispatch on (dtype, dim): the state (all_arrays: check_state's), then the whole
// system.
inline int hermite_check_state(const nbody_state* s, const char* who, bool all_arrays = true) {
  if (int r = check_state(s, all_arrays)) return r;
  NB_ARG(s->first == 0 && s->count == s->sz, "%s needs the whole system (first = 0, count = sz), got [%u, %u+%u) of %u", who, s->first,
         s->first, s->count, s->sz);
  return NBODY_OK;
}

// ... and inside it: eps, the handle, the device, and for a step (start_api != nullptr) that the start call has run.  Every
// argument error before the device is touched, in the header's order.  type: "nbody_hermite" or "nbody_hermite6".
template <typename T>
inline int hermite_check_call(const hermite_handle* h, const nbody_state* s, double eps, hipStream_t st, const char* type, const char* who,
                              const char* start_api, T* e2) {
  if (int r = check_softening<T>(eps, e2)) return r;
  NB_ARG(h != nullptr, "%s is NULL", type);
  NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
         "%s was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", type, h->dtype, h->dim, h->n, s->dtype,
         s->dim, s->sz);
  if (int r = check_same_device(h->device, st, type)) return r;
  if (start_api && !h->started) {
    set_error("%s before %s on this handle", who, start_api);
    return NBODY_ERR_STATE;
  }
  return NBODY_OK;
}

// The tail of a read call, after its argument checks (`bytes` is n rows of D values): refused while recording and before the start
// call; then either `plain`, an [n][D] array of the handle, or D values of group `group` out of the records of G groups.
inline int hermite_read_rows(const hermite_handle* h, const char* type, const char* who, const char* start_api, const void* plain,
                             int group, int G, void* host_out, size_t bytes, hipStream_t st) {
  if (int r = check_same_device(h->device, st, type)) return r;
  device_guard guard(h->device);
  if (capture_id(st) != 0) {
    set_error("%s is blocking: it cannot be recorded (call it outside nbody_graph_begin/end)", who);
    return NBODY_ERR_STATE;
  }
  if (!h->started) {
    set_error("%s before %s on this handle", who, start_api);
    return NBODY_ERR_STATE;
  }
  if (plain) {
    NB_HIP(hipMemcpyAsync(host_out, plain, bytes, hipMemcpyDeviceToHost, st));
  } else {
    const size_t row = h->tsz * size_t(h->dim);
    const char* src  = static_cast<const char*>(h->recs) + size_t(group) * 4 * h->tsz;
    NB_HIP(hipMemcpy2DAsync(host_out, row, src, size_t(4 * G) * h->tsz, row, h->n, hipMemcpyDeviceToHost, st));
  }
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}

}  // namespace nbody
