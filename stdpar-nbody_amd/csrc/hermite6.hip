// Sixth-order Hermite predictor-corrector (Nitadori & Makino 2008) for the direct sum: nbody_hermite6_* of include/nbody_hip.h.
// No reference counterpart.  Fixed dt, Plummer softening required (eps = 0 is refused, as in the fourth-order integrator of hermite.hip).
//
// Three launches per step (six for the start, which evaluates twice), all on the caller's stream, nothing allocated after
// nbody_hermite6_create:
//   predict          one lane per body: the packed source record {xp[3], m, vp[3], 0, ap[3], 0} (12 T; 2D zero-fills component 2) into the
//                    handle's record array, padded with zero-mass records to a whole number of tiles so that the pair kernel never tests a
//                    bound;
//   force+jerk+snap  the hot path: R targets per lane in registers, records staged through LDS tiles of kH6Tile and read as wave-uniform
//                    broadcasts, every tile split over the four waves of the block, the tiles split over grid.y chunks where the targets
//                    alone would not fill the chip; the block's four slices are added in wave order and the raw sums of the chunk go to
//                    the handle's partial array (always, also with one chunk: 3 D values per body beside O(N) pairs);
//   correct          one lane per body: adds the chunks' sums IN CHUNK ORDER, scales by c, applies the corrector and the crackle formula.
// The rounding order of a body's sums (slices of a tile by wave, tiles in order, waves in order, chunks in order) follows from sz
// alone: hermite6_plan_for reads nothing else — not the device, not the CU count — so two runs, an eager step and a replayed one, and
// a handle destroyed and made again give the same bits.  No atomics on a, the jerk or the snap, no waiting between blocks.
#include "common.hpp"

namespace nbody {

constexpr int kH6Block = 256;  // 4 waves: one group of 64 R targets, the tile cut in four
constexpr int kH6Waves = kH6Block / 64;
constexpr int kH6Tile  = 256;  // source records per LDS tile (fixed: the rounding order depends on it); one record per lane to stage
constexpr int kH6Rec   = 12;   // values per record

// source record of the pair kernel: 96 B in double (six ds_read_b128), 48 B in float (three)
template <typename T>
struct alignas(sizeof(T) * 4) h6src_rec {
  T p[3];  // predicted position, D used
  T m;
  T v[3];  // predicted velocity, D used
  T pad0;
  T a[3];  // predicted acceleration, D used
  T pad1;
};

// Launch shape, from sz alone.  R: targets per lane; chunks x tiles_per_chunk >= ntiles: the cut of the source range over grid.y.
// From 65536 bodies on two targets per lane (every record read from LDS serves two pairs and half as many blocks stage the source
// range); below, one.  As many chunks as bring the grid to about 2048 blocks (8 per CU of the largest part), at most 64, at most one
// per tile and — unlike the fourth-order plan — never fewer than two once there are two tiles: the plan then has three boundaries
// (one tile | one tile per chunk | several tiles per chunk, and R), all below 65537 bodies, where a test can afford to stand on both
// sides of each; the second chunk costs 3 D partial sums per body beside O(N) pairs.
struct hermite6_plan {
  uint32_t R, blocks, ntiles, chunks, tiles_per_chunk;
};
inline hermite6_plan hermite6_plan_for(uint32_t sz) {
  hermite6_plan p;
  p.R      = sz >= 65536u ? 2u : 1u;
  p.blocks = (sz + 64u * p.R - 1u) / (64u * p.R);
  p.ntiles = (sz + kH6Tile - 1u) / kH6Tile;
  uint32_t want = (2048u + p.blocks - 1u) / p.blocks;
  if (want > 64u) want = 64u;
  if (want < 2u) want = 2u;
  if (want > p.ntiles) want = p.ntiles;
  p.tiles_per_chunk = (p.ntiles + want - 1u) / want;
  p.chunks          = (p.ntiles + p.tiles_per_chunk - 1u) / p.tiles_per_chunk;
  return p;
}

// what a launch sequence is for: the two passes of the start, and the step
constexpr int kH6StartA = 0;  // records (x, v, 0); keeps a alone
constexpr int kH6Start  = 1;  // records (x, v, a); a, jerk, snap, crackle = 0
constexpr int kH6Step   = 2;  // the predictor; the corrector and the crackle

// ---- predict -------------------------------------------------------------------------------------------------------------------
// The two start passes: the records of the state as it is (ap = 0 in the first: snap needs the accelerations of ALL bodies, which the
// first pass makes).  Otherwise the predictor, with h = dt and k0 the crackle kept from the previous step (Horner in h):
//   xp = x + h v + h^2/2 a0 + h^3/6 j0 + h^4/24 s0 + h^5/120 k0
//   vp = v + h a0 + h^2/2 j0 + h^3/6 s0 + h^4/24 k0
//   ap = a0 + h j0 + h^2/2 s0 + h^3/6 k0
template <typename T, int D, int MODE>
__global__ __launch_bounds__(kH6Block) void hermite6_predict_kernel(const T* __restrict__ m, const T* __restrict__ x, const T* __restrict__ v,
                                                                    const T* __restrict__ a, const T* __restrict__ jerk,
                                                                    const T* __restrict__ snap, const T* __restrict__ crackle,
                                                                    T* __restrict__ recs, T h, uint32_t n, uint32_t padded) {
  const uint32_t i = blockIdx.x * kH6Block + threadIdx.x;
  if (i >= padded) return;
  T r[kH6Rec];
#pragma unroll
  for (int k = 0; k < kH6Rec; ++k) r[k] = T(0);
  if (i < n) {
    r[3] = m[i];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const uint64_t e = uint64_t(i) * D + k;
      if constexpr (MODE != kH6Step) {
        r[k]     = x[e];
        r[4 + k] = v[e];
        if constexpr (MODE == kH6Start) r[8 + k] = a[e];
      } else {
        const T x0 = x[e], v0 = v[e], a0 = a[e], j0 = jerk[e], s0 = snap[e], k0 = crackle[e];
        auto fma = [](T p, T q, T s) { return __builtin_elementwise_fma(p, q, s); };
        r[k]     = fma(h, fma(h * T(0.5), fma(h * T(1.0 / 3.0), fma(h * T(0.25), fma(h * T(0.2), k0, s0), j0), a0), v0), x0);
        r[4 + k] = fma(h, fma(h * T(0.5), fma(h * T(1.0 / 3.0), fma(h * T(0.25), k0, s0), j0), a0), v0);
        r[8 + k] = fma(h, fma(h * T(0.5), fma(h * T(1.0 / 3.0), k0, s0), j0), a0);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kH6Rec; ++k) recs[uint64_t(i) * kH6Rec + k] = r[k];
}

// ---- the pair ------------------------------------------------------------------------------------------------------------------
// U records against the R targets of a lane, stage by stage like pair_batch_hermite (independent chains in flight).  With d = x_j - x_i,
// u = v_j - v_i, b = a_j - a_i, q = |d|^2 + e2 (the softened K1's FMA chain seeded with e2), du = d.u, g2 = |u|^2 + d.b (FMA chains):
//   acc  += w d,                                    w = m q^(-3/2)        — soft_weight's arithmetic, operation for operation
//   jacc += w (u + c1 d),                           c1 = -3 alpha,             alpha = du / q
//   sacc += w (b + c2 u + c3 d),                    c2 = -6 alpha = 2 c1,      c3 = 15 alpha^2 - 3 gamma,  gamma = g2 / q
// from the ONE reciprocal square root y = rsq(q) the force takes.  Double: A = fl(y y), e = fl(1 - q A) (one FMA), so
// 1 / q = A (1 + e + e^2 + O(e^3)), e <= 2^-23, as fma(A, fma(e, e, e), A): truncation 2^-69, two roundings.  alpha, gamma: one more
// rounding each on top of their dot products'; c3 = fma(15 alpha, alpha, -3 gamma).  Float: A = y y from the 1-ulp v_rsq_f32 is 1 / q
// within 2.5 ulp — the size of m y^3's own ~3 ulp — and takes no correction.
// Self pair, coincident bodies at equal velocity and acceleration, zero-mass padding: d = u = b = 0 or w = 0 add exactly 0 (alpha =
// gamma = 0 there, no 0 x inf: q >= e2 keeps everything finite).  All velocities zero: du = 0, c1 = c2 = -0, the jerk's term is 0.
template <typename T, int D, int R, int U>
__device__ __forceinline__ void pair_batch_hermite6(T (&acc)[R][D], T (&jacc)[R][D], T (&sacc)[R][D], const T (&xi)[R][D],
                                                    const T (&vi)[R][D], const T (&ai)[R][D], const h6src_rec<T> (&s)[U],
                                                    const pair_consts<T>& pc, T e2) {
  T d[U][R][D], u[U][R][D], b[U][R][D], q[U][R], du[U][R], g2[U][R], w[U][R], c1[U][R], c3[U][R];
#pragma unroll
  for (int n = 0; n < U; ++n)
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int k = 0; k < D; ++k) {
        d[n][r][k] = s[n].p[k] - xi[r][k];
        u[n][r][k] = s[n].v[k] - vi[r][k];
        b[n][r][k] = s[n].a[k] - ai[r][k];
      }
      T t = e2;
#pragma unroll
      for (int k = 0; k < D; ++k) t = __builtin_elementwise_fma(d[n][r][k], d[n][r][k], t);
      q[n][r] = t;
      T g = d[n][r][0] * u[n][r][0];
#pragma unroll
      for (int k = 1; k < D; ++k) g = __builtin_elementwise_fma(d[n][r][k], u[n][r][k], g);
      du[n][r] = g;
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
      T iq;
      if constexpr (sizeof(T) == 8) {
        const double y  = __builtin_amdgcn_rsq(q[n][r]);
        const double A  = y * y;
        const double e  = __builtin_fma(-q[n][r], A, 1.0);
        const double y3 = A * y;
        const double p  = __builtin_fma(e, pc.k1875, pc.k15);
        const double g  = p * e;
        const double my = s[n].m * y3;
        w[n][r]         = __builtin_fma(my, g, my);  // == pair_math<double>::weight_far<false>
        iq              = __builtin_fma(A, __builtin_fma(e, e, e), A);
      } else {
        const float y = __builtin_amdgcn_rsqf(q[n][r]);
        const float A = y * y;
        w[n][r]       = s[n].m * (A * y);  // == soft_weight<float>
        iq            = A;
      }
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
        const T tj = __builtin_elementwise_fma(c1[n][r], d[n][r][k], u[n][r][k]);
        const T ts = __builtin_elementwise_fma(c3[n][r], d[n][r][k], __builtin_elementwise_fma(c2, u[n][r][k], b[n][r][k]));
        acc[r][k]  = __builtin_elementwise_fma(w[n][r], d[n][r][k], acc[r][k]);
        jacc[r][k] = __builtin_elementwise_fma(w[n][r], tj, jacc[r][k]);
        sacc[r][k] = __builtin_elementwise_fma(w[n][r], ts, sacc[r][k]);
      }
    }
}

// ---- force + jerk + snap -------------------------------------------------------------------------------------------------------
// grid (blocks of 64 R targets, chunks).  part: [chunk][3 D][n] raw sums (a's D components, then the jerk's, then the snap's), unscaled.
template <typename T, int D, int R>
__global__ __launch_bounds__(kH6Block) void hermite6_pair_kernel(const T* __restrict__ flat, T* __restrict__ part, T e2, uint32_t n,
                                                                 uint32_t ntiles, uint32_t tiles_per_chunk) {
  using rec_t       = h6src_rec<T>;
  constexpr int SUB = kH6Tile / kH6Waves;               // records of a tile one wave takes
  constexpr int U   = (sizeof(T) == 8 ? 2 : 4) / R;     // records a batch: 2 pairs in flight per lane in double, 4 in float
  constexpr int NP  = (kH6Waves - 1) * R * 3 * D * 64;  // the other waves' sums, handed over through LDS
  constexpr size_t kTileBytes = sizeof(rec_t) * kH6Tile, kPartBytes = sizeof(T) * NP;
  __shared__ __attribute__((aligned(64))) unsigned char smem[kTileBytes > kPartBytes ? kTileBytes : kPartBytes];
  const rec_t* tile = reinterpret_cast<const rec_t*>(smem);
  T* tflat          = reinterpret_cast<T*>(smem);
  T* hand           = reinterpret_cast<T*>(smem);  // after the last tile has been consumed

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  T xi[R][D], vi[R][D], ai[R][D], acc[R][D], jacc[R][D], sacc[R][D];
  uint32_t ti[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ti[r]            = blockIdx.x * (64 * R) + r * 64 + lane;
    const uint64_t i = ti[r] < n ? ti[r] : 0u;  // clamp: out-of-range lanes compute, never store
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xi[r][k]   = flat[i * kH6Rec + k];
      vi[r][k]   = flat[i * kH6Rec + 4 + k];
      ai[r][k]   = flat[i * kH6Rec + 8 + k];
      acc[r][k]  = T(0);
      jacc[r][k] = T(0);
      sacc[r][k] = T(0);
    }
  }

  const uint32_t t0 = blockIdx.y * tiles_per_chunk;
  const uint32_t t1 = t0 + tiles_per_chunk < ntiles ? t0 + tiles_per_chunk : ntiles;
  const pair_consts<T> pc;

  // one record per lane, value by value: a struct copy of this size is left in private memory (scratch) by the compiler
  T stage[kH6Rec];
  auto stage_load = [&](uint32_t t) {  // the record array is padded to whole tiles
#pragma unroll
    for (int k = 0; k < kH6Rec; ++k) stage[k] = flat[(uint64_t(t) * kH6Tile + threadIdx.x) * kH6Rec + k];
  };
  stage_load(t0);
  for (uint32_t t = t0; t < t1; ++t) {
    __syncthreads();  // every wave is done reading the previous tile
#pragma unroll
    for (int k = 0; k < kH6Rec; ++k) tflat[threadIdx.x * kH6Rec + k] = stage[k];
    __syncthreads();
    if (t + 1 < t1) stage_load(t + 1);  // in flight while this tile is consumed

    const rec_t* src = &tile[wave * SUB];
#pragma unroll 1
    for (int jj = 0; jj < SUB; jj += U) {
      rec_t s[U];  // field by field, for the same reason
#pragma unroll
      for (int n2 = 0; n2 < U; ++n2) {  // wave-uniform address: LDS broadcast
#pragma unroll
        for (int k = 0; k < D; ++k) {
          s[n2].p[k] = src[jj + n2].p[k];
          s[n2].v[k] = src[jj + n2].v[k];
          s[n2].a[k] = src[jj + n2].a[k];
        }
        s[n2].m = src[jj + n2].m;
      }
      pair_batch_hermite6<T, D, R, U>(acc, jacc, sacc, xi, vi, ai, s, pc, e2);
    }
  }

  // the four slices in wave order
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const int base             = ((wave - 1) * R + r) * 3 * D;
        hand[(base + k) * 64 + lane]         = acc[r][k];
        hand[(base + D + k) * 64 + lane]     = jacc[r][k];
        hand[(base + 2 * D + k) * 64 + lane] = sacc[r][k];
      }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int p = 1; p < kH6Waves; ++p)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const int base = ((p - 1) * R + r) * 3 * D;
          acc[r][k] += hand[(base + k) * 64 + lane];
          jacc[r][k] += hand[(base + D + k) * 64 + lane];
          sacc[r][k] += hand[(base + 2 * D + k) * 64 + lane];
        }
    T* out = part + uint64_t(blockIdx.y) * (3 * D) * n;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (ti[r] < n) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          out[uint64_t(k) * n + ti[r]]         = acc[r][k];
          out[uint64_t(D + k) * n + ti[r]]     = jacc[r][k];
          out[uint64_t(2 * D + k) * n + ti[r]] = sacc[r][k];
        }
      }
    }
  }
}

// ---- correct -------------------------------------------------------------------------------------------------------------------
// a1 = c * (chunk sums in chunk order), j1 and s1 likewise.  First start pass: a = a1.  Second: a = a1, jerk = j1, snap = s1, crackle = 0
// (the first step is one order lower, once).  Otherwise the corrector
//   v1 = v + h/2 (a0 + a1) + h^2/10 (j0 - j1) + h^3/120 (s0 + s1),  x1 = x + h/2 (v + v1) + h^2/10 (a0 - a1) + h^3/120 (j0 + j1)
// and the crackle at the new time, the third derivative at t1 of the quintic through (a0, j0, s0) and (a1, j1, s1):
//   k1 = (60 (a1 - a0) - h (24 j0 + 36 j1) + h^2 (9 s1 - 3 s0)) / h^3              (ih3 = 1 / h^3, made by the host as T)
// then a = a1, jerk = j1, snap = s1, crackle = k1.
template <typename T, int D, int MODE>
__global__ __launch_bounds__(kH6Block) void hermite6_correct_kernel(const T* __restrict__ part, T* __restrict__ x, T* __restrict__ v,
                                                                    T* __restrict__ a, T* __restrict__ jerk, T* __restrict__ snap,
                                                                    T* __restrict__ crackle, T c, T h, T ih3, uint32_t n, uint32_t chunks) {
  const uint32_t i = blockIdx.x * kH6Block + threadIdx.x;
  if (i >= n) return;
  const T hh = T(0.5) * h, h2 = h * h, h10 = h2 * T(0.1), h120 = (h2 * h) * T(1.0 / 120.0);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    T sa = part[uint64_t(k) * n + i], sj = part[uint64_t(D + k) * n + i], ss = part[uint64_t(2 * D + k) * n + i];
    for (uint32_t ch = 1; ch < chunks; ++ch) {
      sa += part[(uint64_t(ch) * (3 * D) + k) * n + i];
      sj += part[(uint64_t(ch) * (3 * D) + D + k) * n + i];
      ss += part[(uint64_t(ch) * (3 * D) + 2 * D + k) * n + i];
    }
    const T a1 = c * sa, j1 = c * sj, s1 = c * ss;
    const uint64_t e = uint64_t(i) * D + k;
    if constexpr (MODE == kH6StartA) {
      a[e] = a1;
    } else {
      T k1 = T(0);
      if constexpr (MODE == kH6Step) {
        const T a0 = a[e], j0 = jerk[e], s0 = snap[e], v0 = v[e];
        const T v1 = v0 + __builtin_elementwise_fma(hh, a0 + a1, __builtin_elementwise_fma(h10, j0 - j1, h120 * (s0 + s1)));
        x[e]       = x[e] + __builtin_elementwise_fma(hh, v0 + v1, __builtin_elementwise_fma(h10, a0 - a1, h120 * (j0 + j1)));
        v[e]       = v1;
        const T lin = T(24) * j0 + T(36) * j1, quad = T(9) * s1 - T(3) * s0;
        k1 = __builtin_elementwise_fma(h2, quad, __builtin_elementwise_fma(-h, lin, T(60) * (a1 - a0))) * ih3;
      }
      a[e]       = a1;
      jerk[e]    = j1;
      snap[e]    = s1;
      crackle[e] = k1;
    }
  }
}

}  // namespace nbody

using namespace nbody;

struct nbody_hermite6 {
  int dtype = 0, dim = 0, device = 0;  // device: nbody_hermite6_create_on's; every call runs there
  uint32_t n = 0, padded = 0;
  size_t tsz = 0;
  hermite6_plan plan{};
  void* recs    = nullptr;  // h6src_rec<T>[padded]
  void* part    = nullptr;  // T[chunks][3 D][n]
  void* jerk    = nullptr;  // T[n][D]
  void* snap    = nullptr;  // T[n][D]
  void* crackle = nullptr;  // T[n][D]
  bool started  = false;    // nbody_hermite6_start has run (host call order, which a recorded step replays)
};

namespace nbody {

template <typename T, int D, int R, int MODE>
static int hermite6_launch(nbody_hermite6* h, const nbody_state* s, T e2, hipStream_t st) {
  const hermite6_plan& p = h->plan;
  T* recs                = static_cast<T*>(h->recs);
  T* part                = static_cast<T*>(h->part);
  T *jerk = static_cast<T*>(h->jerk), *snap = static_cast<T*>(h->snap), *crackle = static_cast<T*>(h->crackle);
  const T dt  = static_cast<T>(s->dt);
  const T ih3 = T(1) / (dt * dt * dt);
  hipLaunchKernelGGL((hermite6_predict_kernel<T, D, MODE>), dim3(h->padded / kH6Block), dim3(kH6Block), 0, st,
                     static_cast<const T*>(s->m), static_cast<const T*>(s->x), static_cast<const T*>(s->v), static_cast<const T*>(s->a),
                     jerk, snap, crackle, recs, dt, h->n, h->padded);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((hermite6_pair_kernel<T, D, R>), dim3(p.blocks, p.chunks), dim3(kH6Block), 0, st, recs, part, e2, h->n, p.ntiles,
                     p.tiles_per_chunk);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((hermite6_correct_kernel<T, D, MODE>), dim3((h->n + kH6Block - 1) / kH6Block), dim3(kH6Block), 0, st, part,
                     static_cast<T*>(s->x), static_cast<T*>(s->v), static_cast<T*>(s->a), jerk, snap, crackle, static_cast<T>(s->c), dt, ih3,
                     h->n, p.chunks);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// the common head of start and step: every argument error before the device is touched, in the header's order
template <bool START>
static int hermite6_call(nbody_hermite6* h, const nbody_state* s, double eps, void* stream, const char* who) {
  if (int r = check_state(s)) return r;
  NB_ARG(s->first == 0 && s->count == s->sz, "%s needs the whole system (first = 0, count = sz), got [%u, %u+%u) of %u", who, s->first,
         s->first, s->count, s->sz);
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    T e2;
    if (int r = check_softening<T>(eps, &e2)) return r;
    NB_ARG(h != nullptr, "nbody_hermite6 is NULL");
    NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
           "nbody_hermite6 was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", h->dtype, h->dim, h->n,
           s->dtype, s->dim, s->sz);
    if (int r = check_same_device(h->device, as_stream(stream), "nbody_hermite6")) return r;
    if (!START && !h->started) {
      set_error("nbody_hermite6_step before nbody_hermite6_start on this handle");
      return int(NBODY_ERR_STATE);
    }
    device_guard guard(h->device);
    hipStream_t st = as_stream(stream);
    int r;
    if constexpr (START) {
      r = h->plan.R == 2 ? hermite6_launch<T, D, 2, kH6StartA>(h, s, e2, st) : hermite6_launch<T, D, 1, kH6StartA>(h, s, e2, st);
      if (r == NBODY_OK)
        r = h->plan.R == 2 ? hermite6_launch<T, D, 2, kH6Start>(h, s, e2, st) : hermite6_launch<T, D, 1, kH6Start>(h, s, e2, st);
      if (r == NBODY_OK) h->started = true;
    } else {
      r = h->plan.R == 2 ? hermite6_launch<T, D, 2, kH6Step>(h, s, e2, st) : hermite6_launch<T, D, 1, kH6Step>(h, s, e2, st);
    }
    return r;
  });
}

}  // namespace nbody

extern "C" int nbody_hermite6_create(nbody_hermite6** out, int dtype, int dim, uint32_t n) {
  return nbody_hermite6_create_on(out, dtype, dim, n, -1);
}

extern "C" int nbody_hermite6_create_on(nbody_hermite6** out, int dtype, int dim, uint32_t n, int device) {
  NB_ARG(out != nullptr, "out is NULL");
  *out = nullptr;
  NB_ARG(dtype == NBODY_F32 || dtype == NBODY_F64, "bad dtype %d", dtype);
  NB_ARG(dim == 2 || dim == 3, "bad dim %d", dim);
  NB_ARG(n >= 1 && n <= (1u << 28), "hermite6 needs 1 <= n <= 2^28 (got %u)", n);
  if (captures_on_this_thread() != 0) {
    set_error("nbody_hermite6_create allocates: it cannot be called between nbody_graph_begin and nbody_graph_end");
    return NBODY_ERR_STATE;
  }
  int ndev = 0;
  NB_HIP(hipGetDeviceCount(&ndev));
  if (device < 0) device = current_device();
  NB_ARG(device >= 0 && device < ndev, "device %d out of range (%d HIP devices visible)", device, ndev);
  device_guard guard(device);
  auto* h   = new nbody_hermite6;
  h->device = device;
  h->dtype  = dtype;
  h->dim    = dim;
  h->n      = n;
  h->tsz    = dtype == NBODY_F32 ? 4 : 8;
  h->plan   = hermite6_plan_for(n);
  h->padded = h->plan.ntiles * uint32_t(kH6Tile);
  const size_t row = h->tsz * size_t(dim) * size_t(n);
  hipError_t e     = hipMalloc(&h->recs, h->tsz * kH6Rec * size_t(h->padded));
  if (e == hipSuccess) e = hipMalloc(&h->part, size_t(h->plan.chunks) * 3 * row);
  if (e == hipSuccess) e = hipMalloc(&h->jerk, row);
  if (e == hipSuccess) e = hipMalloc(&h->snap, row);
  if (e == hipSuccess) e = hipMalloc(&h->crackle, row);
  // nothing is cleared: every launch sequence writes all of recs and part before it reads them, and the jerk, the snap and the crackle
  // are written by nbody_hermite6_start before nbody_hermite6_step or nbody_hermite6_read may run (see nbody_hermite_create_on)
  if (e != hipSuccess) {
    int r = hip_fail(e, "nbody_hermite6_create allocation", __FILE__, __LINE__);
    nbody_hermite6_destroy(h);
    return r;
  }
  *out = h;
  return NBODY_OK;
}

extern "C" void nbody_hermite6_destroy(nbody_hermite6* h) {
  if (!h) return;
  device_guard guard(h->device);
  (void)hipFree(h->recs);
  (void)hipFree(h->part);
  (void)hipFree(h->jerk);
  (void)hipFree(h->snap);
  (void)hipFree(h->crackle);
  delete h;
}

extern "C" int nbody_hermite6_start(nbody_hermite6* h, const nbody_state* s, double eps, void* stream) {
  return hermite6_call<true>(h, s, eps, stream, "nbody_hermite6_start");
}

extern "C" int nbody_hermite6_step(nbody_hermite6* h, const nbody_state* s, double eps, void* stream) {
  return hermite6_call<false>(h, s, eps, stream, "nbody_hermite6_step");
}

extern "C" int nbody_hermite6_read(nbody_hermite6* h, int what, void* host_out, size_t bytes, void* stream) {
  NB_ARG(h != nullptr, "nbody_hermite6 is NULL");
  NB_ARG(host_out != nullptr, "host_out is NULL");
  NB_ARG(what >= 0 && what <= 5, "what must be 0 (jerk), 1 (snap), 2 (crackle), 3, 4 or 5 (predicted x, v, a), got %d", what);
  const size_t row = h->tsz * size_t(h->dim);
  NB_ARG(bytes == row * size_t(h->n), "nbody_hermite6_read(what = %d) needs %zu bytes, got %zu", what, row * size_t(h->n), bytes);
  if (int r = check_same_device(h->device, as_stream(stream), "nbody_hermite6")) return r;
  device_guard guard(h->device);
  hipStream_t st = as_stream(stream);
  if (capture_id(st) != 0) {
    set_error("nbody_hermite6_read is blocking: it cannot be recorded (call it outside nbody_graph_begin/end)");
    return NBODY_ERR_STATE;
  }
  if (!h->started) {
    set_error("nbody_hermite6_read before nbody_hermite6_start on this handle");
    return NBODY_ERR_STATE;
  }
  if (what <= 2) {
    const void* src = what == 0 ? h->jerk : what == 1 ? h->snap : h->crackle;
    NB_HIP(hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, st));
  } else {  // D of the record's 12 values: xp at 0, vp at 4, ap at 8
    const char* src = static_cast<const char*>(h->recs) + size_t(what - 3) * 4 * h->tsz;
    NB_HIP(hipMemcpy2DAsync(host_out, row, src, kH6Rec * h->tsz, row, h->n, hipMemcpyDeviceToHost, st));
  }
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}
