// Sixth-order Hermite predictor-corrector (Nitadori & Makino 2008) for the direct sum: nbody_hermite6_* of include/nbody_hip.h.
// No reference counterpart.  Fixed dt, Plummer softening required (eps = 0 is refused, as in the fourth-order integrator of hermite.hip).
//
// Three launches per step (six for the start, which evaluates twice), all on the caller's stream, nothing allocated after
// nbody_hermite6_create:
//   predict          one lane per body: the packed source record {xp[3], m, vp[3], 0, ap[3], 0} (12 T; 2D zero-fills component 2) into the
//                    handle's record array, padded with zero-mass records to a whole number of tiles so that the pair kernel never tests a
//                    bound;
//   force+jerk+snap  the hot path: R targets per lane in registers, records staged through LDS tiles of kHTile and read as wave-uniform
//                    broadcasts, every tile split over the four waves of the block, the tiles split over grid.y chunks where the targets
//                    alone would not fill the chip; the block's four slices are added in wave order and the raw sums of the chunk go to
//                    the handle's partial array (always, also with one chunk: 3 D values per body beside O(N) pairs);
//   correct          one lane per body: adds the chunks' sums IN CHUNK ORDER, scales by c, applies the corrector and the crackle formula.
// The rounding order of a body's sums (slices of a tile by wave, tiles in order, waves in order, chunks in order) follows from sz
// alone: hermite_plan_for reads nothing else — not the device, not the CU count — so two runs, an eager step and a replayed one, and
// a handle destroyed and made again give the same bits.  No atomics on a, the jerk or the snap, no waiting between blocks.
// The plan (hermite_plan_for with at least two chunks), the record, the pair kernel's body (hermite_tile_sum with G = 3) and the
// host-side checks are hermite_tile.hpp's, shared with the fourth-order integrator.
#include "hermite_block_common.hpp"

namespace nbody {

constexpr int kH6Rec = 12;  // values per record: hermite_rec<T, 3>, {xp[3], m, vp[3], 0, ap[3], 0}

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
__global__ __launch_bounds__(kHBlock) void hermite6_predict_kernel(const T* __restrict__ m, const T* __restrict__ x, const T* __restrict__ v,
                                                                   const T* __restrict__ a, const T* __restrict__ jerk,
                                                                   const T* __restrict__ snap, const T* __restrict__ crackle,
                                                                   T* __restrict__ recs, T h, uint32_t n, uint32_t padded) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
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

// ---- force + jerk + snap -------------------------------------------------------------------------------------------------------
// grid (blocks of 64 R targets, chunks).  part: [chunk][3 D][n] raw sums (a's D components, then the jerk's, then the snap's), unscaled.
template <typename T, int D, int R>
__global__ __launch_bounds__(kHBlock) void hermite6_pair_kernel(const T* __restrict__ flat, T* __restrict__ part, T e2, uint32_t n,
                                                                uint32_t ntiles, uint32_t tiles_per_chunk) {
  hermite_tile_sum<T, D, R, 3, false>(flat, part, e2, n, ntiles, tiles_per_chunk, nullptr);
}

// ---- correct -------------------------------------------------------------------------------------------------------------------
// a1 = c * (chunk sums in chunk order), j1 and s1 likewise.  First start pass: a = a1.  Second: a = a1, jerk = j1, snap = s1, crackle = 0
// (the first step is one order lower, once).  Otherwise the corrector
//   v1 = v + h/2 (a0 + a1) + h^2/10 (j0 - j1) + h^3/120 (s0 + s1),  x1 = x + h/2 (v + v1) + h^2/10 (a0 - a1) + h^3/120 (j0 + j1)
// and the crackle at the new time, the third derivative at t1 of the quintic through (a0, j0, s0) and (a1, j1, s1):
//   k1 = (60 (a1 - a0) - h (24 j0 + 36 j1) + h^2 (9 s1 - 3 s0)) / h^3              (ih3 = 1 / h^3, made by the host as T)
// then a = a1, jerk = j1, snap = s1, crackle = k1.
template <typename T, int D, int MODE>
__global__ __launch_bounds__(kHBlock) void hermite6_correct_kernel(const T* __restrict__ part, T* __restrict__ x, T* __restrict__ v,
                                                                   T* __restrict__ a, T* __restrict__ jerk, T* __restrict__ snap,
                                                                   T* __restrict__ crackle, T c, T h, T ih3, uint32_t n, uint32_t chunks) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= n) return;
  const T hh = T(0.5) * h, h2 = h * h, h10 = h2 * T(0.1), h120 = (h2 * h) * T(1.0 / 120.0);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    T s[3];
    hermite_chunk_sums<T, D, 3>(s, part, c, n, i, chunks, k);
    const T a1 = s[0], j1 = s[1], s1 = s[2];
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

struct nbody_hermite6 : hermite_handle {  // started: nbody_hermite6_start has run
  void* jerk    = nullptr;  // T[n][D]
  void* snap    = nullptr;  // T[n][D]
  void* crackle = nullptr;  // T[n][D]
  hermite_block blk;  // block time steps (hermite6_block.inc): allocated by the first nbody_hermite6_block_start
};

namespace nbody {

template <typename T, int D, int R, int MODE>
static int hermite6_launch(nbody_hermite6* h, const nbody_state* s, T e2, hipStream_t st) {
  const hermite_plan& p = h->plan;
  T* recs               = static_cast<T*>(h->recs);
  T* part               = static_cast<T*>(h->part);
  T *jerk = static_cast<T*>(h->jerk), *snap = static_cast<T*>(h->snap), *crackle = static_cast<T*>(h->crackle);
  const T dt  = static_cast<T>(s->dt);
  const T ih3 = T(1) / (dt * dt * dt);
  hipLaunchKernelGGL((hermite6_predict_kernel<T, D, MODE>), dim3(h->padded / kHBlock), dim3(kHBlock), 0, st,
                     static_cast<const T*>(s->m), static_cast<const T*>(s->x), static_cast<const T*>(s->v), static_cast<const T*>(s->a),
                     jerk, snap, crackle, recs, dt, h->n, h->padded);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((hermite6_pair_kernel<T, D, R>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part, e2, h->n, p.ntiles,
                     p.tiles_per_chunk);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((hermite6_correct_kernel<T, D, MODE>), dim3((h->n + kHBlock - 1) / kHBlock), dim3(kHBlock), 0, st, part,
                     static_cast<T*>(s->x), static_cast<T*>(s->v), static_cast<T*>(s->a), jerk, snap, crackle, static_cast<T>(s->c), dt, ih3,
                     h->n, p.chunks);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// the common head of start and step: every argument error before the device is touched, in the header's order
template <bool START>
static int hermite6_call(nbody_hermite6* h, const nbody_state* s, double eps, void* stream, const char* who) {
  if (int r = hermite_check_state(s, who)) return r;
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    T e2;
    hipStream_t st = as_stream(stream);
    if (int r = hermite_check_call<T>(h, s, eps, st, "nbody_hermite6", who, START ? nullptr : "nbody_hermite6_start", &e2)) return r;
    device_guard guard(h->device);
    int r;
    if constexpr (START) {
      r = h->plan.R == 2 ? hermite6_launch<T, D, 2, kH6StartA>(h, s, e2, st) : hermite6_launch<T, D, 1, kH6StartA>(h, s, e2, st);
      if (r == NBODY_OK)
        r = h->plan.R == 2 ? hermite6_launch<T, D, 2, kH6Start>(h, s, e2, st) : hermite6_launch<T, D, 1, kH6Start>(h, s, e2, st);
      if (r == NBODY_OK) h->started = true;
      h->blk.block_on = false;  // levels and tau belong to the state nbody_hermite6_block_start saw
    } else {
      r = h->plan.R == 2 ? hermite6_launch<T, D, 2, kH6Step>(h, s, e2, st) : hermite6_launch<T, D, 1, kH6Step>(h, s, e2, st);
    }
    return r;
  });
}

}  // namespace nbody

#include "hermite6_block.inc"

extern "C" int nbody_hermite6_create(nbody_hermite6** out, int dtype, int dim, uint32_t n) {
  return nbody_hermite6_create_on(out, dtype, dim, n, -1);
}

extern "C" int nbody_hermite6_create_on(nbody_hermite6** out, int dtype, int dim, uint32_t n, int device) {
  if (int r = create_check_args(out, dtype, dim, n, 1, 1u << 28, "hermite6 needs 1 <= n <= 2^28 (got %u)")) return r;
  if (int r = create_check_device(&device, "hermite6", true)) return r;
  device_guard guard(device);
  auto* h = new nbody_hermite6;
  hermite_handle_alloc(h, dtype, dim, n, device, 3, 2);
  const size_t row = h->tsz * size_t(dim) * size_t(n);
  // not cleared either: the jerk, the snap and the crackle are written by nbody_hermite6_start before nbody_hermite6_step or
  // nbody_hermite6_read may run
  h->mem.alloc(&h->jerk, row);
  h->mem.alloc(&h->snap, row);
  h->mem.alloc(&h->crackle, row);
  return create_finish(out, h, nbody_hermite6_destroy, h->mem.error(), "nbody_hermite6_create allocation");
}

extern "C" void nbody_hermite6_destroy(nbody_hermite6* h) {
  if (!h) return;
  device_guard guard(h->device);
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
  // one of the handle's arrays, or a group of the records: xp (kRecP), vp (kRecV), ap (kRecA)
  const void* plain = what == 0 ? h->jerk : what == 1 ? h->snap : what == 2 ? h->crackle : nullptr;
  return hermite_read_rows(h, "nbody_hermite6", "nbody_hermite6_read", "nbody_hermite6_start", plain, what - 3, 3, host_out, bytes,
                           as_stream(stream));
}
