// Fourth-order Hermite predictor-corrector (Makino & Aarseth 1992) for the direct sum: nbody_hermite_* of include/nbody_hip.h.
// No reference counterpart (the reference integrates with one leapfrog step, K3).  Fixed dt, Plummer softening required
// (eps = 0 is refused: without softening the pair term needs K1's near-pair forms, which have no jerk twin here).
//
// Three launches per step, all on the caller's stream, nothing allocated after nbody_hermite_create:
//   predict     one lane per body: the packed source record {xp[3], m, vp[3], 0} (8 T; 2D zero-fills component 2) into the handle's
//               record array, padded with zero-mass records to a whole number of tiles so that the pair kernel never tests a bound;
//   force+jerk  the hot path: R targets per lane in registers, records staged through LDS tiles of kHTile and read as wave-uniform
//               broadcasts, every tile split over the four waves of the block, the tiles split over grid.y chunks where the targets
//               alone would not fill the chip; the block's four slices are added in wave order and the raw sums of the chunk go to
//               the handle's partial array (always, also with one chunk: 2 D values per body beside O(N) pairs);
//   correct     one lane per body: adds the chunks' sums IN CHUNK ORDER, scales by c, applies the corrector.
// The rounding order of a body's sums (slices of a tile by wave, tiles in order, waves in order, chunks in order) follows from sz
// alone: hermite_plan_for reads nothing else — not the device, not the CU count — so two runs, an eager step and a replayed one, and
// a handle destroyed and made again give the same bits.  No atomics on a or the jerk, no waiting between blocks.
// Block (individual) time steps on the same handle: hermite_block.inc, included below (the schedule: block_schedule.hpp).  The plan,
// the record, the pair kernel's body (hermite_tile_sum with G = 2) and the host-side checks are hermite_tile.hpp's, shared with the
// sixth-order integrator, as is hermite_block_common.hpp, through which both come in.
#include "hermite_block_common.hpp"

namespace nbody {

template <typename T>
using hsrc_rec = hermite_rec<T, 2>;  // {xp[3], m, vp[3], 0}

// ---- predict -------------------------------------------------------------------------------------------------------------------
// START: the records of the state as it is (force_jerk at (x, v)); otherwise the predictor
//   xp = x + dt v + dt^2/2 a0 + dt^3/6 j0,  vp = v + dt a0 + dt^2/2 j0      (Horner in dt).
template <typename T, int D, bool START>
__global__ __launch_bounds__(kHBlock) void hermite_predict_kernel(const T* __restrict__ m, const T* __restrict__ x, const T* __restrict__ v,
                                                                  const T* __restrict__ a, const T* __restrict__ jerk,
                                                                  hsrc_rec<T>* __restrict__ recs, T dt, uint32_t n, uint32_t padded) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= padded) return;
  hsrc_rec<T> r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r.g[kRecP][k] = r.g[kRecV][k] = T(0);
  if (i < n) {
    r.g[kRecP][kRecM] = m[i];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const uint64_t e = uint64_t(i) * D + k;
      if constexpr (START) {
        r.g[kRecP][k] = x[e];
        r.g[kRecV][k] = v[e];
      } else {
        const T a0 = a[e], j0 = jerk[e], v0 = v[e];
        r.g[kRecP][k] =
            __builtin_elementwise_fma(dt, __builtin_elementwise_fma(dt * T(0.5), __builtin_elementwise_fma(dt * T(1.0 / 3.0), j0, a0), v0), x[e]);
        r.g[kRecV][k] = __builtin_elementwise_fma(dt, __builtin_elementwise_fma(dt * T(0.5), j0, a0), v0);
      }
    }
  }
  recs[i] = r;
}

// ---- force + jerk --------------------------------------------------------------------------------------------------------------
// grid (blocks of 64 R targets, chunks).  part: [chunk][2 D][n] raw sums (a's D components, then the jerk's), unscaled.
template <typename T, int D, int R>
__global__ __launch_bounds__(kHBlock) void hermite_force_jerk_kernel(const hsrc_rec<T>* __restrict__ recs, T* __restrict__ part, T e2,
                                                                     uint32_t n, uint32_t ntiles, uint32_t tiles_per_chunk) {
  hermite_tile_sum<T, D, R, 2, false>(reinterpret_cast<const T*>(recs), part, e2, n, ntiles, tiles_per_chunk, nullptr);
}

// ---- correct -------------------------------------------------------------------------------------------------------------------
// a1 = c * (chunk sums in chunk order), j1 likewise.  START: a = a1, jerk = j1.  Otherwise the corrector
//   v1 = v + dt/2 (a0 + a1) + dt^2/12 (j0 - j1),  x1 = x + dt/2 (v + v1) + dt^2/12 (a0 - a1),  then a = a1, jerk = j1.
template <typename T, int D, bool START>
__global__ __launch_bounds__(kHBlock) void hermite_correct_kernel(const T* __restrict__ part, T* __restrict__ x, T* __restrict__ v,
                                                                  T* __restrict__ a, T* __restrict__ jerk, T c, T dt, uint32_t n,
                                                                  uint32_t chunks) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= n) return;
  const T hdt = T(0.5) * dt, dt12 = (dt * dt) * T(1.0 / 12.0);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    T s[2];
    hermite_chunk_sums<T, D, 2>(s, part, c, n, i, chunks, k);
    const T a1 = s[0], j1 = s[1];
    const uint64_t e = uint64_t(i) * D + k;
    if constexpr (!START) {
      const T a0 = a[e], j0 = jerk[e], v0 = v[e];
      const T v1 = v0 + __builtin_elementwise_fma(hdt, a0 + a1, dt12 * (j0 - j1));
      x[e]       = x[e] + __builtin_elementwise_fma(hdt, v0 + v1, dt12 * (a0 - a1));
      v[e]       = v1;
    }
    a[e]    = a1;
    jerk[e] = j1;
  }
}

}  // namespace nbody

using namespace nbody;

struct nbody_hermite : hermite_handle {  // started: nbody_hermite_force_jerk has run
  void* jerk = nullptr;  // T[n][D]
  hermite_block blk;  // block time steps (hermite_block.inc): allocated by the first nbody_hermite_block_start
};

namespace nbody {

template <typename T, int D, int R, bool START>
static int hermite_launch(nbody_hermite* h, const nbody_state* s, T e2, hipStream_t st) {
  const hermite_plan& p = h->plan;
  auto* recs            = static_cast<hsrc_rec<T>*>(h->recs);
  T* part               = static_cast<T*>(h->part);
  T* jerk               = static_cast<T*>(h->jerk);
  const T dt            = static_cast<T>(s->dt);
  hipLaunchKernelGGL((hermite_predict_kernel<T, D, START>), dim3(h->padded / kHBlock), dim3(kHBlock), 0, st, static_cast<const T*>(s->m),
                     static_cast<const T*>(s->x), static_cast<const T*>(s->v), static_cast<const T*>(s->a), jerk, recs, dt, h->n,
                     h->padded);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((hermite_force_jerk_kernel<T, D, R>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part, e2, h->n,
                     p.ntiles, p.tiles_per_chunk);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((hermite_correct_kernel<T, D, START>), dim3((h->n + kHBlock - 1) / kHBlock), dim3(kHBlock), 0, st, part,
                     static_cast<T*>(s->x), static_cast<T*>(s->v), static_cast<T*>(s->a), jerk, static_cast<T>(s->c), dt, h->n, p.chunks);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// the common head of force_jerk and step: every argument error before the device is touched, in the header's order
template <bool START>
static int hermite_call(nbody_hermite* h, const nbody_state* s, double eps, void* stream, const char* who) {
  if (int r = hermite_check_state(s, who)) return r;
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    T e2;
    if (int r = hermite_check_call<T>(h, s, eps, as_stream(stream), "nbody_hermite", who, START ? nullptr : "nbody_hermite_force_jerk", &e2))
      return r;
    device_guard guard(h->device);
    const int r = h->plan.R == 2 ? hermite_launch<T, D, 2, START>(h, s, e2, as_stream(stream))
                                 : hermite_launch<T, D, 1, START>(h, s, e2, as_stream(stream));
    if (START && r == NBODY_OK) h->started = true;
    if (START) h->blk.block_on = false;  // levels and tau belong to the state nbody_hermite_block_start saw
    return r;
  });
}

}  // namespace nbody

#include "hermite_block.inc"

extern "C" int nbody_hermite_create(nbody_hermite** out, int dtype, int dim, uint32_t n) {
  return nbody_hermite_create_on(out, dtype, dim, n, -1);
}

extern "C" int nbody_hermite_create_on(nbody_hermite** out, int dtype, int dim, uint32_t n, int device) {
  if (int r = create_check_args(out, dtype, dim, n, 1, 1u << 28, "hermite needs 1 <= n <= 2^28 (got %u)")) return r;
  if (int r = create_check_device(&device, "hermite", true)) return r;
  device_guard guard(device);
  auto* h = new nbody_hermite;
  hermite_handle_alloc(h, dtype, dim, n, device, 2, 1);
  // not cleared either: the jerk is written by nbody_hermite_force_jerk before nbody_hermite_step or nbody_hermite_read may run
  h->mem.alloc(&h->jerk, h->tsz * size_t(dim) * size_t(n));
  return create_finish(out, h, nbody_hermite_destroy, h->mem.error(), "nbody_hermite_create allocation");
}

extern "C" void nbody_hermite_destroy(nbody_hermite* h) {
  if (!h) return;
  device_guard guard(h->device);
  delete h;
}

extern "C" int nbody_hermite_force_jerk(nbody_hermite* h, const nbody_state* s, double eps, void* stream) {
  return hermite_call<true>(h, s, eps, stream, "nbody_hermite_force_jerk");
}

extern "C" int nbody_hermite_step(nbody_hermite* h, const nbody_state* s, double eps, void* stream) {
  return hermite_call<false>(h, s, eps, stream, "nbody_hermite_step");
}

extern "C" int nbody_hermite_read(nbody_hermite* h, int what, void* host_out, size_t bytes, void* stream) {
  NB_ARG(h != nullptr, "nbody_hermite is NULL");
  NB_ARG(host_out != nullptr, "host_out is NULL");
  NB_ARG(what >= 0 && what <= 2, "what must be 0 (jerk), 1 (predicted x) or 2 (predicted v), got %d", what);
  const size_t row = h->tsz * size_t(h->dim);
  NB_ARG(bytes == row * size_t(h->n), "nbody_hermite_read(what = %d) needs %zu bytes, got %zu", what, row * size_t(h->n), bytes);
  // the jerk, or a group of the records: xp (kRecP), vp (kRecV)
  return hermite_read_rows(h, "nbody_hermite", "nbody_hermite_read", "nbody_hermite_force_jerk", what == 0 ? h->jerk : nullptr, what - 1, 2,
                           host_out, bytes, as_stream(stream));
}
