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
// alone: hermite_plan reads nothing else — not the device, not the CU count — so two runs, an eager step and a replayed one, and
// a handle destroyed and made again give the same bits.  No atomics on a or the jerk, no waiting between blocks.
// Block (individual) time steps on the same handle: hermite_block.inc, included below; the body of the force + jerk kernel is
// hermite_pair_body.inc, shared with the kernel of the active set.
#include "common.hpp"

namespace nbody {

constexpr int kHBlock = 256;  // 4 waves: one group of 64 R targets, the tile cut in four
constexpr int kHWaves = kHBlock / 64;
constexpr int kHTile  = 256;  // source records per LDS tile (fixed: the rounding order depends on it); one record per lane to stage

// source record of the pair kernel: 64 B in double (four ds_read_b128), 32 B in float (two)
template <typename T>
struct alignas(sizeof(T) * 8) hsrc_rec {
  T p[3];  // predicted position, D used
  T m;
  T v[3];  // predicted velocity, D used
  T pad;
};

// Launch shape, from sz alone.  R: targets per lane; chunks x tiles_per_chunk >= ntiles: the cut of the source range over grid.y.
// From 65536 bodies on two targets per lane still leave every SIMD two waves; below, one target per lane and as many chunks as bring
// the grid to about 2048 blocks (8 per CU of the largest part), at most 64 and at most one per tile.
struct hermite_plan {
  uint32_t R, blocks, ntiles, chunks, tiles_per_chunk;
};
inline hermite_plan hermite_plan_for(uint32_t sz) {
  hermite_plan p;
  p.R      = sz >= 65536u ? 2u : 1u;
  p.blocks = (sz + 64u * p.R - 1u) / (64u * p.R);
  p.ntiles = (sz + kHTile - 1u) / kHTile;
  uint32_t want = (2048u + p.blocks - 1u) / p.blocks;
  if (want > 64u) want = 64u;
  if (want > p.ntiles) want = p.ntiles;
  if (want < 1u) want = 1u;
  p.tiles_per_chunk = (p.ntiles + want - 1u) / want;
  p.chunks          = (p.ntiles + p.tiles_per_chunk - 1u) / p.tiles_per_chunk;
  return p;
}

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
  for (int k = 0; k < 3; ++k) r.p[k] = r.v[k] = T(0);
  r.m = r.pad = T(0);
  if (i < n) {
    r.m = m[i];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const uint64_t e = uint64_t(i) * D + k;
      if constexpr (START) {
        r.p[k] = x[e];
        r.v[k] = v[e];
      } else {
        const T a0 = a[e], j0 = jerk[e], v0 = v[e];
        r.p[k] = __builtin_elementwise_fma(dt, __builtin_elementwise_fma(dt * T(0.5), __builtin_elementwise_fma(dt * T(1.0 / 3.0), j0, a0), v0), x[e]);
        r.v[k] = __builtin_elementwise_fma(dt, __builtin_elementwise_fma(dt * T(0.5), j0, a0), v0);
      }
    }
  }
  recs[i] = r;
}

// ---- the pair ------------------------------------------------------------------------------------------------------------------
// U records against the R targets of a lane, stage by stage like pair_batch_soft (independent chains in flight).  With d = x_j - x_i,
// u = v_j - v_i, q = |d|^2 + e2 (the softened K1's FMA chain seeded with e2), du = d.u (FMA chain):
//   acc  += w d,                w = m q^(-3/2)            — soft_weight's arithmetic, operation for operation
//   jacc += w (u + alpha d),    alpha = -3 du / q
// from the ONE reciprocal square root y = rsq(q) the force takes.  Double: A = fl(y y), e = fl(1 - q A) (one FMA: the exact residual
// of the ROUNDED A up to 2^-76), so 1 / q = A / (1 - e) = A (1 + e + e^2 + O(e^3)), e <= 2^-23:
//   B = -3 A (<= 1/2 ulp beyond A's), alpha' = fma(B, fma(e, e, e), B) (truncation 2^-69, one rounding), alpha = du alpha' (one rounding):
//   alpha is within 2 ulp of -3 fl(d.u) / q, against w's <= 2.5 ulp of m q^(-3/2); t = fma(alpha, d, u) rounds once.  The jerk's
//   pair term fl-error is therefore <= 2.5 ulp on its w u part and <= 5 ulp on its w alpha d part.
// Float: A = y y from the 1-ulp v_rsq_f32 is 1 / q within 2.5 ulp — the size of m y^3's own ~3 ulp — and takes no correction.
// Self pair, coincident bodies at equal velocity, zero-mass padding: d = 0 (and u = 0) or w = 0 add exactly 0; q >= e2 keeps all finite.
template <typename T, int D, int R, int U>
__device__ __forceinline__ void pair_batch_hermite(T (&acc)[R][D], T (&jacc)[R][D], const T (&xi)[R][D], const T (&vi)[R][D],
                                                   const hsrc_rec<T> (&s)[U], const pair_consts<T>& pc, T e2) {
  T d[U][R][D], u[U][R][D], q[U][R], du[U][R], w[U][R], al[U][R];
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int k = 0; k < D; ++k) {
        d[b][r][k] = s[b].p[k] - xi[r][k];
        u[b][r][k] = s[b].v[k] - vi[r][k];
      }
      T t = e2;
#pragma unroll
      for (int k = 0; k < D; ++k) t = __builtin_elementwise_fma(d[b][r][k], d[b][r][k], t);
      q[b][r] = t;
      T g = d[b][r][0] * u[b][r][0];
#pragma unroll
      for (int k = 1; k < D; ++k) g = __builtin_elementwise_fma(d[b][r][k], u[b][r][k], g);
      du[b][r] = g;
    }
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (sizeof(T) == 8) {
        const double y  = __builtin_amdgcn_rsq(q[b][r]);
        const double A  = y * y;
        const double e  = __builtin_fma(-q[b][r], A, 1.0);
        const double y3 = A * y;
        const double p  = __builtin_fma(e, pc.k1875, pc.k15);
        const double g  = p * e;
        const double my = s[b].m * y3;
        w[b][r]         = __builtin_fma(my, g, my);  // == pair_math<double>::weight_far<false>
        const double B  = -3.0 * A;
        const double ap = __builtin_fma(B, __builtin_fma(e, e, e), B);
        al[b][r]        = du[b][r] * ap;
      } else {
        const float y = __builtin_amdgcn_rsqf(q[b][r]);
        const float A = y * y;
        w[b][r]       = s[b].m * (A * y);  // == soft_weight<float>
        al[b][r]      = du[b][r] * (-3.0f * A);
      }
    }
#pragma unroll
  for (int b = 0; b < U; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const T t  = __builtin_elementwise_fma(al[b][r], d[b][r][k], u[b][r][k]);
        acc[r][k]  = __builtin_elementwise_fma(w[b][r], d[b][r][k], acc[r][k]);
        jacc[r][k] = __builtin_elementwise_fma(w[b][r], t, jacc[r][k]);
      }
}

// ---- force + jerk --------------------------------------------------------------------------------------------------------------
// grid (blocks of 64 R targets, chunks).  part: [chunk][2 D][n] raw sums (a's D components, then the jerk's), unscaled.
template <typename T, int D, int R>
__global__ __launch_bounds__(kHBlock) void hermite_force_jerk_kernel(const hsrc_rec<T>* __restrict__ recs, T* __restrict__ part, T e2,
                                                                     uint32_t n, uint32_t ntiles, uint32_t tiles_per_chunk) {
#define HFJ_GATHER 0
#include "hermite_pair_body.inc"
#undef HFJ_GATHER
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
    T sa = part[uint64_t(k) * n + i], sj = part[uint64_t(D + k) * n + i];
    for (uint32_t ch = 1; ch < chunks; ++ch) {
      sa += part[(uint64_t(ch) * (2 * D) + k) * n + i];
      sj += part[(uint64_t(ch) * (2 * D) + D + k) * n + i];
    }
    const T a1 = c * sa, j1 = c * sj;
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

struct nbody_hermite {
  int dtype = 0, dim = 0, device = 0;  // device: nbody_hermite_create_on's; every call runs there
  uint32_t n = 0, padded = 0;
  size_t tsz = 0;
  hermite_plan plan{};
  void* recs = nullptr;  // hsrc_rec<T>[padded]
  void* part = nullptr;  // T[chunks][2 D][n]
  void* jerk = nullptr;  // T[n][D]
  bool started = false;  // nbody_hermite_force_jerk has run (host call order, which a recorded step replays)
  // block time steps (hermite_block.inc): allocated by the first nbody_hermite_block_start
  int32_t* blev    = nullptr;  // level l_i, [n]
  uint32_t* btau   = nullptr;  // last update time tau_i in ticks, [n]
  uint32_t* bact   = nullptr;  // active list of the block step in flight, ascending, [n]
  uint32_t* bcount = nullptr;  // active bodies per schedule strip, then its exclusive scan, [bstrips]
  uint32_t* bsched = nullptr;  // {running minimum, n_act, tau_next, -}
  uint32_t* bpin   = nullptr;  // pinned, mapped host memory: {n_act, tau_next}, written by the schedule
  uint32_t* bpin_dev = nullptr;  // its device address
  void* bpart      = nullptr;  // T[bslots][2 D]: partial sums of the active set, sized for the worst n_act
  uint32_t bstrips = 0, blast = 0;  // blast: n_act of the last block step
  uint64_t bslots  = 0;
  int blevels      = 0;      // max_level of the last block_start
  double bdt       = 0.0;    // its s->dt
  bool block_on    = false;  // nbody_hermite_block_start has run and no nbody_hermite_force_jerk since
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
  if (int r = check_state(s)) return r;
  NB_ARG(s->first == 0 && s->count == s->sz, "%s needs the whole system (first = 0, count = sz), got [%u, %u+%u) of %u", who, s->first,
         s->first, s->count, s->sz);
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    T e2;
    if (int r = check_softening<T>(eps, &e2)) return r;
    NB_ARG(h != nullptr, "nbody_hermite is NULL");
    NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
           "nbody_hermite was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", h->dtype, h->dim, h->n,
           s->dtype, s->dim, s->sz);
    if (int r = check_same_device(h->device, as_stream(stream), "nbody_hermite")) return r;
    if (!START && !h->started) {
      set_error("nbody_hermite_step before nbody_hermite_force_jerk on this handle");
      return int(NBODY_ERR_STATE);
    }
    device_guard guard(h->device);
    const int r = h->plan.R == 2 ? hermite_launch<T, D, 2, START>(h, s, e2, as_stream(stream))
                                 : hermite_launch<T, D, 1, START>(h, s, e2, as_stream(stream));
    if (START && r == NBODY_OK) h->started = true;
    if (START) h->block_on = false;  // levels and tau belong to the state nbody_hermite_block_start saw
    return r;
  });
}

}  // namespace nbody

#include "hermite_block.inc"

extern "C" int nbody_hermite_create(nbody_hermite** out, int dtype, int dim, uint32_t n) {
  return nbody_hermite_create_on(out, dtype, dim, n, -1);
}

extern "C" int nbody_hermite_create_on(nbody_hermite** out, int dtype, int dim, uint32_t n, int device) {
  NB_ARG(out != nullptr, "out is NULL");
  *out = nullptr;
  NB_ARG(dtype == NBODY_F32 || dtype == NBODY_F64, "bad dtype %d", dtype);
  NB_ARG(dim == 2 || dim == 3, "bad dim %d", dim);
  NB_ARG(n >= 1 && n <= (1u << 28), "hermite needs 1 <= n <= 2^28 (got %u)", n);
  if (captures_on_this_thread() != 0) {
    set_error("nbody_hermite_create allocates: it cannot be called between nbody_graph_begin and nbody_graph_end");
    return NBODY_ERR_STATE;
  }
  int ndev = 0;
  NB_HIP(hipGetDeviceCount(&ndev));
  if (device < 0) device = current_device();
  NB_ARG(device >= 0 && device < ndev, "device %d out of range (%d HIP devices visible)", device, ndev);
  device_guard guard(device);
  auto* h   = new nbody_hermite;
  h->device = device;
  h->dtype  = dtype;
  h->dim    = dim;
  h->n      = n;
  h->tsz    = dtype == NBODY_F32 ? 4 : 8;
  h->plan   = hermite_plan_for(n);
  h->padded = h->plan.ntiles * uint32_t(kHTile);
  hipError_t e = hipMalloc(&h->recs, h->tsz * 8 * size_t(h->padded));
  if (e == hipSuccess) e = hipMalloc(&h->part, h->tsz * size_t(h->plan.chunks) * 2 * size_t(dim) * size_t(n));
  if (e == hipSuccess) e = hipMalloc(&h->jerk, h->tsz * size_t(dim) * size_t(n));
  // nothing is cleared: every launch sequence writes all of recs and part before it reads them, and the jerk is written by
  // nbody_hermite_force_jerk before nbody_hermite_step or nbody_hermite_read may run.  (A memset here would be ordered against the
  // NULL stream only, not against the non-blocking stream of a context, and could land after the first predict.)
  if (e != hipSuccess) {
    int r = hip_fail(e, "nbody_hermite_create allocation", __FILE__, __LINE__);
    nbody_hermite_destroy(h);
    return r;
  }
  *out = h;
  return NBODY_OK;
}

extern "C" void nbody_hermite_destroy(nbody_hermite* h) {
  if (!h) return;
  device_guard guard(h->device);
  (void)hipFree(h->recs);
  (void)hipFree(h->part);
  (void)hipFree(h->jerk);
  hermite_block_free(h);
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
  if (int r = check_same_device(h->device, as_stream(stream), "nbody_hermite")) return r;
  device_guard guard(h->device);
  hipStream_t st = as_stream(stream);
  if (capture_id(st) != 0) {
    set_error("nbody_hermite_read is blocking: it cannot be recorded (call it outside nbody_graph_begin/end)");
    return NBODY_ERR_STATE;
  }
  if (!h->started) {
    set_error("nbody_hermite_read before nbody_hermite_force_jerk on this handle");
    return NBODY_ERR_STATE;
  }
  if (what == 0) {
    NB_HIP(hipMemcpyAsync(host_out, h->jerk, bytes, hipMemcpyDeviceToHost, st));
  } else {  // D of the record's 8 values: xp at 0, vp at 4
    const char* src = static_cast<const char*>(h->recs) + (what == 2 ? 4 * h->tsz : 0);
    NB_HIP(hipMemcpy2DAsync(host_out, row, src, 8 * h->tsz, row, h->n, hipMemcpyDeviceToHost, st));
  }
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}
