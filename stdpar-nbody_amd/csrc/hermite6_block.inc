// Block (individual) time steps for the sixth-order Hermite integrator: nbody_hermite6_block_* of include/nbody_hip.h.  Included by
// hermite6.hip after struct nbody_hermite6; the scheme (the levels and ticks of nbody_hermite_block_*, the predictor with the crackle,
// the criterion of Nitadori & Makino 2008) is stated in the header.  NBODY_F64 only: the criterion takes a fifth difference of the
// force, which lies below float's rounding of the sums (DESIGN.md §7), so no float kernel is instantiated here.
//
// One block step is seven or eight launches on the caller's stream and one 8-byte read-back, as in hermite_block.inc:
//   schedule   min, count, scan, compact: block_schedule.hpp's four kernels over the body order;
//   predict    ALL bodies to tau_next, h_i = T(tau_next - tau_i) * tick, the 12-value record of hermite6_predict_kernel;
//   force+jerk+snap  the active targets, gathered through the list, against all N records: hermite_tile_sum<T, D, R, 3, true>, launched
//              in the shape of hermite_block_plan_for(sz, n_act, 2);
//   reduce     only where the active set is cut into more than kSerialChunks chunks: hermite_block_reduce_kernel
//              (hermite_block_common.hpp);
//   correct    one lane per active body: chunk sums in chunk order, the corrector and the crackle with h = step_i * tick, the new level.
// `scan` writes (n_act, tau_next) into pinned host memory; the host synchronises after `predict` and sizes the last launches from it.

namespace nbody {

// ---- predict with per-body h -------------------------------------------------------------------------------------------------------
// hermite6_predict_kernel's three Horner chains with h_i = T(tau_next - tau_i) * tick in place of h; the same record, the same padding.
template <typename T, int D>
__global__ __launch_bounds__(kHBlock) void hermite6_block_predict_kernel(const T* __restrict__ m, const T* __restrict__ x, const T* __restrict__ v,
                                                                         const T* __restrict__ a, const T* __restrict__ jerk,
                                                                         const T* __restrict__ snap, const T* __restrict__ crackle,
                                                                         const uint32_t* __restrict__ tau, const uint32_t* __restrict__ sched,
                                                                         T* __restrict__ recs, T tick, uint32_t n, uint32_t padded) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= padded) return;
  T r[kH6Rec];
#pragma unroll
  for (int k = 0; k < kH6Rec; ++k) r[k] = T(0);
  if (i < n) {
    const T h = T(sched[kSchedNext] - tau[i]) * tick;
    r[3]      = m[i];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const uint64_t e = uint64_t(i) * D + k;
      const T x0 = x[e], v0 = v[e], a0 = a[e], j0 = jerk[e], s0 = snap[e], k0 = crackle[e];
      auto fma = [](T p, T q, T s) { return __builtin_elementwise_fma(p, q, s); };
      r[k]     = fma(h, fma(h * T(0.5), fma(h * T(1.0 / 3.0), fma(h * T(0.25), fma(h * T(0.2), k0, s0), j0), a0), v0), x0);
      r[4 + k] = fma(h, fma(h * T(0.5), fma(h * T(1.0 / 3.0), fma(h * T(0.25), k0, s0), j0), a0), v0);
      r[8 + k] = fma(h, fma(h * T(0.5), fma(h * T(1.0 / 3.0), k0, s0), j0), a0);
    }
  }
#pragma unroll
  for (int k = 0; k < kH6Rec; ++k) recs[uint64_t(i) * kH6Rec + k] = r[k];
}

// ---- force + jerk + snap of the active set -----------------------------------------------------------------------------------------
// grid (blocks of 64 R active slots, chunks).  part: [chunk][3 D][n_act] raw sums over the slots.
template <typename T, int D, int R>
__global__ __launch_bounds__(kHBlock) void hermite6_block_active_kernel(const T* __restrict__ flat, T* __restrict__ part, T e2, uint32_t n_act,
                                                                        uint32_t ntiles, uint32_t tiles_per_chunk,
                                                                        const uint32_t* __restrict__ act) {
  hermite_tile_sum<T, D, R, 3, true>(flat, part, e2, n_act, ntiles, tiles_per_chunk, act);
}

// ---- correct + crackle + new level ---------------------------------------------------------------------------------------------------
// hermite6_correct_kernel's corrector and crackle with h = step_i * tick, then the derivatives at the new time of the quintic through
// (a0, j0, s0) at 0 and (a1, j1, s1) at h:
//   a3 = k1,   a4 = (360 (a1 - a0) - h (168 j0 + 192 j1) + h^2 (36 s1 - 24 s0)) / h^4,
//   a5 = (720 (a1 - a0) - 360 h (j0 + j1) + 60 h^2 (s1 - s0)) / h^5
//   want = eta ((|a1| |s1| + |j1|^2) / (|a3| |a5| + |a4|^2))^(1/6)                                         (denominator 0: no limit)
// and block_next_level.  1 / h = idt 2^l and 1 / h^3 = ih3_0 2^(3 l) are exact scalings of the host's idt = 1 / T(dtmax) and
// ih3_0 = 1 / (dtmax dtmax dtmax) (the latter as hermite6_launch makes its ih3).  One lane per active body, a few hundred at most of
// them per pair sum over N sources: the division and the cube root cost nothing that shows.
template <typename T, int D>
__global__ __launch_bounds__(kHBlock) void hermite6_block_correct_kernel(const T* __restrict__ part, const uint32_t* __restrict__ act,
                                                                         const uint32_t* __restrict__ sched, T* __restrict__ x, T* __restrict__ v,
                                                                         T* __restrict__ a, T* __restrict__ jerk, T* __restrict__ snap,
                                                                         T* __restrict__ crackle, int32_t* __restrict__ lev,
                                                                         uint32_t* __restrict__ tau, T c, T tick, T idt, T ih3_0, T eta,
                                                                         uint32_t n_act, uint32_t chunks, int32_t L) {
  const uint32_t s = blockIdx.x * kHBlock + threadIdx.x;
  if (s >= n_act) return;
  const uint32_t i     = act[s];
  const uint32_t next  = sched[kSchedNext];
  const int32_t l      = lev[i];
  const uint32_t step  = step_of(l, L);
  const T h = T(step) * tick, ih = idt * T(1u << l), ih3 = ih3_0 * T(1ull << (3 * l)), ih4 = ih3 * ih, ih5 = ih4 * ih;
  const T hh = T(0.5) * h, h2 = h * h, h10 = h2 * T(0.1), h120 = (h2 * h) * T(1.0 / 120.0);
  T n_a1 = T(0), n_j1 = T(0), n_s1 = T(0), n_a3 = T(0), n_a4 = T(0), n_a5 = T(0);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    T sum[3];
    hermite_chunk_sums<T, D, 3>(sum, part, c, n_act, s, chunks, k);
    const T a1 = sum[0], j1 = sum[1], s1 = sum[2];
    const uint64_t e = uint64_t(i) * D + k;
    const T a0 = a[e], j0 = jerk[e], s0 = snap[e], v0 = v[e];
    const T v1 = v0 + __builtin_elementwise_fma(hh, a0 + a1, __builtin_elementwise_fma(h10, j0 - j1, h120 * (s0 + s1)));
    x[e]       = x[e] + __builtin_elementwise_fma(hh, v0 + v1, __builtin_elementwise_fma(h10, a0 - a1, h120 * (j0 + j1)));
    v[e]       = v1;
    const T lin = T(24) * j0 + T(36) * j1, quad = T(9) * s1 - T(3) * s0;
    const T k1  = __builtin_elementwise_fma(h2, quad, __builtin_elementwise_fma(-h, lin, T(60) * (a1 - a0))) * ih3;
    a[e]        = a1;
    jerk[e]     = j1;
    snap[e]     = s1;
    crackle[e]  = k1;
    const T da   = a1 - a0;
    const T lin4 = T(168) * j0 + T(192) * j1, quad4 = T(36) * s1 - T(24) * s0;
    const T a4   = __builtin_elementwise_fma(h2, quad4, __builtin_elementwise_fma(-h, lin4, T(360) * da)) * ih4;
    const T a5   = __builtin_elementwise_fma(h2, T(60) * (s1 - s0), __builtin_elementwise_fma(-h, T(360) * (j0 + j1), T(720) * da)) * ih5;
    n_a1 = __builtin_elementwise_fma(a1, a1, n_a1);
    n_j1 = __builtin_elementwise_fma(j1, j1, n_j1);
    n_s1 = __builtin_elementwise_fma(s1, s1, n_s1);
    n_a3 = __builtin_elementwise_fma(k1, k1, n_a3);
    n_a4 = __builtin_elementwise_fma(a4, a4, n_a4);
    n_a5 = __builtin_elementwise_fma(a5, a5, n_a5);
  }
  // |j1|^2 and |a4|^2 are the sums themselves
  const T num = __builtin_elementwise_fma(__builtin_elementwise_sqrt(n_a1), __builtin_elementwise_sqrt(n_s1), n_j1);
  const T den = __builtin_elementwise_fma(__builtin_elementwise_sqrt(n_a3), __builtin_elementwise_sqrt(n_a5), n_a4);
  lev[i] = den > T(0) ? block_next_level(eta * cbrt(__builtin_elementwise_sqrt(num / den)), true, h, l, L, step, next)
                      : block_next_level(T(0), false, h, l, L, step, next);
  tau[i] = next == (1u << L) ? 0u : next;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct h6_block_consts {  // double: the only type the block steps are provided in
  double e2, eta, tick, dtmax, idt, ih3_0;
};

// The common head of block_start and block_step after the state, the whole-system rule and the dtype: every other argument error
// before the device is touched, in the header's order; then the call-sequence refusals.  A step takes the level count of the handle,
// not max_level.
static int hermite6_block_check(nbody_hermite6* h, const nbody_state* s, double eps, double eta, bool is_start, int max_level,
                                hipStream_t st, const char* who, h6_block_consts* out) {
  const char* eta_name = is_start ? "eta_start" : "eta";
  if (int r = check_softening<double>(eps, &out->e2)) return r;
  NB_ARG(eta > 0.0 && eta <= DBL_MAX, "%s: %s = %g must be finite and > 0", who, eta_name, eta);
  if (is_start) NB_ARG(max_level >= 0 && max_level <= 20, "%s: max_level = %d must be in 0 .. 20", who, max_level);
  NB_ARG(h != nullptr, "nbody_hermite6 is NULL");
  NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
         "nbody_hermite6 was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", h->dtype, h->dim, h->n,
         s->dtype, s->dim, s->sz);
  const int L = is_start ? max_level : h->blk.sched.levels;
  out->eta    = eta;
  out->dtmax  = s->dt;
  out->tick   = out->dtmax;
  for (int k = 0; k < L; ++k) out->tick *= 0.5;
  out->idt   = 1.0 / out->dtmax;
  out->ih3_0 = 1.0 / (out->dtmax * out->dtmax * out->dtmax);  // hermite6_launch's ih3, operation for operation
  const double ih3_deepest = out->ih3_0 * double(1ull << (3 * L));
  NB_ARG(s->dt > 0.0 && s->dt <= DBL_MAX && out->tick >= DBL_MIN && out->idt >= DBL_MIN && out->idt <= DBL_MAX && out->ih3_0 >= DBL_MIN &&
             ih3_deepest <= DBL_MAX,
         "%s: dt = %g must be finite and > 0, and dt / 2^%d, 1 / dt and 2^%d / dt^3 normal numbers", who, s->dt, L, 3 * L);
  if (int r = check_same_device(h->device, st, "nbody_hermite6")) return r;
  if (capture_id(st) != 0 || (is_start && captures_on_this_thread() != 0)) {
    set_error("%s %s: it cannot be called between nbody_graph_begin and nbody_graph_end", who,
              is_start ? "allocates on first use" : "is blocking (it reads the size of the active set back)");
    return NBODY_ERR_STATE;
  }
  if (!is_start) {
    if (!h->blk.block_on) {
      set_error("%s before nbody_hermite6_block_start on this handle (or after a later nbody_hermite6_start)", who);
      return NBODY_ERR_STATE;
    }
    NB_ARG(s->dt == h->blk.sched.dt, "%s: the state's dt = %g is not the dt = %g nbody_hermite6_block_start was called with", who, s->dt,
           h->blk.sched.dt);
  }
  return NBODY_OK;
}

template <int D>
static int hermite6_block_start_launch(nbody_hermite6* h, const nbody_state* s, const h6_block_consts& bc, double eta_start, int L,
                                       hipStream_t st) {
  using T          = double;
  hermite_block& b = h->blk;
  if (int r = hermite_block_alloc(&b, h, 3, 2, "nbody_hermite6_block_start allocation")) return r;
  b.block_on = false;
  int r = h->plan.R == 2 ? hermite6_launch<T, D, 2, kH6StartA>(h, s, bc.e2, st) : hermite6_launch<T, D, 1, kH6StartA>(h, s, bc.e2, st);
  if (r == NBODY_OK)
    r = h->plan.R == 2 ? hermite6_launch<T, D, 2, kH6Start>(h, s, bc.e2, st) : hermite6_launch<T, D, 1, kH6Start>(h, s, bc.e2, st);
  if (r != NBODY_OK) return r;
  h->started = true;
  hipLaunchKernelGGL((hermite_block_init_kernel<T, D>), dim3((h->n + kHBlock - 1) / kHBlock), dim3(kHBlock), 0, st,
                     static_cast<const T*>(s->a), static_cast<const T*>(h->jerk), b.sched.lev, b.sched.tau, eta_start, bc.dtmax, h->n,
                     int32_t(L));
  NB_HIP(hipGetLastError());
  if (int r2 = block_schedule_start(&b.sched, L, s->dt, st)) return r2;
  b.block_on = true;
  return NBODY_OK;
}

// one block step; *n_active and *tau_next are always written on success
template <int D>
static int hermite6_block_step_launch(nbody_hermite6* h, const nbody_state* s, const h6_block_consts& bc, hipStream_t st, uint32_t* n_active,
                                      uint32_t* tau_next) {
  using T            = double;
  hermite_block& b   = h->blk;
  block_schedule& sc = b.sched;
  const int32_t L    = sc.levels;
  const uint32_t n   = h->n;
  T *jerk = static_cast<T*>(h->jerk), *snap = static_cast<T*>(h->snap), *crackle = static_cast<T*>(h->crackle);
  T* recs = static_cast<T*>(h->recs);
  T* part = static_cast<T*>(b.bpart);
  if (int r = block_schedule_active(&sc, st)) return r;
  hipLaunchKernelGGL((hermite6_block_predict_kernel<T, D>), dim3(h->padded / kHBlock), dim3(kHBlock), 0, st, static_cast<const T*>(s->m),
                     static_cast<const T*>(s->x), static_cast<const T*>(s->v), static_cast<const T*>(s->a), jerk, snap, crackle, sc.tau,
                     sc.sched, recs, bc.tick, n, h->padded);
  NB_HIP(hipGetLastError());
  NB_HIP(hipStreamSynchronize(st));
  uint32_t n_act, next;
  hermite_plan p;
  bool reduce;
  if (int r = hermite_block_shape(&b, "nbody_hermite6", 2, &n_act, &next, &p, &reduce)) return r;
  if (p.R == 2)
    hipLaunchKernelGGL((hermite6_block_active_kernel<T, D, 2>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part, bc.e2, n_act,
                       p.ntiles, p.tiles_per_chunk, sc.act);
  else
    hipLaunchKernelGGL((hermite6_block_active_kernel<T, D, 1>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part, bc.e2, n_act,
                       p.ntiles, p.tiles_per_chunk, sc.act);
  NB_HIP(hipGetLastError());
  uint32_t chunks = p.chunks;
  if (reduce) {
    T* out = part + uint64_t(p.chunks) * (3 * D) * n_act;
    hipLaunchKernelGGL((hermite_block_reduce_kernel<T>), dim3((3 * D * n_act + kHWaves - 1) / kHWaves), dim3(kHBlock), 0, st, part, out, n_act,
                       uint32_t(3 * D), p.chunks, (p.chunks + 63u) / 64u);
    NB_HIP(hipGetLastError());
    part   = out;
    chunks = 1;
  }
  hipLaunchKernelGGL((hermite6_block_correct_kernel<T, D>), dim3((n_act + kHBlock - 1) / kHBlock), dim3(kHBlock), 0, st, part, sc.act,
                     sc.sched, static_cast<T*>(s->x), static_cast<T*>(s->v), static_cast<T*>(s->a), jerk, snap, crackle, sc.lev, sc.tau,
                     static_cast<T>(s->c), bc.tick, bc.idt, bc.ih3_0, bc.eta, n_act, chunks, L);
  NB_HIP(hipGetLastError());
  sc.last   = n_act;
  *n_active = n_act;
  *tau_next = next;
  return NBODY_OK;
}

// block_start (is_start) | block_step (steps == nullptr) | block_advance (steps: {block steps, body steps})
static int hermite6_block_call(nbody_hermite6* h, const nbody_state* s, double eps, double eta, bool is_start, int max_level, void* stream,
                               const char* who, uint32_t* n_active, uint32_t* tau, uint64_t* steps) {
  if (int r = hermite_check_state(s, who)) return r;
  NB_ARG(s->dtype == NBODY_F64,
         "%s needs NBODY_F64: the step criterion takes a fifth difference of the force, which is below float's rounding of the force "
         "sums (a float run falls to the deepest level); use nbody_hermite6_step or nbody_hermite_block_* in float", who);
  h6_block_consts bc;
  hipStream_t st = as_stream(stream);
  if (int r = hermite6_block_check(h, s, eps, eta, is_start, max_level, st, who, &bc)) return r;
  device_guard guard(h->device);
  auto run = [&](auto dim_tag) -> int {
    constexpr int D = decltype(dim_tag)::value;
    if (is_start) return hermite6_block_start_launch<D>(h, s, bc, eta, max_level, st);
    return block_schedule_run(
        &h->blk.sched, [&](uint32_t* na, uint32_t* tn) { return hermite6_block_step_launch<D>(h, s, bc, st, na, tn); }, n_active, tau, steps);
  };
  return s->dim == 2 ? run(std::integral_constant<int, 2>{}) : run(std::integral_constant<int, 3>{});
}

}  // namespace nbody

extern "C" int nbody_hermite6_block_start(nbody_hermite6* h, const nbody_state* s, double eps, double eta_start, int max_level, void* stream) {
  return nbody::hermite6_block_call(h, s, eps, eta_start, true, max_level, stream, "nbody_hermite6_block_start", nullptr, nullptr, nullptr);
}

extern "C" int nbody_hermite6_block_step(nbody_hermite6* h, const nbody_state* s, double eps, double eta, void* stream, uint32_t* n_active,
                                         uint32_t* tau) {
  return nbody::hermite6_block_call(h, s, eps, eta, false, 0, stream, "nbody_hermite6_block_step", n_active, tau, nullptr);
}

extern "C" int nbody_hermite6_block_advance(nbody_hermite6* h, const nbody_state* s, double eps, double eta, void* stream,
                                            uint64_t* block_steps, uint64_t* body_steps) {
  uint64_t steps[2] = {0, 0};
  const int r = nbody::hermite6_block_call(h, s, eps, eta, false, 0, stream, "nbody_hermite6_block_advance", nullptr, nullptr, steps);
  if (r == NBODY_OK) {
    if (block_steps) *block_steps = steps[0];
    if (body_steps) *body_steps = steps[1];
  }
  return r;
}

extern "C" int nbody_hermite6_block_read(nbody_hermite6* h, int what, void* host_out, size_t bytes, void* stream) {
  return nbody::hermite_block_read(h, h ? &h->blk : nullptr, "nbody_hermite6", what, host_out, bytes, stream);
}
