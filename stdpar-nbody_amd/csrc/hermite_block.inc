// Block (individual) time steps for the Hermite integrator: nbody_hermite_block_* of include/nbody_hip.h.  Included by hermite.hip
// after struct nbody_hermite; the scheme (levels, ticks, the Aarseth criterion) is stated in the header.
//
// One block step is seven or eight launches on the caller's stream and one 8-byte read-back:
//   schedule   min, count, scan, compact: block_schedule.hpp's four kernels over the body order — tau_next, then the active indices
//              in ascending body order;
//   predict    ALL bodies to tau_next, h_i = T(tau_next - tau_i) * tick, the packed record of hermite_predict_kernel;
//   force+jerk the active targets, gathered through the list, against all N records: hermite_tile_sum (hermite_tile.hpp) as it is,
//              launched in the shape of hermite_block_plan_for(sz, n_act, 1);
//   reduce     only where the active set is cut into more than kSerialChunks chunks (fewer than 2048 active bodies of a large system):
//              hermite_block_reduce_kernel (hermite_block_common.hpp);
//   correct    one lane per active body: chunk sums in chunk order, the corrector with h = step_i * tick, the new level.
// `scan` writes (n_act, tau_next) into pinned host memory; the host synchronises after `predict` and sizes the last launches from it.

namespace nbody {

// ---- predict with per-body h -------------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(kHBlock) void hermite_block_predict_kernel(const T* __restrict__ m, const T* __restrict__ x, const T* __restrict__ v,
                                                                        const T* __restrict__ a, const T* __restrict__ jerk,
                                                                        const uint32_t* __restrict__ tau, const uint32_t* __restrict__ sched,
                                                                        hsrc_rec<T>* __restrict__ recs, T tick, uint32_t n, uint32_t padded) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= padded) return;
  hsrc_rec<T> r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r.g[kRecP][k] = r.g[kRecV][k] = T(0);
  if (i < n) {
    const T dt = T(sched[kSchedNext] - tau[i]) * tick;
    r.g[kRecP][kRecM] = m[i];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const uint64_t e = uint64_t(i) * D + k;
      const T a0 = a[e], j0 = jerk[e], v0 = v[e];
      r.g[kRecP][k] =
          __builtin_elementwise_fma(dt, __builtin_elementwise_fma(dt * T(0.5), __builtin_elementwise_fma(dt * T(1.0 / 3.0), j0, a0), v0), x[e]);
      r.g[kRecV][k] = __builtin_elementwise_fma(dt, __builtin_elementwise_fma(dt * T(0.5), j0, a0), v0);
    }
  }
  recs[i] = r;
}

// ---- force + jerk of the active set ----------------------------------------------------------------------------------------------
// grid (blocks of 64 R active slots, chunks).  part: [chunk][2 D][n_act] raw sums over the slots.
template <typename T, int D, int R>
__global__ __launch_bounds__(kHBlock) void hermite_block_active_kernel(const hsrc_rec<T>* __restrict__ recs, T* __restrict__ part, T e2,
                                                                       uint32_t n_act, uint32_t ntiles, uint32_t tiles_per_chunk,
                                                                       const uint32_t* __restrict__ act) {
  hermite_tile_sum<T, D, R, 2, true>(reinterpret_cast<const T*>(recs), part, e2, n_act, ntiles, tiles_per_chunk, act);
}

// ---- correct + new level ---------------------------------------------------------------------------------------------------------
// hermite_correct_kernel's corrector with h = step_i * tick, then from a0, j0 (old) and a1, j1 (new)
//   a2 = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2,  a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3,  a2 <- a2 + h a3
//   want = sqrt(eta (|a1| |a2| + |j1|^2) / (|j1| |a3| + |a2|^2))       (denominator 0: no limit)
// and block_next_level.  1 / h = 2^l / dtmax is idt * 2^l, an exact scaling of the host's idt = 1 / T(dtmax).
template <typename T, int D>
__global__ __launch_bounds__(kHBlock) void hermite_block_correct_kernel(const T* __restrict__ part, const uint32_t* __restrict__ act,
                                                                        const uint32_t* __restrict__ sched, T* __restrict__ x, T* __restrict__ v,
                                                                        T* __restrict__ a, T* __restrict__ jerk, int32_t* __restrict__ lev,
                                                                        uint32_t* __restrict__ tau, T c, T tick, T idt, T eta, uint32_t n_act,
                                                                        uint32_t chunks, int32_t L) {
  const uint32_t s = blockIdx.x * kHBlock + threadIdx.x;
  if (s >= n_act) return;
  const uint32_t i    = act[s];
  const uint32_t next = sched[kSchedNext];
  const int32_t l     = lev[i];
  const uint32_t step = step_of(l, L);
  const T dt = T(step) * tick, ih = idt * T(1u << l);
  const T hdt = T(0.5) * dt, dt12 = (dt * dt) * T(1.0 / 12.0), ih2 = ih * ih, ih3 = ih2 * ih;
  T n_a1 = T(0), n_j1 = T(0), n_a2 = T(0), n_a3 = T(0);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    T sa = part[uint64_t(k) * n_act + s], sj = part[uint64_t(D + k) * n_act + s];
    for (uint32_t ch = 1; ch < chunks; ++ch) {
      sa += part[(uint64_t(ch) * (2 * D) + k) * n_act + s];
      sj += part[(uint64_t(ch) * (2 * D) + D + k) * n_act + s];
    }
    const T a1 = c * sa, j1 = c * sj;
    const uint64_t e = uint64_t(i) * D + k;
    const T a0 = a[e], j0 = jerk[e], v0 = v[e];
    const T v1 = v0 + __builtin_elementwise_fma(hdt, a0 + a1, dt12 * (j0 - j1));
    x[e]       = x[e] + __builtin_elementwise_fma(hdt, v0 + v1, dt12 * (a0 - a1));
    v[e]       = v1;
    a[e]       = a1;
    jerk[e]    = j1;
    const T da = a0 - a1;
    const T a3 = (T(12) * da + T(6) * dt * (j0 + j1)) * ih3;
    const T a2 = (T(-6) * da - dt * (T(4) * j0 + T(2) * j1)) * ih2 + dt * a3;
    n_a1 = __builtin_elementwise_fma(a1, a1, n_a1);
    n_j1 = __builtin_elementwise_fma(j1, j1, n_j1);
    n_a2 = __builtin_elementwise_fma(a2, a2, n_a2);
    n_a3 = __builtin_elementwise_fma(a3, a3, n_a3);
  }
  // |j1|^2 and |a2|^2 are the sums themselves
  const T num = __builtin_elementwise_fma(__builtin_elementwise_sqrt(n_a1), __builtin_elementwise_sqrt(n_a2), n_j1);
  const T den = __builtin_elementwise_fma(__builtin_elementwise_sqrt(n_j1), __builtin_elementwise_sqrt(n_a3), n_a2);
  lev[i] = den > T(0) ? block_next_level(__builtin_elementwise_sqrt(eta * num / den), true, dt, l, L, step, next)
                      : block_next_level(T(0), false, dt, l, L, step, next);
  tau[i] = next == (1u << L) ? 0u : next;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
template <typename T>
struct block_consts {
  T e2, eta, tick, dtmax, idt;
};

// The common head of block_start and block_step: every argument error before the device is touched, in the header's order; then the
// two call-sequence refusals.  A step takes the level count of the handle, not max_level.
template <typename T>
static int hermite_block_check(nbody_hermite* h, const nbody_state* s, double eps, double eta, bool is_start, int max_level,
                               hipStream_t st, const char* who, block_consts<T>* out) {
  const char* eta_name = is_start ? "eta_start" : "eta";
  if (int r = check_softening<T>(eps, &out->e2)) return r;
  NB_ARG(eta > 0.0 && eta <= DBL_MAX && T(eta) > T(0), "%s: %s = %g must be finite and > 0", who, eta_name, eta);
  if (is_start) NB_ARG(max_level >= 0 && max_level <= 20, "%s: max_level = %d must be in 0 .. 20", who, max_level);
  NB_ARG(h != nullptr, "nbody_hermite is NULL");
  NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
         "nbody_hermite was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", h->dtype, h->dim, h->n,
         s->dtype, s->dim, s->sz);
  const int L = is_start ? max_level : h->blk.sched.levels;
  out->eta    = T(eta);
  out->dtmax  = T(s->dt);
  out->tick   = out->dtmax;
  for (int k = 0; k < L; ++k) out->tick *= T(0.5);
  out->idt = T(1) / out->dtmax;
  NB_ARG(s->dt > 0.0 && s->dt <= DBL_MAX && out->tick >= (sizeof(T) == 4 ? T(FLT_MIN) : T(DBL_MIN)) && out->idt > T(0) &&
             out->idt <= (sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)),
         "%s: dt = %g must be finite and > 0, and dt / 2^%d and 1 / dt normal numbers", who, s->dt, L);
  if (int r = check_same_device(h->device, st, "nbody_hermite")) return r;
  if (capture_id(st) != 0 || (is_start && captures_on_this_thread() != 0)) {
    set_error("%s %s: it cannot be called between nbody_graph_begin and nbody_graph_end", who,
              is_start ? "allocates on first use" : "is blocking (it reads the size of the active set back)");
    return NBODY_ERR_STATE;
  }
  if (!is_start) {
    if (!h->blk.block_on) {
      set_error("%s before nbody_hermite_block_start on this handle (or after a later nbody_hermite_force_jerk)", who);
      return NBODY_ERR_STATE;
    }
    NB_ARG(s->dt == h->blk.sched.dt, "%s: the state's dt = %g is not the dt = %g nbody_hermite_block_start was called with", who, s->dt,
           h->blk.sched.dt);
  }
  return NBODY_OK;
}

template <typename T, int D>
static int hermite_block_start_launch(nbody_hermite* h, const nbody_state* s, const block_consts<T>& bc, T eta_start, int L, hipStream_t st) {
  hermite_block& b = h->blk;
  if (int r = hermite_block_alloc(&b, h, 2, 1, "nbody_hermite_block_start allocation")) return r;
  const int r = h->plan.R == 2 ? hermite_launch<T, D, 2, true>(h, s, bc.e2, st) : hermite_launch<T, D, 1, true>(h, s, bc.e2, st);
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
template <typename T, int D>
static int hermite_block_step_launch(nbody_hermite* h, const nbody_state* s, const block_consts<T>& bc, hipStream_t st, uint32_t* n_active,
                                     uint32_t* tau_next) {
  hermite_block& b     = h->blk;
  block_schedule& sc   = b.sched;
  const int32_t L = sc.levels;
  const uint32_t n = h->n;
  T* jerk = static_cast<T*>(h->jerk);
  auto* recs = static_cast<hsrc_rec<T>*>(h->recs);
  T* part    = static_cast<T*>(b.bpart);
  if (int r = block_schedule_active(&sc, st)) return r;
  hipLaunchKernelGGL((hermite_block_predict_kernel<T, D>), dim3(h->padded / kHBlock), dim3(kHBlock), 0, st, static_cast<const T*>(s->m),
                     static_cast<const T*>(s->x), static_cast<const T*>(s->v), static_cast<const T*>(s->a), jerk, sc.tau, sc.sched, recs,
                     bc.tick, n, h->padded);
  NB_HIP(hipGetLastError());
  NB_HIP(hipStreamSynchronize(st));
  uint32_t n_act, next;
  hermite_plan p;
  bool reduce;
  if (int r = hermite_block_shape(&b, "nbody_hermite", 1, &n_act, &next, &p, &reduce)) return r;
  if (p.R == 2)
    hipLaunchKernelGGL((hermite_block_active_kernel<T, D, 2>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part, bc.e2, n_act,
                       p.ntiles, p.tiles_per_chunk, sc.act);
  else
    hipLaunchKernelGGL((hermite_block_active_kernel<T, D, 1>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part, bc.e2, n_act,
                       p.ntiles, p.tiles_per_chunk, sc.act);
  NB_HIP(hipGetLastError());
  uint32_t chunks = p.chunks;
  if (reduce) {
    T* out = part + uint64_t(p.chunks) * (2 * D) * n_act;
    hipLaunchKernelGGL((hermite_block_reduce_kernel<T>), dim3((2 * D * n_act + kHWaves - 1) / kHWaves), dim3(kHBlock), 0, st, part, out, n_act,
                       uint32_t(2 * D), p.chunks, (p.chunks + 63u) / 64u);
    NB_HIP(hipGetLastError());
    part   = out;
    chunks = 1;
  }
  hipLaunchKernelGGL((hermite_block_correct_kernel<T, D>), dim3((n_act + kHBlock - 1) / kHBlock), dim3(kHBlock), 0, st, part, sc.act,
                     sc.sched, static_cast<T*>(s->x), static_cast<T*>(s->v), static_cast<T*>(s->a), jerk, sc.lev, sc.tau,
                     static_cast<T>(s->c), bc.tick, bc.idt, bc.eta, n_act, chunks, L);
  NB_HIP(hipGetLastError());
  sc.last   = n_act;
  *n_active = n_act;
  *tau_next = next;
  return NBODY_OK;
}

// block_start (is_start) | block_step (steps == nullptr) | block_advance (steps: {block steps, body steps})
static int hermite_block_call(nbody_hermite* h, const nbody_state* s, double eps, double eta, bool is_start, int max_level, void* stream,
                              const char* who, uint32_t* n_active, uint32_t* tau, uint64_t* steps) {
  if (int r = hermite_check_state(s, who)) return r;
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    block_consts<T> bc;
    hipStream_t st = as_stream(stream);
    if (int r = hermite_block_check<T>(h, s, eps, eta, is_start, max_level, st, who, &bc)) return r;
    device_guard guard(h->device);
    if (is_start) return hermite_block_start_launch<T, D>(h, s, bc, T(eta), max_level, st);
    return block_schedule_run(
        &h->blk.sched, [&](uint32_t* na, uint32_t* tn) { return hermite_block_step_launch<T, D>(h, s, bc, st, na, tn); }, n_active, tau, steps);
  });
}

}  // namespace nbody

extern "C" int nbody_hermite_block_start(nbody_hermite* h, const nbody_state* s, double eps, double eta_start, int max_level, void* stream) {
  return nbody::hermite_block_call(h, s, eps, eta_start, true, max_level, stream, "nbody_hermite_block_start", nullptr, nullptr, nullptr);
}

extern "C" int nbody_hermite_block_step(nbody_hermite* h, const nbody_state* s, double eps, double eta, void* stream, uint32_t* n_active,
                                        uint32_t* tau) {
  return nbody::hermite_block_call(h, s, eps, eta, false, 0, stream, "nbody_hermite_block_step", n_active, tau, nullptr);
}

extern "C" int nbody_hermite_block_advance(nbody_hermite* h, const nbody_state* s, double eps, double eta, void* stream, uint64_t* block_steps,
                                           uint64_t* body_steps) {
  uint64_t steps[2] = {0, 0};
  const int r = nbody::hermite_block_call(h, s, eps, eta, false, 0, stream, "nbody_hermite_block_advance", nullptr, nullptr, steps);
  if (r == NBODY_OK) {
    if (block_steps) *block_steps = steps[0];
    if (body_steps) *body_steps = steps[1];
  }
  return r;
}

extern "C" int nbody_hermite_block_read(nbody_hermite* h, int what, void* host_out, size_t bytes, void* stream) {
  return nbody::hermite_block_read(h, h ? &h->blk : nullptr, "nbody_hermite", what, host_out, bytes, stream);
}
