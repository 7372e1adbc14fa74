// Block (individual) time steps for the octree leapfrog: nbody_octree_block_* of include/nbody_hip.h.  Included by octree.hip after
// struct nbody_octree and the phase runners; the scheme (levels, ticks, the criterion) is stated in the header.
//
// One block step, on the caller's stream, with one 8-byte read-back:
//   schedule   min, count, scan, compact: block_schedule.hpp's four kernels over the body order — tau_next, then the active list;
//   predict    ALL bodies to tau_next into the handle's xp, h_i = T(tau_next - tau_i) * tick;
//   build      the tree on xp: bounds, keys + sort + cells, multipoles — the launches of a fixed step, on a view whose x is xp;
//   walk list  count / scan / compact again, over the key order the build has just produced (sidx = the sorted body indices);
//   walk       ot_force_softened_kernel as it is, through the walks' one launch (ot_walk_launch): list = the walk list, nlist = n_act,
//              x = xp, a = the handle's a1 — it writes the listed rows only;
//   kick       one lane per active body: v += h/2 (a + a1), x = xp, a = a1, the new level, tau.
// The host synchronises after the walk list is queued and sizes the last two launches from (n_act, tau_next).

namespace nbody {

constexpr int kOtbBlock = kSchedBlock;

// ---- the criterion ---------------------------------------------------------------------------------------------------------------
// want = sqrt(k / |a|), k = 2 eta eps (one T, from the host); a2 = |a|^2.  Callers test a2 > 0 first.
template <typename T>
__device__ __forceinline__ T otb_want(T k, T a2) {
  return __builtin_elementwise_sqrt(k / __builtin_elementwise_sqrt(a2));
}

// start: the smallest level whose step dtmax 2^-l is <= want, at most L (|a| = 0: level 0).  tau = 0.
template <typename T, int D>
__global__ __launch_bounds__(kOtbBlock) void otb_init_kernel(const T* __restrict__ a, int32_t* __restrict__ lev, uint32_t* __restrict__ tau,
                                                             T k, T dtmax, uint32_t n, int32_t L) {
  const uint32_t i = blockIdx.x * kOtbBlock + threadIdx.x;
  if (i >= n) return;
  T a2 = T(0);
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const T ac = a[uint64_t(i) * D + c];
    a2         = __builtin_elementwise_fma(ac, ac, a2);
  }
  lev[i] = a2 > T(0) ? block_first_level(otb_want(k, a2), dtmax, L) : 0;
  tau[i] = 0u;
}

// ---- predict: one lane per coordinate --------------------------------------------------------------------------------------------
// xp = x + h v + h^2/2 a as fma(h, fma(h/2, a, v), x): three roundings (h, the inner and the outer FMA; h/2 is exact).
template <typename T, int D>
__global__ __launch_bounds__(kOtbBlock) void otb_predict_kernel(const T* __restrict__ x, const T* __restrict__ v, const T* __restrict__ a,
                                                                const uint32_t* __restrict__ tau, const uint32_t* __restrict__ sched,
                                                                T* __restrict__ xp, T tick, uint32_t nd) {
  const uint32_t e = blockIdx.x * kOtbBlock + threadIdx.x;  // nd = n D <= 3 * 2^28
  if (e >= nd) return;
  const T h = T(sched[kSchedNext] - tau[e / uint32_t(D)]) * tick;
  xp[e]     = __builtin_elementwise_fma(h, __builtin_elementwise_fma(h * T(0.5), a[e], v[e]), x[e]);
}

// ---- kick + new level: one lane per active body -----------------------------------------------------------------------------------
// h = step_i * tick (an active body's tau_next - tau_i is its step).  v = fma(h/2, a0 + a1, v): three roundings with h's.
// New level: block_next_level with want = sqrt(k / |a1|) (|a1| = 0: no limit).
template <typename T, int D>
__global__ __launch_bounds__(kOtbBlock) void otb_kick_kernel(const uint32_t* __restrict__ act, const uint32_t* __restrict__ sched,
                                                             const T* __restrict__ xp, const T* __restrict__ a1, T* __restrict__ x,
                                                             T* __restrict__ v, T* __restrict__ a, int32_t* __restrict__ lev,
                                                             uint32_t* __restrict__ tau, T k, T tick, uint32_t n_act, uint32_t n,
                                                             int32_t L) {
  const uint32_t s = blockIdx.x * kOtbBlock + threadIdx.x;
  if (s >= n_act) return;
  const uint32_t i = act[s];
  if (i >= n) return;  // never: the list holds body indices
  const uint32_t next = sched[kSchedNext];
  const int32_t l     = lev[i];
  const uint32_t step = step_of(l, L);
  const T dt = T(step) * tick, hdt = T(0.5) * dt;
  T n2 = T(0);
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const uint64_t e = uint64_t(i) * D + c;
    const T a0 = a[e], an = a1[e];
    v[e] = __builtin_elementwise_fma(hdt, a0 + an, v[e]);
    x[e] = xp[e];
    a[e] = an;
    n2   = __builtin_elementwise_fma(an, an, n2);
  }
  lev[i] = n2 > T(0) ? block_next_level(otb_want(k, n2), true, dt, l, L, step, next) : block_next_level(T(0), false, dt, l, L, step, next);
  tau[i] = next == (1u << L) ? 0u : next;
}

}  // namespace nbody

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct nbody_octree_block {
  int dtype = 0, dim = 0, device = 0;  // device: nbody_octree_block_create_on's; every call runs there
  uint32_t n = 0;
  size_t tsz = 0;
  nbody::block_schedule sched;  // levels, tau, the active list in ascending body order, the schedule words
  uint32_t* wlist = nullptr;    // the active bodies in the tree's key order: what the walk takes, [n]
  void* xp        = nullptr;    // predicted positions of the last block step, T[n][D]
  void* a1        = nullptr;    // the walk's output: rows of the active bodies, T[n][D]
  bool on = false, stepped = false;  // start has run; a block step has run since
  nbody::device_buffers mem;    // owns the schedule's arrays, wlist, xp and a1
};

namespace nbody {

template <typename T>
struct otb_consts {
  T e2, k, tick, dtmax;
};

// The common head of start, step and advance: every argument error before the device is touched, in the header's order; then the
// call-sequence refusals.  A step takes the level count of the handle, not max_level.
template <typename T>
static int otb_check(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, double eps, double eta, bool is_start, int max_level,
                     hipStream_t st, const char* who, otb_consts<T>* out) {
  if (int r = check_softening<T>(eps, &out->e2)) return r;
  out->k = T(2) * T(eta) * T(eps);
  NB_ARG(eta > 0.0 && eta <= DBL_MAX && T(eta) > T(0) && out->k > T(0) && out->k <= (sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)),
         "%s: eta = %g must be finite and > 0, and 2 eta eps a positive finite number of the state's type", who, eta);
  if (is_start) NB_ARG(max_level >= 0 && max_level <= 20, "%s: max_level = %d must be in 0 .. 20", who, max_level);
  NB_ARG(h != nullptr, "nbody_octree_block is NULL");
  NB_ARG(t != nullptr, "nbody_octree is NULL");
  NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
         "nbody_octree_block was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", h->dtype, h->dim, h->n,
         s->dtype, s->dim, s->sz);
  NB_ARG(t->dtype == s->dtype && t->dim == s->dim && t->n == s->sz,
         "octree was created for (dtype=%d, dim=%d, n=%u), state is (%d, %d, %u)", t->dtype, t->dim, t->n, s->dtype, s->dim, s->sz);
  const int L = is_start ? max_level : h->sched.levels;
  out->dtmax  = T(s->dt);
  out->tick   = out->dtmax;
  for (int j = 0; j < L; ++j) out->tick *= T(0.5);
  NB_ARG(s->dt > 0.0 && s->dt <= DBL_MAX && out->tick >= (sizeof(T) == 4 ? T(FLT_MIN) : T(DBL_MIN)) &&
             out->dtmax <= (sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)),
         "%s: dt = %g must be finite and > 0, and dt / 2^%d a normal number", who, s->dt, L);
  if (int r = check_same_device(h->device, st, "nbody_octree_block")) return r;
  if (int r = check_same_device(t->device, st, "nbody_octree")) return r;
  if (capture_id(st) != 0) {
    set_error("%s %s: it cannot be called between nbody_graph_begin and nbody_graph_end", who,
              is_start ? "starts a run of block steps, which are not recordable" : "is blocking (it reads the size of the active set back)");
    return NBODY_ERR_STATE;
  }
  if (int r = ot_walk_refused(t, "softened")) return r;  // after nbody_octree_set_walk(t, 2): the softened walk's refusal
  if (!is_start) {
    if (!h->on) {
      set_error("%s before nbody_octree_block_start on this handle", who);
      return NBODY_ERR_STATE;
    }
    NB_ARG(s->dt == h->sched.dt, "%s: the state's dt = %g is not the dt = %g nbody_octree_block_start was called with", who, s->dt,
           h->sched.dt);
  }
  return NBODY_OK;
}

// bounds, insert, multipoles on the view `s` (clear has nothing to launch): the tree's phase flags as after the four phase calls
template <typename T, int D>
static int otb_build(nbody_octree* t, const nbody_state* s, hipStream_t st) {
  t->phase.cleared();
  if (int r = ot_bounds_run<T, D>(t, s, st)) return r;
  t->phase.bounds_done();
  if (int r = ot_insert_run<T, D>(t, s, st)) return r;
  t->phase.insert_done();
  if (int r = ot_tree_run<T, D>(t, st)) return r;
  t->phase.tree_done();
  return NBODY_OK;
}

template <typename T, int D>
static int otb_start_launch(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, const otb_consts<T>& bc, double theta, int L,
                            hipStream_t st) {
  h->on = h->stepped = false;
  if (int r = otb_build<T, D>(t, s, st)) return r;
  if (int r = ot_force_run<T, D>(t, s, theta, st, kOtSoft, bc.e2)) return r;
  hipLaunchKernelGGL((otb_init_kernel<T, D>), dim3((h->n + kOtbBlock - 1) / kOtbBlock), dim3(kOtbBlock), 0, st,
                     static_cast<const T*>(s->a), h->sched.lev, h->sched.tau, bc.k, bc.dtmax, h->n, int32_t(L));
  NB_HIP(hipGetLastError());
  if (int r = block_schedule_start(&h->sched, L, s->dt, st)) return r;
  h->on = true;
  return NBODY_OK;
}

// one block step; *n_active and *tau_next are always written on success
template <typename T, int D>
static int otb_step_launch(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, const otb_consts<T>& bc, double theta,
                           hipStream_t st, uint32_t* n_active, uint32_t* tau_next) {
  block_schedule& sc = h->sched;
  const int32_t L    = sc.levels;
  const uint32_t n   = h->n;
  T* xp              = static_cast<T*>(h->xp);
  T* a1              = static_cast<T*>(h->a1);
  if (int r = block_schedule_active(&sc, st)) return r;
  hipLaunchKernelGGL((otb_predict_kernel<T, D>), dim3((n * uint32_t(D) + kOtbBlock - 1) / kOtbBlock), dim3(kOtbBlock), 0, st,
                     static_cast<const T*>(s->x), static_cast<const T*>(s->v), static_cast<const T*>(s->a), sc.tau, sc.sched, xp, bc.tick,
                     n * uint32_t(D));
  NB_HIP(hipGetLastError());
  nbody_state sp = *s;  // the predicted system: the tree is built on it and the walk reads its positions
  sp.x           = xp;
  if (int r = otb_build<T, D>(t, &sp, st)) return r;
  if (int r = block_schedule_list(&sc, t->idx[t->sorted_buf], h->wlist, kSchedNext, false, st)) return r;
  NB_HIP(hipStreamSynchronize(st));
  uint32_t n_act, next;
  if (int r = block_schedule_pair(&sc, "nbody_octree", false, &n_act, &next)) {
    h->on = false;
    return r;
  }
  // the softened walk of ot_force_run, over the walk list, from xp into a1
  if (int r = ot_walk_launch<T, D>(t, ot_force_softened_kernel<T, D, false>, ot_force_softened_kernel<T, D, true>, h->wlist, n_act,
                                   static_cast<const T*>(xp), a1, static_cast<T>(s->c), 0u, theta, st, bc.e2))
    return r;
  hipLaunchKernelGGL((otb_kick_kernel<T, D>), dim3((n_act + kOtbBlock - 1) / kOtbBlock), dim3(kOtbBlock), 0, st, sc.act, sc.sched, xp, a1,
                     static_cast<T*>(s->x), static_cast<T*>(s->v), static_cast<T*>(s->a), sc.lev, sc.tau, bc.k, bc.tick, n_act, n, L);
  NB_HIP(hipGetLastError());
  sc.last    = n_act;
  h->stepped = true;
  *n_active  = n_act;
  *tau_next  = next;
  return NBODY_OK;
}

// start (is_start) | step (steps == nullptr) | advance (steps: {block steps, body steps})
static int otb_call(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, double theta, double eps, double eta, bool is_start,
                    int max_level, void* stream, const char* who, uint32_t* n_active, uint32_t* tau, uint64_t* steps) {
  if (int r = check_state(s)) return r;
  NB_ARG(s->first == 0 && s->count == s->sz, "%s needs the whole system (first = 0, count = sz), got [%u, %u+%u) of %u", who, s->first,
         s->first, s->count, s->sz);
  return dispatch(s->dtype, s->dim, [&](auto tg) -> int {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    otb_consts<T> bc;
    hipStream_t st = as_stream(stream);
    if (int r = otb_check<T>(h, t, s, eps, eta, is_start, max_level, st, who, &bc)) return r;
    device_guard guard(h->device);
    if (is_start) return otb_start_launch<T, D>(h, t, s, bc, theta, max_level, st);
    return block_schedule_run(
        &h->sched, [&](uint32_t* na, uint32_t* tn) { return otb_step_launch<T, D>(h, t, s, bc, theta, st, na, tn); }, n_active, tau, steps);
  });
}

}  // namespace nbody

extern "C" int nbody_octree_block_create(nbody_octree_block** out, int dtype, int dim, uint32_t n) {
  return nbody_octree_block_create_on(out, dtype, dim, n, -1);
}

extern "C" int nbody_octree_block_create_on(nbody_octree_block** out, int dtype, int dim, uint32_t n, int device) {
  if (int r = create_check_args(out, dtype, dim, n, 1, 1u << 28, "octree block steps need 1 <= n <= 2^28 (got %u)")) return r;
  if (int r = create_check_device(&device, "octree_block", true)) return r;
  device_guard guard(device);
  auto* h   = new nbody_octree_block;
  h->device = device;
  h->dtype  = dtype;
  h->dim    = dim;
  h->n      = n;
  h->tsz    = dtype == NBODY_F32 ? 4 : 8;
  const size_t rows = h->tsz * size_t(dim) * size_t(n);
  hipError_t e      = block_schedule_alloc(&h->sched, n, h->mem);
  h->mem.alloc(&h->wlist, sizeof(uint32_t) * size_t(n));
  h->mem.alloc(&h->xp, rows);
  h->mem.alloc(&h->a1, rows);
  if (e == hipSuccess) e = h->mem.error();
  // nothing is cleared: start writes lev, tau and the schedule words, and every block step writes xp, the lists and the listed rows
  // of a1 before it reads them
  return create_finish(out, h, nbody_octree_block_destroy, e, "nbody_octree_block_create allocation");
}

extern "C" void nbody_octree_block_destroy(nbody_octree_block* h) {
  if (!h) return;
  device_guard guard(h->device);
  delete h;
}

extern "C" int nbody_octree_block_start(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, double theta, double eps, double eta,
                                        int max_level, void* stream) {
  return nbody::otb_call(h, t, s, theta, eps, eta, true, max_level, stream, "nbody_octree_block_start", nullptr, nullptr, nullptr);
}

extern "C" int nbody_octree_block_step(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, double theta, double eps, double eta,
                                       void* stream, uint32_t* n_active, uint32_t* tau) {
  return nbody::otb_call(h, t, s, theta, eps, eta, false, 0, stream, "nbody_octree_block_step", n_active, tau, nullptr);
}

extern "C" int nbody_octree_block_advance(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, double theta, double eps,
                                          double eta, void* stream, uint64_t* block_steps, uint64_t* body_steps) {
  uint64_t steps[2] = {0, 0};
  const int r = nbody::otb_call(h, t, s, theta, eps, eta, false, 0, stream, "nbody_octree_block_advance", nullptr, nullptr, steps);
  if (r == NBODY_OK) {
    if (block_steps) *block_steps = steps[0];
    if (body_steps) *body_steps = steps[1];
  }
  return r;
}

extern "C" int nbody_octree_block_read(nbody_octree_block* h, int what, void* host_out, size_t bytes, void* stream) {
  NB_ARG(h != nullptr, "nbody_octree_block is NULL");
  NB_ARG(host_out != nullptr, "host_out is NULL");
  NB_ARG(what >= 0 && what <= 3,
         "what must be 0 (levels), 1 (tau), 2 (the active list of the last block step) or 3 (its predicted positions), got %d", what);
  if (int r = check_same_device(h->device, as_stream(stream), "nbody_octree_block")) return r;
  device_guard guard(h->device);
  hipStream_t st = as_stream(stream);
  if (capture_id(st) != 0) {
    set_error("nbody_octree_block_read is blocking: it cannot be recorded (call it outside nbody_graph_begin/end)");
    return NBODY_ERR_STATE;
  }
  if (!h->on || (what >= 2 && !h->stepped)) {
    set_error("nbody_octree_block_read(what = %d) before nbody_octree_block_%s on this handle", what, h->on ? "step" : "start");
    return NBODY_ERR_STATE;
  }
  size_t need     = h->tsz * size_t(h->dim) * size_t(h->n);
  const void* src = what == 3 ? h->xp : block_schedule_array(&h->sched, what, &need);
  NB_ARG(bytes == need, "nbody_octree_block_read(what = %d) needs %zu bytes, got %zu", what, need, bytes);
  if (need) NB_HIP(hipMemcpyAsync(host_out, src, need, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}
