// Block (individual) time steps for the octree leapfrog: nbody_octree_block_* of include/nbody_hip.h.  Included by octree.hip after
// struct nbody_octree and the phase runners; the scheme (levels, ticks, the criterion) is stated in the header.
//
// One block step, on the caller's stream, with one 8-byte read-back:
//   schedule   min        tau_next = min_i(tau_i + step_i): strips of kOtbStrip bodies, wave and block minimum, one atomicMin of an
//                         unsigned integer per block (a minimum does not depend on the order it is taken in);
//              count      due bodies (tau_i + step_i == tau_next) per strip of POSITIONS of an order: the body order (sidx == NULL)
//                         or the tree's key order (sidx = the sorted body indices);
//              scan       ONE block: exclusive scan of the strips' counts; the body-order pass publishes (n_act, tau_next) to the
//                         schedule words and to pinned host memory and re-arms the minimum;
//              compact    the due bodies of the order, order kept: the strip's offset + the counts of the earlier rows and waves of
//                         the strip + the lane's rank in its wave's ballot.  No atomics: a slot follows from lev and tau alone;
//   predict    ALL bodies to tau_next into the handle's xp, h_i = T(tau_next - tau_i) * tick;
//   build      the tree on xp: bounds, keys + sort + cells, multipoles — the launches of a fixed step, on a view whose x is xp;
//   walk list  count / scan / compact again, over the key order the build has just produced;
//   walk       ot_force_softened_kernel as it is, list = the walk list, nlist = n_act, x = xp, a = the handle's a1: it writes the
//              listed rows only;
//   kick       one lane per active body: v += h/2 (a + a1), x = xp, a = a1, the new level, tau.
// The host synchronises after the walk list is queued and sizes the last two launches from (n_act, tau_next).

namespace nbody {

constexpr int kOtbBlock      = 256;
constexpr int kOtbWaves      = kOtbBlock / 64;
constexpr int kOtbItems      = 16;                     // rows of kOtbBlock positions per schedule strip
constexpr uint32_t kOtbStrip = kOtbBlock * kOtbItems;  // 4096 positions per schedule block
constexpr uint32_t kOtbNoTime = 0xffffffffu;

// sched[0]: the running minimum (kOtbNoTime between steps), sched[1]: n_act, sched[2]: tau_next of the step in flight
enum { kOtbMin = 0, kOtbCount = 1, kOtbNext = 2, kOtbWords = 4 };

__device__ __forceinline__ uint32_t otb_step_of(int32_t lev, int32_t L) { return 1u << (L - lev); }

// ---- schedule ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOtbBlock) void otb_sched_min_kernel(const int32_t* __restrict__ lev, const uint32_t* __restrict__ tau,
                                                                  uint32_t* __restrict__ sched, uint32_t n, int32_t L) {
  __shared__ uint32_t wmin[kOtbWaves];
  uint32_t mn = kOtbNoTime;
#pragma unroll
  for (int k = 0; k < kOtbItems; ++k) {
    const uint32_t i = blockIdx.x * kOtbStrip + k * kOtbBlock + threadIdx.x;
    if (i < n) {
      const uint32_t due = tau[i] + otb_step_of(lev[i], L);
      mn                 = due < mn ? due : mn;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = __shfl_xor(mn, off);
    mn               = o < mn ? o : mn;
  }
  if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kOtbWaves; ++w) mn = wmin[w] < mn ? wmin[w] : mn;
    atomicMin(&sched[kOtbMin], mn);
  }
}

// position p of the order -> its body (sidx == NULL: the body order itself); true when that body is due at `next`
__device__ __forceinline__ bool otb_due(const int32_t* lev, const uint32_t* tau, const uint32_t* sidx, uint32_t p, uint32_t n, int32_t L,
                                        uint32_t next, uint32_t* body) {
  if (p >= n) return false;
  const uint32_t i = sidx ? sidx[p] : p;
  *body            = i;
  return i < n && tau[i] + otb_step_of(lev[i], L) == next;  // (i < n always: the sort's indices are a permutation)
}

// `word`: the schedule word that holds tau_next — kOtbMin before the body-order scan has published it, kOtbNext after
__global__ __launch_bounds__(kOtbBlock) void otb_list_count_kernel(const int32_t* __restrict__ lev, const uint32_t* __restrict__ tau,
                                                                   const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ sched,
                                                                   int word, uint32_t* __restrict__ bcount, uint32_t n, int32_t L) {
  __shared__ uint32_t wcnt[kOtbWaves];
  const uint32_t next = sched[word];
  uint32_t c = 0, body = 0;
#pragma unroll
  for (int k = 0; k < kOtbItems; ++k) {
    const uint32_t p = blockIdx.x * kOtbStrip + k * kOtbBlock + threadIdx.x;
    c += uint32_t(__popcll(__ballot(otb_due(lev, tau, sidx, p, n, L, next, &body))));
  }
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kOtbWaves; ++w) c += wcnt[w];
    bcount[blockIdx.x] = c;
  }
}

__device__ __forceinline__ uint32_t otb_wave_inclusive_scan(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

// one block: bcount[0 .. nb) -> its exclusive scan in place.  publish: the total to sched[kOtbCount] and the host, tau_next to
// sched[kOtbNext], and the running minimum re-armed for the next step (its readers of this step have finished: stream order)
__global__ __launch_bounds__(kOtbBlock) void otb_list_scan_kernel(uint32_t* __restrict__ bcount, uint32_t* __restrict__ sched,
                                                                  uint32_t* __restrict__ host_pair, uint32_t nb, int publish) {
  __shared__ uint32_t wsum[kOtbWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t running = 0;
  for (uint32_t base = 0; base < nb; base += kOtbBlock) {
    const uint32_t j   = base + threadIdx.x;
    const uint32_t v   = j < nb ? bcount[j] : 0u;
    const uint32_t inc = otb_wave_inclusive_scan(v, lane);
    __syncthreads();  // the previous round's wsum has been read
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kOtbWaves; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (j < nb) bcount[j] = running + before + inc - v;
    running += total;
  }
  if (publish && threadIdx.x == 0) {
    const uint32_t next = sched[kOtbMin];
    sched[kOtbCount]    = running;
    sched[kOtbNext]     = next;
    sched[kOtbMin]      = kOtbNoTime;
    host_pair[0]        = running;  // pinned host memory: read by the host after it has synchronised with the stream
    host_pair[1]        = next;
  }
}

__global__ __launch_bounds__(kOtbBlock) void otb_list_compact_kernel(const int32_t* __restrict__ lev, const uint32_t* __restrict__ tau,
                                                                     const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ sched,
                                                                     const uint32_t* __restrict__ boff, uint32_t* __restrict__ out,
                                                                     uint32_t n, int32_t L) {
  __shared__ uint32_t cnt[kOtbItems * kOtbWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t next = sched[kOtbNext];
  uint64_t ballot[kOtbItems];
  uint32_t body[kOtbItems];
#pragma unroll
  for (int k = 0; k < kOtbItems; ++k) {
    const uint32_t p = blockIdx.x * kOtbStrip + k * kOtbBlock + threadIdx.x;
    body[k]          = 0u;
    ballot[k]        = __ballot(otb_due(lev, tau, sidx, p, n, L, next, &body[k]));
    if (lane == 0) cnt[k * kOtbWaves + wave] = uint32_t(__popcll(ballot[k]));
  }
  __syncthreads();
  if (wave == 0) {  // exclusive scan of the 64 (row, wave) counts, in position order
    const uint32_t v = cnt[lane];
    cnt[lane]        = otb_wave_inclusive_scan(v, lane) - v;
  }
  __syncthreads();
  const uint32_t base  = boff[blockIdx.x];
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < kOtbItems; ++k) {
    if ((ballot[k] >> lane) & 1ull) {
      const uint32_t slot = base + cnt[k * kOtbWaves + wave] + uint32_t(__popcll(ballot[k] & below));
      if (slot < n) out[slot] = body[k];  // slot < n always: n_act <= n
    }
  }
}

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
  int32_t l = 0;
  if (a2 > T(0)) {
    const T want = otb_want(k, a2);
    T hs         = dtmax;
    while (l < L && hs > want) {
      hs *= T(0.5);
      ++l;
    }
  }
  lev[i] = l;
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
  const T h = T(sched[kOtbNext] - tau[e / uint32_t(D)]) * tick;
  xp[e]     = __builtin_elementwise_fma(h, __builtin_elementwise_fma(h * T(0.5), a[e], v[e]), x[e]);
}

// ---- kick + new level: one lane per active body -----------------------------------------------------------------------------------
// h = step_i * tick (an active body's tau_next - tau_i is its step).  v = fma(h/2, a0 + a1, v): three roundings with h's.
// New level from want = sqrt(k / |a1|) (|a1| = 0: no limit): if want < h, the smallest level deeper than l whose step is <= want, at
// most L; else if want >= 2 h, l > 0 and tau_next lies on the coarser level's grid, l - 1; else l.
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
  const uint32_t next = sched[kOtbNext];
  const int32_t l     = lev[i];
  const uint32_t step = otb_step_of(l, L);
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
  const bool coarser_grid = l > 0 && (next & (2u * step - 1u)) == 0u;
  int32_t nl = l;
  if (n2 > T(0)) {
    const T want = otb_want(k, n2);
    if (want < dt) {
      T hs = hdt;
      nl   = l + 1;
      while (nl < L && hs > want) {
        hs *= T(0.5);
        ++nl;
      }
      if (nl > L) nl = L;
    } else if (want >= T(2) * dt && coarser_grid) {
      nl = l - 1;  // one doubling at most, and only onto the coarser level's grid
    }
  } else if (coarser_grid) {
    nl = l - 1;  // no limit
  }
  lev[i] = nl;
  tau[i] = next == (1u << L) ? 0u : next;
}

}  // namespace nbody

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct nbody_octree_block {
  int dtype = 0, dim = 0, device = 0;  // device: nbody_octree_block_create_on's; every call runs there
  uint32_t n = 0, strips = 0;
  size_t tsz = 0;
  int32_t* lev     = nullptr;  // level l_i, [n]
  uint32_t* tau    = nullptr;  // last update time tau_i in ticks, [n]
  uint32_t* act    = nullptr;  // active list of the last block step, ascending body order, [n]
  uint32_t* wlist  = nullptr;  // the same bodies in the tree's key order: what the walk takes, [n]
  uint32_t* bcount = nullptr;  // due bodies per schedule strip, then its exclusive scan, [strips]
  uint32_t* sched  = nullptr;  // {running minimum, n_act, tau_next, -}
  uint32_t* pin    = nullptr;  // pinned, mapped host memory: {n_act, tau_next}, written by the schedule
  uint32_t* pin_dev = nullptr;  // its device address
  void* xp         = nullptr;  // predicted positions of the last block step, T[n][D]
  void* a1         = nullptr;  // the walk's output: rows of the active bodies, T[n][D]
  uint32_t last    = 0;        // n_act of the last block step
  int levels       = 0;        // max_level of the last start
  double dt        = 0.0;      // its s->dt
  bool on = false, stepped = false;  // start has run; a block step has run since
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
  const int L = is_start ? max_level : h->levels;
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
  if (int r = ot_soft_walk_form(t)) return r;  // after nbody_octree_set_walk(t, 2): the softened walk's refusal
  if (!is_start) {
    if (!h->on) {
      set_error("%s before nbody_octree_block_start on this handle", who);
      return NBODY_ERR_STATE;
    }
    NB_ARG(s->dt == h->dt, "%s: the state's dt = %g is not the dt = %g nbody_octree_block_start was called with", who, s->dt, h->dt);
  }
  return NBODY_OK;
}

// bounds, insert, multipoles on the view `s` (clear has nothing to launch): the tree's phase flags as after the four phase calls
template <typename T, int D>
static int otb_build(nbody_octree* t, const nbody_state* s, hipStream_t st) {
  t->inserted = t->have_tree = t->have_quad = false;
  if (int r = ot_bounds_run<T, D>(t, s, st)) return r;
  t->have_bounds = true;
  if (int r = ot_insert_run<T, D>(t, s, st)) return r;
  t->inserted = true;
  if (int r = ot_tree_run<T, D>(t, st)) return r;
  t->have_tree = true;
  return NBODY_OK;
}

template <typename T, int D>
static int otb_start_launch(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, const otb_consts<T>& bc, double theta, int L,
                            hipStream_t st) {
  h->on = h->stepped = false;
  if (int r = otb_build<T, D>(t, s, st)) return r;
  if (int r = ot_force_run<T, D>(t, s, theta, st, true, bc.e2)) return r;
  hipLaunchKernelGGL((otb_init_kernel<T, D>), dim3((h->n + kOtbBlock - 1) / kOtbBlock), dim3(kOtbBlock), 0, st,
                     static_cast<const T*>(s->a), h->lev, h->tau, bc.k, bc.dtmax, h->n, int32_t(L));
  NB_HIP(hipGetLastError());
  NB_HIP(hipMemsetAsync(h->sched, 0xff, sizeof(uint32_t) * kOtbWords, st));
  h->levels = L;
  h->dt     = s->dt;
  h->last   = 0;
  h->on     = true;
  return NBODY_OK;
}

// count, scan, compact of the due bodies over one order; word: where tau_next is while `count` runs
static int otb_list(nbody_octree_block* h, const uint32_t* sidx, uint32_t* out, int word, bool publish, hipStream_t st) {
  const int32_t L = h->levels;
  hipLaunchKernelGGL(otb_list_count_kernel, dim3(h->strips), dim3(kOtbBlock), 0, st, h->lev, h->tau, sidx, h->sched, word, h->bcount, h->n, L);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(otb_list_scan_kernel, dim3(1), dim3(kOtbBlock), 0, st, h->bcount, h->sched, h->pin_dev, h->strips, publish ? 1 : 0);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(otb_list_compact_kernel, dim3(h->strips), dim3(kOtbBlock), 0, st, h->lev, h->tau, sidx, h->sched, h->bcount, out, h->n, L);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// one block step; *n_active and *tau_next are always written on success
template <typename T, int D>
static int otb_step_launch(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, const otb_consts<T>& bc, double theta,
                           hipStream_t st, uint32_t* n_active, uint32_t* tau_next) {
  const int32_t L  = h->levels;
  const uint32_t n = h->n;
  T* xp            = static_cast<T*>(h->xp);
  T* a1            = static_cast<T*>(h->a1);
  hipLaunchKernelGGL(otb_sched_min_kernel, dim3(h->strips), dim3(kOtbBlock), 0, st, h->lev, h->tau, h->sched, n, L);
  NB_HIP(hipGetLastError());
  if (int r = otb_list(h, nullptr, h->act, kOtbMin, true, st)) return r;
  hipLaunchKernelGGL((otb_predict_kernel<T, D>), dim3((n * uint32_t(D) + kOtbBlock - 1) / kOtbBlock), dim3(kOtbBlock), 0, st,
                     static_cast<const T*>(s->x), static_cast<const T*>(s->v), static_cast<const T*>(s->a), h->tau, h->sched, xp, bc.tick,
                     n * uint32_t(D));
  NB_HIP(hipGetLastError());
  nbody_state sp = *s;  // the predicted system: the tree is built on it and the walk reads its positions
  sp.x           = xp;
  if (int r = otb_build<T, D>(t, &sp, st)) return r;
  if (int r = otb_list(h, t->idx[t->sorted_buf], h->wlist, kOtbNext, false, st)) return r;
  NB_HIP(hipStreamSynchronize(st));
  const uint32_t n_act = h->pin[0], next = h->pin[1];
  if (n_act < 1u || n_act > n || next < 1u || next > (1u << L)) {
    h->on = false;
    set_error("nbody_octree_block_step: the schedule on the device is not one of this handle (n_act = %u of %u, tau_next = %u of %u)",
              n_act, n, next, 1u << L);
    return NBODY_ERR_STATE;
  }
  {  // the softened walk of ot_force_run, over the walk list, from xp into a1
    const uint32_t per_wave = 64u >> D;
    const uint32_t blocks   = (n_act + per_wave - 1) / per_wave;
    const uint32_t budget   = t->step_budget ? t->step_budget : t->capacity;
#define NB_OTB_WALK(CNT)                                                                                                               \
  hipLaunchKernelGGL((ot_force_softened_kernel<T, D, CNT>), dim3(blocks), dim3(64), 0, st, static_cast<const ot_node<T>*>(t->rootrec), \
                     static_cast<const ot_group<T, D>*>(t->groups), h->wlist, n_act, static_cast<const T*>(xp), a1,                    \
                     static_cast<T>(s->c), 0u, static_cast<T>(theta), budget, static_cast<const T*>(t->root),                          \
                     t->lvl_count + ((D == 3 ? kMaxLevels<3> : kMaxLevels<2>) + 2), t->counters, bc.e2)
    if (t->counters_on) NB_OTB_WALK(true);
    else NB_OTB_WALK(false);
#undef NB_OTB_WALK
    NB_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL((otb_kick_kernel<T, D>), dim3((n_act + kOtbBlock - 1) / kOtbBlock), dim3(kOtbBlock), 0, st, h->act, h->sched, xp, a1,
                     static_cast<T*>(s->x), static_cast<T*>(s->v), static_cast<T*>(s->a), h->lev, h->tau, bc.k, bc.tick, n_act, n, L);
  NB_HIP(hipGetLastError());
  h->last    = n_act;
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
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    otb_consts<T> bc;
    hipStream_t st = as_stream(stream);
    if (int r = otb_check<T>(h, t, s, eps, eta, is_start, max_level, st, who, &bc)) return r;
    device_guard guard(h->device);
    if (is_start) return otb_start_launch<T, D>(h, t, s, bc, theta, max_level, st);
    uint32_t na = 0, tn = 0;
    uint64_t nsteps = 0, nbody = 0;
    do {
      if (int r = otb_step_launch<T, D>(h, t, s, bc, theta, st, &na, &tn)) return r;
      ++nsteps;
      nbody += na;
    } while (steps && tn != (1u << h->levels));
    if (n_active) *n_active = na;
    if (tau) *tau = tn;
    if (steps) {
      steps[0] = nsteps;
      steps[1] = nbody;
    }
    return int(NBODY_OK);
  });
}

}  // namespace nbody

extern "C" int nbody_octree_block_create(nbody_octree_block** out, int dtype, int dim, uint32_t n) {
  return nbody_octree_block_create_on(out, dtype, dim, n, -1);
}

extern "C" int nbody_octree_block_create_on(nbody_octree_block** out, int dtype, int dim, uint32_t n, int device) {
  NB_ARG(out != nullptr, "out is NULL");
  *out = nullptr;
  NB_ARG(dtype == NBODY_F32 || dtype == NBODY_F64, "bad dtype %d", dtype);
  NB_ARG(dim == 2 || dim == 3, "bad dim %d", dim);
  NB_ARG(n >= 1 && n <= (1u << 28), "octree block steps need 1 <= n <= 2^28 (got %u)", n);
  if (captures_on_this_thread() != 0) {
    set_error("nbody_octree_block_create allocates: it cannot be called between nbody_graph_begin and nbody_graph_end");
    return NBODY_ERR_STATE;
  }
  int ndev = 0;
  NB_HIP(hipGetDeviceCount(&ndev));
  if (device < 0) device = current_device();
  NB_ARG(device >= 0 && device < ndev, "device %d out of range (%d HIP devices visible)", device, ndev);
  device_guard guard(device);
  auto* h   = new nbody_octree_block;
  h->device = device;
  h->dtype  = dtype;
  h->dim    = dim;
  h->n      = n;
  h->tsz    = dtype == NBODY_F32 ? 4 : 8;
  h->strips = uint32_t((size_t(n) + kOtbStrip - 1) / kOtbStrip);
  const size_t rows = h->tsz * size_t(dim) * size_t(n);
  hipError_t e      = hipMalloc(reinterpret_cast<void**>(&h->lev), sizeof(int32_t) * size_t(n));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->tau), sizeof(uint32_t) * size_t(n));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->act), sizeof(uint32_t) * size_t(n));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->wlist), sizeof(uint32_t) * size_t(n));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->bcount), sizeof(uint32_t) * h->strips);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->sched), sizeof(uint32_t) * kOtbWords);
  if (e == hipSuccess) e = hipMalloc(&h->xp, rows);
  if (e == hipSuccess) e = hipMalloc(&h->a1, rows);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&h->pin), sizeof(uint32_t) * 2, hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->pin_dev), h->pin, 0);
  // nothing is cleared: start writes lev, tau and the schedule words, and every block step writes xp, the lists and the listed rows
  // of a1 before it reads them
  if (e != hipSuccess) {
    int r = hip_fail(e, "nbody_octree_block_create allocation", __FILE__, __LINE__);
    nbody_octree_block_destroy(h);
    return r;
  }
  *out = h;
  return NBODY_OK;
}

extern "C" void nbody_octree_block_destroy(nbody_octree_block* h) {
  if (!h) return;
  device_guard guard(h->device);
  (void)hipFree(h->lev);
  (void)hipFree(h->tau);
  (void)hipFree(h->act);
  (void)hipFree(h->wlist);
  (void)hipFree(h->bcount);
  (void)hipFree(h->sched);
  (void)hipFree(h->xp);
  (void)hipFree(h->a1);
  if (h->pin) (void)hipHostFree(h->pin);
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
  const size_t need = what == 3 ? h->tsz * size_t(h->dim) * size_t(h->n) : 4 * size_t(what == 2 ? h->last : h->n);
  NB_ARG(bytes == need, "nbody_octree_block_read(what = %d) needs %zu bytes, got %zu", what, need, bytes);
  const void* src = what == 0 ? static_cast<const void*>(h->lev) : what == 1 ? static_cast<const void*>(h->tau) : what == 2 ? h->act : h->xp;
  if (need) NB_HIP(hipMemcpyAsync(host_out, src, need, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}
